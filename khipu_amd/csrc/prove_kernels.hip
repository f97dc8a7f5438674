// kh_trie_prove and kh_verify_proofs: their kernels (prove.h holds the bodies), then the host
// driver and the C entry points (host.h).  A cold compilation unit of its own like
// export_kernels.hip: the hot kernels of khst.hip keep their placement (tests/test_code_layout.py).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "prove.h"
#include "host.h"

using namespace khst;

// Count: one thread per key; the hits of its proof (64-bit: the scan of n < 2^31 keys of up to
// 130 hits each does not fit 32 bits) and whether the key is present.
__global__ void __launch_bounds__(BS) k_prove_count(AMap M, Recs R, const uint64_t* K, const uint32_t* trie,
                                                    uint64_t n, uint64_t* cnt, uint8_t* found) {
  const uint64_t i = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (i >= n) return;
  uint64_t c = 0;
  found[i] = prove_walk(M, R, trie ? trie[i] : 0u, K + 4 * i, [&](uint64_t) { ++c; });
  cnt[i] = c;
}
// Fill: the same walk, the hits of key i written at pos[i] (the exclusive scan of the counts);
// a walk never writes past its own count.
__global__ void __launch_bounds__(BS) k_prove_fill(AMap M, Recs R, const uint64_t* K, const uint32_t* trie,
                                                   uint64_t n, const uint64_t* pos, uint64_t* hits) {
  const uint64_t i = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (i >= n) return;
  uint64_t at = pos[i];
  const uint64_t end = pos[i + 1];
  prove_walk(M, R, trie ? trie[i] : 0u, K + 4 * i, [&](uint64_t h) {
    if (at < end) hits[at] = h;
    ++at;
  });
}
__global__ void __launch_bounds__(BS) k_prove_iota(uint32_t* v, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (i < n) v[i] = (uint32_t)i;
}
// KH_PROVE_SHARED, over the sorted hits: first[i] = 1 where a new (record, node) starts ...
__global__ void __launch_bounds__(BS) k_prove_first(const uint64_t* sorted, uint64_t n, uint32_t* first) {
  const uint64_t i = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (i < n) first[i] = i == 0 || sorted[i] != sorted[i - 1];
}
// ... and, rank the exclusive scan of first: the distinct hits packed in order, and every hit's
// place in that table scattered back to where the hit stood in the proofs (src)
__global__ void __launch_bounds__(BS) k_prove_rank(const uint64_t* sorted, const uint32_t* src, const uint32_t* first,
                                                   const uint32_t* rank, uint64_t n, uint64_t* table,
                                                   uint32_t* path_idx) {
  const uint64_t i = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (i >= n) return;
  const uint32_t f = first[i], u = rank[i] + f - 1;
  if (f) table[u] = sorted[i];
  path_idx[src[i]] = u;
}

// Verification: one thread per key walks its listed nodes (hashed beforehand, once per table
// node); the value's place in the table and its length for the copy.
__global__ void __launch_bounds__(BS) k_proof_walk(ProofTable T, const uint8_t* roots, uint64_t nroots,
                                                   const uint8_t* keys, const uint32_t* path_idx,
                                                   const uint64_t* path_off, uint64_t n, uint8_t* status,
                                                   uint64_t* vsrc, uint64_t* vlen) {
  const uint64_t i = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (i >= n) return;
  const uint8_t* val;
  uint32_t vl;
  const uint64_t p0 = path_off[i];
  status[i] = proof_walk(T, roots + (nroots == 1 ? 0 : 32 * i), keys + 32 * i, path_idx + p0, path_off[i + 1] - p0,
                         &val, &vl);
  vsrc[i] = vl ? (uint64_t)(val - T.rlp) : 0;
  vlen[i] = vl;
}
__global__ void __launch_bounds__(BS) k_proof_copy(const uint8_t* rlp, const uint64_t* vsrc, const uint64_t* vlen,
                                                   const uint64_t* voff, uint64_t n, uint8_t* out) {
  const uint64_t i = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (i >= n) return;
  const uint8_t* src = rlp + vsrc[i];
  uint8_t* dst = out + voff[i];
  for (uint64_t b = 0, L = vlen[i]; b < L; ++b) dst[b] = src[b];
}

// ---------------------------------------------------------------------------
// host: Merkle proofs and their verifier (prove.h)
// ---------------------------------------------------------------------------
// The proofs of n keys (host buffers).  Count walk, 64-bit scan, fill walk (the same body), for
// KH_PROVE_SHARED a sort of the hits with an adjacent-unique pass, then the export kernels in
// list mode over the hits.  Hit counts and encoding bytes are scanned in 64 bits: n < 2^31 keys
// of up to 130 nodes of up to 532 B pass 2^32 either way; the listed nodes of a call are capped at
// 2^32 - 1 (path_idx is 32 bits wide).
static int trie_prove(kh_trie* h, const uint32_t* trie, const uint8_t* keys, uint32_t klen, uint64_t n, uint32_t flags,
                      uint8_t* found, uint8_t* hashes32, uint64_t node_cap, uint8_t* rlp, uint64_t rlp_cap,
                      uint64_t* off, uint32_t* path_idx, uint64_t path_cap, uint64_t* path_off, uint64_t* n_nodes,
                      uint64_t* rlp_len, uint64_t* n_path) {
  trie_settle(h);
  kh_ctx* c = h->c;
  hipStream_t st = c->st;
  // KH_PROVE_TRIE_KEYS: the keys are trie keys already (a range scan's), never hashed
  const bool hash = (h->flags & KH_HASH_KEYS) && !(flags & KH_PROVE_TRIE_KEYS);
  query_check(h, trie, klen, n, hash);
  *n_nodes = *rlp_len = *n_path = 0;
  if (n == 0) {
    path_off[0] = 0;
    if (off) off[0] = 0;
    return KH_OK;
  }
  const bool shared = (flags & KH_PROVE_SHARED) != 0;
  // the keys and trie ids staged, the keys hashed as a commit hashes them
  uint8_t* dk;
  uint32_t* dt;
  stage_query_keys(c, trie, keys, klen, n, dk, dt);
  Layout L1;
  uint64_t *K, *pos, *tot;
  uint8_t* fnd;
  char* scr1;
  L1.add(K, n * 4 + 8);
  L1.add(pos, n + 1);
  L1.add(fnd, n);
  L1.add(scr1, scan_scratch_size(n + 1, 8));
  L1.add(tot, 8);
  place(h->gbuf, L1);
  if (hash) {
    hash_keys_to(st, (const uint8_t*)dk, klen, n, K);
  } else {
    HIPCHK(hipMemcpyAsync(K, dk, n * 32, hipMemcpyDeviceToDevice, st));
  }
  const bool any = h->rn && h->mcap;  // (else an empty trie or forest: every proof is empty)
  const Recs R = recs_of(h);
  const uint8_t* heap = (const uint8_t*)h->heap.p;
  if (any) {
    hipLaunchKernelGGL(k_prove_count, GRID(n, BS), dim3(BS), 0, st, map_of(h), R, (const uint64_t*)K,
                       (const uint32_t*)dt, n, pos, fnd);
    LAUNCH_CHECK();
  } else {
    HIPCHK(hipMemsetAsync(pos, 0, n * 8, st));
    HIPCHK(hipMemsetAsync(fnd, 0, n, st));
  }
  scan_u64(pos, pos, n, tot, scr1, st);
  HIPCHK(hipMemcpyAsync(pos + n, tot, 8, hipMemcpyDeviceToDevice, st));
  HIPCHK(hipMemcpyAsync(c->h_pinned, tot, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  const uint64_t np = c->h_pinned[0];
  if (np >= (1ULL << 32)) throw KhError{KH_EINVAL, "the proofs list 2^32 nodes or more: prove fewer keys a call"};
  // the hits in proof order, then the node table's hit list (shared: the distinct hits, sorted)
  Layout L2;
  uint64_t *hits, *hits2, *table;
  uint32_t *src, *src2, *first, *rank, *pidx, *utot;
  char *rscr, *scr2;
  L2.add(hits, np + 1);
  L2.add(pidx, np + 1);
  L2.add(hits2, np + 1, shared);
  L2.add(table, np + 1, shared);
  L2.add(src, np + 1, shared);
  L2.add(src2, np + 1, shared);
  L2.add(first, np + 1, shared);
  L2.add(rank, np + 1, shared);
  L2.add(rscr, radix_scratch_size(np + 1), shared);
  L2.add(scr2, scan_scratch_size(np + 1, 4), shared);
  L2.add(utot, 4);
  place(c->ws1, L2);
  uint64_t nn = np;
  const uint64_t* list = hits;
  if (np) {
    hipLaunchKernelGGL(k_prove_fill, GRID(n, BS), dim3(BS), 0, st, map_of(h), R, (const uint64_t*)K, (const uint32_t*)dt,
                       n, (const uint64_t*)pos, hits);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(k_prove_iota, GRID(np, BS), dim3(BS), 0, st, shared ? src : pidx, np);
    LAUNCH_CHECK();
    if (shared) {
      // a hit is 2 * record + which < 2^33: five 8-bit digits
      const bool flip = sort_pairs_u64(hits, src, hits2, src2, np, 0, 40, rscr, st);
      const uint64_t* sk = flip ? hits2 : hits;
      const uint32_t* sv = flip ? src2 : src;
      hipLaunchKernelGGL(k_prove_first, GRID(np, BS), dim3(BS), 0, st, sk, np, first);
      LAUNCH_CHECK();
      scan_u32(first, rank, np, utot, scr2, st);
      hipLaunchKernelGGL(k_prove_rank, GRID(np, BS), dim3(BS), 0, st, sk, sv, (const uint32_t*)first,
                         (const uint32_t*)rank, np, table, pidx);
      LAUNCH_CHECK();
      HIPCHK(hipMemcpyAsync(c->h_pinned, utot, 4, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      nn = (uint32_t)c->h_pinned[0];
      list = table;
    }
  }
  // the table's encodings: sizes, 64-bit scan, write (list mode, one node an item)
  Layout L3;
  uint32_t *byt, *stash;
  uint64_t* tb;
  char* scr3;
  L3.add(byt, nn + 1);
  L3.add(stash, (nn + 1) * EXP_LANES);
  L3.add(scr3, scan_scratch_size(nn + 1, 8));
  L3.add(tb, 8);
  place(c->ws2, L3);
  // (the offsets scanned in place in the emitted set's off array, which the write pass reads)
  h->xbuf.ensure(nn * 32 + (nn + 1) * 8 + 2048);
  uint64_t* doff = (uint64_t*)((uint8_t*)h->xbuf.p + ((nn * 32 + 255) & ~255ULL));
  uint64_t total = 0;
  if (nn) {
    hipLaunchKernelGGL(k_export_sizes, GRID(nn * EXP_LANES, BS), dim3(BS), 0, st, map_of(h), R, heap, list, (uint64_t)0,
                       nn, EXP_ALL_TRIES, stash, (uint32_t*)nullptr, byt);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(k_u32_to_u64, GRID(nn, BS), dim3(BS), 0, st, (const uint32_t*)byt, nn, doff);
    LAUNCH_CHECK();
    scan_u64(doff, doff, nn, tb, scr3, st);
    HIPCHK(hipMemcpyAsync(doff + nn, tb, 8, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(c->h_pinned, tb, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    total = c->h_pinned[0];
  }
  *n_nodes = nn;
  *rlp_len = total;
  *n_path = np;
  if (nn > node_cap || total > rlp_cap || np > path_cap)
    return set_err(KH_ENOSPC, "proof output too small (*n_nodes / *rlp_len / *n_path hold the sizes needed)");
  if ((nn && (!hashes32 || !off)) || (total && !rlp) || (np && !path_idx))
    throw KhError{KH_EINVAL, "null output buffer"};
  if (nn) {
    DevBuf& enc = c->out_emit;  // the encodings (hashes and offsets: the handle's xbuf, above)
    enc.ensure(total + 1024);
    hipLaunchKernelGGL(k_export_write, GRID(nn * EXP_LANES, BS), dim3(BS), 0, st, R, heap, list, (uint64_t)0, nn,
                       EXP_ALL_TRIES, (const uint32_t*)stash, (const uint32_t*)nullptr, (const uint32_t*)nullptr,
                       (uint8_t*)h->xbuf.p, (uint8_t*)enc.p, doff, (uint8_t*)nullptr, (const uint64_t*)doff);
    LAUNCH_CHECK();
    HIPCHK(hipMemcpyAsync(hashes32, h->xbuf.p, nn * 32, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(off, doff, (nn + 1) * 8, hipMemcpyDeviceToHost, st));
    if (total) HIPCHK(hipMemcpyAsync(rlp, enc.p, total, hipMemcpyDeviceToHost, st));
  } else if (off) {
    off[0] = 0;
  }
  if (np) HIPCHK(hipMemcpyAsync(path_idx, pidx, np * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(path_off, pos, (n + 1) * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(found, fnd, n, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return KH_OK;
}

// The proofs of n keys checked (host buffers, the shared context): the table's nodes hashed once
// each, one walk per key, the values packed.
static int verify_proofs(const uint8_t* roots32, uint64_t nroots, const uint8_t* keys, uint32_t klen, uint64_t n,
                         uint32_t flags, const uint8_t* rlp, const uint64_t* off, uint64_t n_nodes,
                         const uint32_t* path_idx, const uint64_t* path_off, uint8_t* status, uint8_t* vals,
                         uint64_t val_cap, uint64_t* voff, uint64_t* val_bytes) {
  if (val_bytes) *val_bytes = 0;
  if (n == 0) {
    voff[0] = 0;
    return KH_OK;
  }
  for (uint64_t j = 0; j < n_nodes; ++j) {
    if (off[j + 1] < off[j]) throw KhError{KH_EINVAL, "node offsets must not decrease"};
    if (off[j + 1] - off[j] > 0xFFFFFFFFull) throw KhError{KH_EINVAL, "a node longer than 2^32 - 1 bytes"};
  }
  for (uint64_t i = 0; i < n; ++i)
    if (path_off[i + 1] < path_off[i]) throw KhError{KH_EINVAL, "path offsets must not decrease"};
  const uint64_t p0 = path_off[0], np = path_off[n] - p0;
  const uint64_t b0 = n_nodes ? off[0] : 0, nb = n_nodes ? off[n_nodes] - b0 : 0;
  if ((np && !path_idx) || (nb && !rlp)) throw KhError{KH_EINVAL, "null buffer"};
  kh_ctx* c = shared_ctx(current_device());
  std::lock_guard<std::recursive_mutex> g(c->mu);
  HIPCHK(hipSetDevice(c->dev));
  hipStream_t st = c->st;
  std::vector<uint64_t> roff(n_nodes + 1, 0), rpo(n + 1);
  for (uint64_t j = 0; j <= n_nodes && n_nodes; ++j) roff[j] = off[j] - b0;
  for (uint64_t i = 0; i <= n; ++i) rpo[i] = path_off[i] - p0;
  Layout Li;
  uint8_t *dk, *droots, *drlp;
  uint64_t *doff, *dpo;
  uint32_t* dpi;
  Li.add(dk, n * klen + 64);
  Li.add(droots, nroots * 32);
  Li.add(drlp, nb + 64);
  Li.add(doff, n_nodes + 1);
  Li.add(dpi, np + 1);
  Li.add(dpo, n + 1);
  place(c->in_keys, Li);
  HIPCHK(hipMemcpyAsync(dk, keys, n * klen, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(droots, roots32, nroots * 32, hipMemcpyHostToDevice, st));
  if (nb) HIPCHK(hipMemcpyAsync(drlp, rlp + b0, nb, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(doff, roff.data(), (n_nodes + 1) * 8, hipMemcpyHostToDevice, st));
  if (np) HIPCHK(hipMemcpyAsync(dpi, path_idx + p0, np * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(dpo, rpo.data(), (n + 1) * 8, hipMemcpyHostToDevice, st));
  Layout Lw;
  uint64_t *K, *nh, *vsrc, *vlen, *dvoff, *tot;
  uint8_t* dst;
  char* scr;
  Lw.add(K, n * 4 + 8);
  Lw.add(nh, n_nodes * 4 + 4);
  Lw.add(vsrc, n);
  Lw.add(vlen, n + 1);
  Lw.add(dvoff, n + 1);
  Lw.add(dst, n);
  Lw.add(scr, scan_scratch_size(n + 1, 8));
  Lw.add(tot, 8);
  place(c->ws1, Lw);
  if (flags & KH_HASH_KEYS) {
    hash_keys_to(st, (const uint8_t*)dk, klen, n, K);
  } else {
    HIPCHK(hipMemcpyAsync(K, dk, n * 32, hipMemcpyDeviceToDevice, st));
  }
  if (n_nodes) {
    hipLaunchKernelGGL(k_kec_batch, GRID(n_nodes, BS), dim3(BS), 0, st, (const uint8_t*)drlp, (const uint64_t*)doff,
                       n_nodes, nh);
    LAUNCH_CHECK();
  }
  const ProofTable T{drlp, doff, nh, n_nodes};
  hipLaunchKernelGGL(k_proof_walk, GRID(n, BS), dim3(BS), 0, st, T, (const uint8_t*)droots, nroots, (const uint8_t*)K,
                     (const uint32_t*)dpi, (const uint64_t*)dpo, n, dst, vsrc, vlen);
  LAUNCH_CHECK();
  scan_u64(vlen, dvoff, n, tot, scr, st);
  HIPCHK(hipMemcpyAsync(dvoff + n, tot, 8, hipMemcpyDeviceToDevice, st));
  HIPCHK(hipMemcpyAsync(c->h_pinned, tot, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  const uint64_t total = c->h_pinned[0];
  if (val_bytes) *val_bytes = total;
  if (total > val_cap || (total && !vals))
    return set_err(KH_ENOSPC, "value output too small (*val_bytes holds the size needed)");
  c->out_emit.ensure(total + 64);
  if (total) {
    hipLaunchKernelGGL(k_proof_copy, GRID(n, BS), dim3(BS), 0, st, (const uint8_t*)drlp, (const uint64_t*)vsrc,
                       (const uint64_t*)vlen, (const uint64_t*)dvoff, n, (uint8_t*)c->out_emit.p);
    LAUNCH_CHECK();
    HIPCHK(hipMemcpyAsync(vals, c->out_emit.p, total, hipMemcpyDeviceToHost, st));
  }
  HIPCHK(hipMemcpyAsync(status, dst, n, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(voff, dvoff, (n + 1) * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return KH_OK;
}

extern "C" {

int kh_trie_prove(kh_trie* h, const uint32_t* trie, const uint8_t* keys, uint32_t klen, uint64_t n, uint32_t flags,
                  uint8_t* found, uint8_t* hashes32, uint64_t node_cap, uint8_t* rlp, uint64_t rlp_cap, uint64_t* off,
                  uint32_t* path_idx, uint64_t path_cap, uint64_t* path_off, uint64_t* n_nodes, uint64_t* rlp_len,
                  uint64_t* n_path) {
  if (!h || !path_off || !n_nodes || !rlp_len || !n_path) return set_err(KH_EINVAL, "null handle or outputs");
  if (flags & ~(KH_PROVE_SHARED | KH_PROVE_TRIE_KEYS)) return set_err(KH_EINVAL, "unknown prove flag");
  if (n && (!keys || !found)) return set_err(KH_EINVAL, "null buffer");
  API_TRY({
    HANDLE_LOCK(h);
    HIPCHK(hipSetDevice(h->c->dev));
    return trie_prove(h, trie, keys, klen, n, flags, found, hashes32, node_cap, rlp, rlp_cap, off, path_idx, path_cap,
                      path_off, n_nodes, rlp_len, n_path);
  })
}

int kh_verify_proofs(const uint8_t* roots32, uint64_t nroots, const uint8_t* keys, uint32_t klen, uint64_t n,
                     uint32_t flags, const uint8_t* rlp, const uint64_t* off, uint64_t n_nodes, const uint32_t* path_idx,
                     const uint64_t* path_off, uint8_t* status, uint8_t* vals, uint64_t val_cap, uint64_t* voff,
                     uint64_t* val_bytes) {
  if (!voff) return set_err(KH_EINVAL, "null value offsets");
  if (flags & ~KH_HASH_KEYS) return set_err(KH_EINVAL, "unknown verify flag");
  if (!(flags & KH_HASH_KEYS) && klen != 32) return set_err(KH_EINVAL, "keys must be 32 bytes unless KH_HASH_KEYS");
  if (klen == 0 || klen > 4096) return set_err(KH_EINVAL, "bad key length");
  if (n >= (1ULL << 31) || n_nodes >= (1ULL << 32)) return set_err(KH_EINVAL, "batch too large");
  if (nroots != 1 && nroots != n) return set_err(KH_EINVAL, "one root, or one root per key");
  if (n && (!roots32 || !keys || !status || !path_off || (n_nodes && !off))) return set_err(KH_EINVAL, "null buffer");
  API_TRY({
    return verify_proofs(roots32, nroots, keys, klen, n, flags, rlp, off, n_nodes, path_idx, path_off, status, vals,
                         val_cap, voff, val_bytes);
  })
}

}  // extern "C"
