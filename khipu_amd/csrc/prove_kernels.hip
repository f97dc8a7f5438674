// kh_trie_prove, kh_verify_proofs and kh_trie_commit_witness_host: their kernels (prove.h and
// witness.h hold the bodies), then the host drivers and the C entry points (host.h).  A cold
// compilation unit of its own like export_kernels.hip: the hot kernels of khst.hip keep their
// placement (tests/test_code_layout.py).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "witness.h"
#include "host.h"
#include "wave.h"

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

// ---- commit witnesses (witness.h).  The ops are the upserts [0, nup) then the deletes [nup, n).
// the deletes into their set, one thread each
__global__ void __launch_bounds__(BS) k_wit_dels(WDels D, const uint64_t* K, const uint32_t* T, uint64_t nup,
                                                 uint64_t n) {
  const uint64_t i = nup + (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (i < n) wdels_insert(D, K, T, i);
}
// Count: the hits of op i's walk, and the records all walks visit (nvis: sizes the visited set)
__global__ void __launch_bounds__(BS) k_wit_count(AMap M, Recs R, const uint64_t* K, const uint32_t* T, uint64_t n,
                                                  uint64_t* cnt, unsigned long long* nvis) {
  const uint64_t i = (uint64_t)blockIdx.x * BS + threadIdx.x;
  unsigned long long v = 0;
  if (i < n) {
    uint64_t c = 0;
    wit_walk(M, R, T ? T[i] : 0u, K + 4 * i, [&](uint64_t) { ++c; }, [&](uint32_t, uint32_t) { ++v; });
    cnt[i] = c;
  }
  wave_atomic_add(nvis, v);  // (every lane of the wave is here: one atomic a wave)
}
// the (trie id, hash to fetch) pairs of a refusal, at claimed places; cnt counts them all
struct WMiss {
  uint32_t* trie;
  uint64_t* hash;
  unsigned long long* cnt;
  uint64_t cap;
};
__device__ __forceinline__ void wit_miss(const Recs& R, const WMiss& X, uint32_t r) {
  const unsigned long long t = atomicAdd(X.cnt, 1ULL);
  if (t >= X.cap) return;
  X.trie[t] = R.rt[r];
  for (int q = 0; q < 4; ++q) X.hash[4 * t + q] = R.rbref[4ull * r + q];
}
// Fill: the same walk, its hits at pos[i], its marks into the visited set; the stubs reached
__global__ void __launch_bounds__(BS) k_wit_fill(AMap M, Recs R, WSet V, WDels D, bool join, const uint64_t* K,
                                                 const uint32_t* T, uint64_t nup, uint64_t n, const uint64_t* pos,
                                                 uint64_t* hits, WMiss X) {
  const uint64_t i = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (i >= n) return;
  const uint32_t t = T ? T[i] : 0u;
  const uint64_t* key = K + 4 * i;
  const bool del = i >= nup;
  const bool up = !del && !(join && wdels_has(D, K, T, t, key));  // (a key also deleted is a delete)
  uint64_t at = pos[i];
  const uint64_t end = pos[i + 1];
  wit_op(
      M, R, V, t, key, up, del,
      [&](uint64_t h) {
        if (at < end) hits[at] = h;
        ++at;
      },
      [&](uint32_t r) { wit_miss(R, X, r); });
}
// the visited branch records by branch depth: a 64-bin histogram, the bins' starts, the slots
// scattered into their bins (any order inside a bin)
__global__ void __launch_bounds__(BS) k_wit_bins(WSet V, Recs R, unsigned long long* hist) {
  const uint64_t s = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (s > V.mask) return;
  const uint32_t r = V.rec[s];
  if (r != NONE && wit_is_branch(R, r)) atomicAdd(&hist[R.rdb[r]], 1ULL);
}
__global__ void k_wit_starts(const unsigned long long* hist, unsigned long long* cur) {
  if (blockIdx.x || threadIdx.x) return;
  unsigned long long at = 0;
  for (int d = 0; d < 64; ++d) {
    cur[d] = at;
    at += hist[d];
  }
}
__global__ void __launch_bounds__(BS) k_wit_scatter(WSet V, Recs R, unsigned long long* cur, uint32_t* blist,
                                                    uint64_t cap) {
  const uint64_t s = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (s > V.mask) return;
  const uint32_t r = V.rec[s];
  if (r == NONE || !wit_is_branch(R, r)) return;
  const unsigned long long p = atomicAdd(&cur[R.rdb[r]], 1ULL);
  if (p < cap) blist[p] = (uint32_t)s;
}
// one depth's visited branches judged (deepest first, a launch a depth): the collapse children
// appended to the hits past the walks' (ncol counts them; hits holds room for one per branch)
__global__ void __launch_bounds__(BS) k_wit_eval(AMap M, Recs R, WSet V, const uint32_t* blist, uint64_t lo,
                                                 uint64_t cnt, uint64_t* hits, uint64_t np, uint64_t hcap,
                                                 unsigned long long* ncol, WMiss X) {
  const uint64_t i = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (i >= cnt) return;
  wit_eval(
      M, R, V, blist[lo + i],
      [&](uint64_t h) {
        const unsigned long long p = np + atomicAdd(ncol, 1ULL);
        if (p < hcap) hits[p] = h;
      },
      [&](uint32_t r) { wit_miss(R, X, r); });
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
// What kh_trie_prove and kh_trie_commit_witness_host do with their hits, once each:
// the arrays of np hits (shared: with the sort's and the adjacent-unique pass's)
struct HitBufs {
  uint64_t *hits, *hits2, *table;
  uint32_t *src, *src2, *first, *rank, *pidx, *utot;
  char *rscr, *scr2;
  void declare(Layout& L, uint64_t np, bool shared) {
    L.add(hits, np + 1);
    L.add(pidx, np + 1);
    L.add(hits2, np + 1, shared);
    L.add(table, np + 1, shared);
    L.add(src, np + 1, shared);
    L.add(src2, np + 1, shared);
    L.add(first, np + 1, shared);
    L.add(rank, np + 1, shared);
    L.add(rscr, radix_scratch_size(np + 1), shared);
    L.add(scr2, scan_scratch_size(np + 1, 4), shared);
    L.add(utot, 4);
  }
};
// KH_PROVE_SHARED: the np hits sorted, the distinct ones packed in order (the node table's list,
// returned; nn their number) and every hit's place in it left in H.pidx.  One sync.
static const uint64_t* hits_share(kh_ctx* c, const HitBufs& H, uint64_t np, uint64_t& nn) {
  hipStream_t st = c->st;
  hipLaunchKernelGGL(k_prove_iota, GRID(np, BS), dim3(BS), 0, st, H.src, np);
  LAUNCH_CHECK();
  // a hit is 2 * record + which < 2^33: five 8-bit digits
  const bool flip = sort_pairs_u64(H.hits, H.src, H.hits2, H.src2, np, 0, 40, H.rscr, st);
  const uint64_t* sk = flip ? H.hits2 : H.hits;
  const uint32_t* sv = flip ? H.src2 : H.src;
  hipLaunchKernelGGL(k_prove_first, GRID(np, BS), dim3(BS), 0, st, sk, np, H.first);
  LAUNCH_CHECK();
  scan_u32(H.first, H.rank, np, H.utot, H.scr2, st);
  hipLaunchKernelGGL(k_prove_rank, GRID(np, BS), dim3(BS), 0, st, sk, sv, (const uint32_t*)H.first,
                     (const uint32_t*)H.rank, np, H.table, H.pidx);
  LAUNCH_CHECK();
  HIPCHK(hipMemcpyAsync(c->h_pinned, H.utot, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  nn = (uint32_t)c->h_pinned[0];
  return H.table;
}
// the table's encodings: sizes, 64-bit scan (list mode, one node an item); returns their bytes.
// One sync.
struct HitSizes {
  uint32_t* stash;
  uint64_t* doff;
};
static uint64_t hits_sizes(kh_trie* h, const uint64_t* list, uint64_t nn, HitSizes& Z) {
  kh_ctx* c = h->c;
  hipStream_t st = c->st;
  Layout L3;
  uint32_t* byt;
  uint64_t* tb;
  char* scr3;
  L3.add(byt, nn + 1);
  L3.add(Z.stash, (nn + 1) * EXP_LANES);
  L3.add(scr3, scan_scratch_size(nn + 1, 8));
  L3.add(tb, 8);
  place(c->ws2, L3);
  // (the offsets scanned in place in the emitted set's off array, which the write pass reads)
  h->xbuf.ensure(nn * 32 + (nn + 1) * 8 + 2048);
  Z.doff = (uint64_t*)((uint8_t*)h->xbuf.p + ((nn * 32 + 255) & ~255ULL));
  if (!nn) return 0;
  hipLaunchKernelGGL(k_export_sizes, GRID(nn * EXP_LANES, BS), dim3(BS), 0, st, map_of(h), recs_of(h),
                     (const uint8_t*)h->heap.p, list, (uint64_t)0, nn, EXP_ALL_TRIES, Z.stash, (uint32_t*)nullptr, byt);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(k_u32_to_u64, GRID(nn, BS), dim3(BS), 0, st, (const uint32_t*)byt, nn, Z.doff);
  LAUNCH_CHECK();
  scan_u64(Z.doff, Z.doff, nn, tb, scr3, st);
  HIPCHK(hipMemcpyAsync(Z.doff + nn, tb, 8, hipMemcpyDeviceToDevice, st));
  HIPCHK(hipMemcpyAsync(c->h_pinned, tb, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return c->h_pinned[0];
}
// ... and the write pass: hashes, offsets and encodings to the host buffers (copies left in flight)
static void hits_write(kh_trie* h, const uint64_t* list, uint64_t nn, uint64_t total, const HitSizes& Z,
                       uint8_t* hashes32, uint8_t* rlp, uint64_t* off) {
  kh_ctx* c = h->c;
  hipStream_t st = c->st;
  if (nn) {
    DevBuf& enc = c->out_emit;  // the encodings (hashes and offsets: the handle's xbuf, above)
    enc.ensure(total + 1024);
    hipLaunchKernelGGL(k_export_write, GRID(nn * EXP_LANES, BS), dim3(BS), 0, st, recs_of(h), (const uint8_t*)h->heap.p,
                       list, (uint64_t)0, nn, EXP_ALL_TRIES, (const uint32_t*)Z.stash, (const uint32_t*)nullptr,
                       (const uint32_t*)nullptr, (uint8_t*)h->xbuf.p, (uint8_t*)enc.p, Z.doff, (uint8_t*)nullptr,
                       (const uint64_t*)Z.doff);
    LAUNCH_CHECK();
    HIPCHK(hipMemcpyAsync(hashes32, h->xbuf.p, nn * 32, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(off, Z.doff, (nn + 1) * 8, hipMemcpyDeviceToHost, st));
    if (total) HIPCHK(hipMemcpyAsync(rlp, enc.p, total, hipMemcpyDeviceToHost, st));
  } else if (off) {
    off[0] = 0;
  }
}

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
  HitBufs H;
  H.declare(L2, np, shared);
  place(c->ws1, L2);
  uint64_t* const hits = H.hits;
  uint32_t* const pidx = H.pidx;
  uint64_t nn = np;
  const uint64_t* list = hits;
  if (np) {
    hipLaunchKernelGGL(k_prove_fill, GRID(n, BS), dim3(BS), 0, st, map_of(h), R, (const uint64_t*)K, (const uint32_t*)dt,
                       n, (const uint64_t*)pos, hits);
    LAUNCH_CHECK();
    if (shared) {
      list = hits_share(c, H, np, nn);
    } else {
      hipLaunchKernelGGL(k_prove_iota, GRID(np, BS), dim3(BS), 0, st, pidx, np);
      LAUNCH_CHECK();
    }
  }
  HitSizes Z;
  const uint64_t total = hits_sizes(h, list, nn, Z);
  *n_nodes = nn;
  *rlp_len = total;
  *n_path = np;
  if (nn > node_cap || total > rlp_cap || np > path_cap)
    return set_err(KH_ENOSPC, "proof output too small (*n_nodes / *rlp_len / *n_path hold the sizes needed)");
  if ((nn && (!hashes32 || !off)) || (total && !rlp) || (np && !path_idx))
    throw KhError{KH_EINVAL, "null output buffer"};
  hits_write(h, list, nn, total, Z, hashes32, rlp, off);
  if (np) HIPCHK(hipMemcpyAsync(path_idx, pidx, np * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(path_off, pos, (n + 1) * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(found, fnd, n, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return KH_OK;
}

// The commit witness of a batch (host buffers; witness.h).  The ops staged and hashed as a commit's,
// the deletes into their set, count walk, 64-bit scan, fill walk into the visited set; the visited
// branches binned by depth (one sync: the hits, the visits and the stubs reached), one launch per
// depth present, deepest first; then kh_trie_prove's shared tail over the walks' hits and the
// collapse children.  Work and memory follow the ops and their walks.  Nothing of the handle is
// written: its records, map, roots, write-back set and missing list stay as they are.
static const char* const MSG_WIT_STUB =
    "the batch needs a node the handle does not hold (MPTNodeMissingException): the hashes are listed";
static uint64_t pow2_at_least(uint64_t v) {
  uint64_t p = 16;
  while (p < v) p <<= 1;
  return p;
}
static int wit_refuse(kh_ctx* c, const WMiss& X, uint64_t k, uint32_t* miss_tries, uint8_t* miss_hashes32,
                      uint64_t miss_cap, uint64_t* n_missing) {
  *n_missing = k;
  const uint64_t w = std::min({k, miss_cap, X.cap});
  if (w) {
    HIPCHK(hipMemcpyAsync(miss_tries, X.trie, w * 4, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipMemcpyAsync(miss_hashes32, X.hash, w * 32, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
  }
  return set_err(KH_ENODE, MSG_WIT_STUB);
}
static int trie_commit_witness(kh_trie* h, const uint32_t* up_trie, const uint8_t* up_keys, uint64_t nup,
                               const uint32_t* del_trie, const uint8_t* del_keys, uint64_t ndel, uint32_t klen,
                               uint8_t* hashes32, uint64_t node_cap, uint8_t* rlp, uint64_t rlp_cap, uint64_t* off,
                               uint64_t* n_nodes, uint64_t* rlp_len, uint64_t* n_collapse, uint32_t* miss_tries,
                               uint8_t* miss_hashes32, uint64_t miss_cap, uint64_t* n_missing) {
  trie_settle(h);
  kh_ctx* c = h->c;
  hipStream_t st = c->st;
  const bool hash = (h->flags & KH_HASH_KEYS) != 0;
  if (nup >= (1ULL << 31) || ndel >= (1ULL << 31)) throw KhError{KH_EINVAL, "batch too large"};
  const uint64_t n = nup + ndel;
  if (h->forest && ((nup && !up_trie) || (ndel && !del_trie))) throw KhError{KH_EINVAL, "forest ops need trie ids"};
  query_check(h, nup ? up_trie : del_trie, klen, n, hash);
  auto nothing = [&] {
    *n_nodes = *rlp_len = *n_missing = 0;
    if (n_collapse) *n_collapse = 0;
    if (off) off[0] = 0;
    return KH_OK;
  };
  const bool any = h->rn && h->mcap;  // (else an empty trie or forest)
  if (n == 0 || !any) return nothing();
  // the keys and trie ids of both kinds staged as one list, the keys hashed as a commit hashes them
  std::vector<uint8_t> hk(n * klen);
  std::vector<uint32_t> ht(h->forest ? n : 0);
  if (nup) memcpy(hk.data(), up_keys, nup * klen);
  if (ndel) memcpy(hk.data() + nup * klen, del_keys, ndel * klen);
  if (h->forest && nup) memcpy(ht.data(), up_trie, nup * 4);
  if (h->forest && ndel) memcpy(ht.data() + nup, del_trie, ndel * 4);
  uint8_t* dk;
  uint32_t* dt;
  stage_query_keys(c, h->forest ? ht.data() : nullptr, hk.data(), klen, n, dk, dt);
  const bool join = nup && ndel;
  const uint64_t dcap = join ? pow2_at_least(2 * ndel) : 0;
  Layout L1;
  uint64_t *K, *pos, *tot;
  unsigned long long *ctr, *cur;  // ctr: [0] visits, [1] stubs listed, [2] collapse children, [8, 72) depth bins
  char* scr1;
  WDels D{};
  L1.add(K, n * 4 + 8);
  L1.add(pos, n + 1);
  L1.add(scr1, scan_scratch_size(n + 1, 8));
  L1.add(tot, 8);
  L1.add(ctr, 72);
  L1.add(cur, 64);
  L1.add(D.idx, dcap, join);
  place(h->gbuf, L1);
  D.mask = dcap ? dcap - 1 : 0;
  if (hash) {
    hash_keys_to(st, (const uint8_t*)dk, klen, n, K);
  } else {
    HIPCHK(hipMemcpyAsync(K, dk, n * 32, hipMemcpyDeviceToDevice, st));
  }
  HIPCHK(hipMemsetAsync(ctr, 0, 72 * 8, st));
  const Recs R = recs_of(h);
  const AMap M = map_of(h);
  if (join) {
    HIPCHK(hipMemsetAsync(D.idx, 0xFF, dcap * 4, st));
    hipLaunchKernelGGL(k_wit_dels, GRID(ndel, BS), dim3(BS), 0, st, D, (const uint64_t*)K, (const uint32_t*)dt, nup, n);
    LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_wit_count, GRID(n, BS), dim3(BS), 0, st, M, R, (const uint64_t*)K, (const uint32_t*)dt, n, pos,
                     ctr);
  LAUNCH_CHECK();
  scan_u64(pos, pos, n, tot, scr1, st);
  HIPCHK(hipMemcpyAsync(pos + n, tot, 8, hipMemcpyDeviceToDevice, st));
  HIPCHK(hipMemcpyAsync(c->h_pinned, tot, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(c->h_pinned + 1, ctr, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  const uint64_t np = c->h_pinned[0], nv = c->h_pinned[1];
  if (np + nv >= (1ULL << 31)) throw KhError{KH_EINVAL, "the walks visit 2^31 nodes or more: fewer ops a call"};
  if (np == 0) return nothing();  // (ids the forest does not hold, emptied tries)
  // the hits (a collapse child per visited branch at the most), the visited set, the branches by
  // depth and the refusal's list
  const uint64_t hcap = np + nv, vcap = pow2_at_least(2 * nv);
  const uint64_t xcap = std::min<uint64_t>(h->nstubs, std::max(n, nv));
  Layout L2;
  HitBufs H;
  WSet V{};
  WMiss X{};
  uint32_t* blist;
  H.declare(L2, hcap, true);
  L2.add_all(vcap, V.rec, V.st, V.mk);
  L2.add(blist, nv + 1);
  L2.add(X.trie, xcap);
  L2.add(X.hash, xcap * 4);
  place(c->ws1, L2);
  V.mask = vcap - 1;
  X.cnt = ctr + 1;
  X.cap = xcap;
  HIPCHK(hipMemsetAsync(V.rec, 0xFF, vcap * 4, st));
  HIPCHK(hipMemsetAsync(V.st, 0, vcap * 4, st));
  HIPCHK(hipMemsetAsync(V.mk, 0, vcap * 4, st));
  hipLaunchKernelGGL(k_wit_fill, GRID(n, BS), dim3(BS), 0, st, M, R, V, D, join, (const uint64_t*)K, (const uint32_t*)dt,
                     nup, n, (const uint64_t*)pos, H.hits, X);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(k_wit_bins, GRID(vcap, BS), dim3(BS), 0, st, V, R, ctr + 8);
  LAUNCH_CHECK();
  HIPCHK(hipMemcpyAsync(c->h_pinned, ctr, 72 * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (c->h_pinned[1]) return wit_refuse(c, X, c->h_pinned[1], miss_tries, miss_hashes32, miss_cap, n_missing);
  uint64_t bins[64], nb = 0;
  for (int d = 0; d < 64; ++d) nb += bins[d] = c->h_pinned[8 + d];
  if (nb) {
    hipLaunchKernelGGL(k_wit_starts, dim3(1), dim3(64), 0, st, (const unsigned long long*)(ctr + 8), cur);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(k_wit_scatter, GRID(vcap, BS), dim3(BS), 0, st, V, R, cur, blist, nv + 1);
    LAUNCH_CHECK();
    uint64_t lo = nb;
    for (int d = 63; d >= 0; --d) {
      if (!bins[d]) continue;
      lo -= bins[d];
      hipLaunchKernelGGL(k_wit_eval, GRID(bins[d], BS), dim3(BS), 0, st, M, R, V, (const uint32_t*)blist, lo, bins[d],
                         H.hits, np, hcap, ctr + 2, X);
      LAUNCH_CHECK();
    }
    HIPCHK(hipMemcpyAsync(c->h_pinned, ctr, 3 * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (c->h_pinned[1]) return wit_refuse(c, X, c->h_pinned[1], miss_tries, miss_hashes32, miss_cap, n_missing);
  }
  const uint64_t ncol = nb ? c->h_pinned[2] : 0;
  if (np + ncol > hcap) throw KhError{KH_EINTERNAL, "commit witness: more collapse children than branches"};
  uint64_t nn = 0;
  const uint64_t* list = hits_share(c, H, np + ncol, nn);
  HitSizes Z;
  const uint64_t total = hits_sizes(h, list, nn, Z);
  *n_nodes = nn;
  *rlp_len = total;
  if (nn > node_cap || total > rlp_cap)
    return set_err(KH_ENOSPC, "witness output too small (*n_nodes / *rlp_len hold the sizes needed)");
  if (nn && (!hashes32 || !off || (total && !rlp))) throw KhError{KH_EINVAL, "null output buffer"};
  hits_write(h, list, nn, total, Z, hashes32, rlp, off);
  HIPCHK(hipStreamSynchronize(st));
  if (n_collapse) *n_collapse = ncol;
  *n_missing = 0;
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

int kh_trie_commit_witness_host(kh_trie* h, const uint32_t* up_trie, const uint8_t* up_keys, uint64_t nup,
                                const uint32_t* del_trie, const uint8_t* del_keys, uint64_t ndel, uint32_t klen,
                                uint32_t flags, uint8_t* hashes32, uint64_t node_cap, uint8_t* rlp, uint64_t rlp_cap,
                                uint64_t* off, uint64_t* n_nodes, uint64_t* rlp_len, uint64_t* n_collapse,
                                uint32_t* miss_tries, uint8_t* miss_hashes32, uint64_t miss_cap, uint64_t* n_missing) {
  if (!h || !n_nodes || !rlp_len || !n_missing) return set_err(KH_EINVAL, "null handle or outputs");
  if (flags & ~KH_HASH_KEYS) return set_err(KH_EINVAL, "unknown witness flag");
  if ((flags & KH_HASH_KEYS) && !(h->flags & KH_HASH_KEYS))
    return set_err(KH_EINVAL, "KH_HASH_KEYS differs from the flag the trie was opened with");
  if ((nup && !up_keys) || (ndel && !del_keys) || (miss_cap && (!miss_tries || !miss_hashes32)))
    return set_err(KH_EINVAL, "null buffer");
  API_TRY({
    HANDLE_LOCK(h);
    HIPCHK(hipSetDevice(h->c->dev));
    return trie_commit_witness(h, up_trie, up_keys, nup, del_trie, del_keys, ndel, klen, hashes32, node_cap, rlp, rlp_cap,
                               off, n_nodes, rlp_len, n_collapse, miss_tries, miss_hashes32, miss_cap, n_missing);
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
