// kh_trie_export_nodes and kh_trie_nodes_by_hash: their kernels (export.h holds the bodies), then
// the host driver and the C entry points (host.h).  A compilation unit of its own: a code object of
// its own cannot shift the placement of the hot kernels of khst.hip (tests/test_code_layout.py).
// The kernels take the POD views Recs and AMap and raw pointers; kh_trie_prove (prove_kernels.hip)
// launches them in list mode through host.h's prototypes.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "export.h"
#include "host.h"

using namespace khst;

namespace {
constexpr uint32_t GROUPS = BS / EXP_LANES;  // records per block

// sums over the 16 lanes of a record's group (a group never straddles a wave)
__device__ __forceinline__ uint32_t group_sum(uint32_t v) {
#pragma unroll
  for (int o = EXP_LANES / 2; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, EXP_LANES);
  return v;
}
__device__ __forceinline__ uint32_t group_prefix(uint32_t v, uint32_t lane) {  // exclusive
  uint32_t s = v;
#pragma unroll
  for (int o = 1; o < (int)EXP_LANES; o <<= 1) {
    const uint32_t u = (uint32_t)__shfl_up((int)s, o, EXP_LANES);
    if (lane >= (uint32_t)o) s += u;
  }
  return s - v;
}
// item i of a pass: record r0 + i with the node store's selection, or the by-hash hit list[i]
__device__ __forceinline__ uint32_t item_of(const Recs& R, const uint64_t* list, uint64_t r0, uint32_t filter,
                                            uint64_t i, uint64_t* r) {
  if (list) {
    const uint64_t h = list[i];
    *r = h >> 1;
    return h == EXP_NO_HIT ? 0u : ((h & 1) ? EXP_LOWER : EXP_UPPER);
  }
  *r = r0 + i;
  return exp_select(R, r0 + i, filter);
}
}  // namespace

// Sizes: 16 lanes per item, lane c probing child c of a branch whose body is written; the child
// records go to stash[16 i + c] for the write pass.  cnt (nullable) / bytes: per item.
__global__ void __launch_bounds__(BS) k_export_sizes(AMap M, Recs R, const uint8_t* heap, const uint64_t* list,
                                                     uint64_t r0, uint64_t n, uint32_t filter, uint32_t* stash,
                                                     uint32_t* cnt, uint32_t* bytes) {
  const uint64_t i = (uint64_t)blockIdx.x * GROUPS + threadIdx.x / EXP_LANES;
  const uint32_t lane = threadIdx.x % EXP_LANES;
  const bool in = i < n;  // (every lane stays for the shuffles)
  uint64_t r = 0;
  const uint32_t sel = in ? item_of(R, list, r0, filter, i, &r) : 0u;
  uint32_t il = 0;
  if (sel && exp_needs_children(R, r, sel)) {
    const uint32_t child = exp_child(R, M, r, lane);
    stash[i * EXP_LANES + lane] = child;
    il = exp_item_len(R, child);
  }
  const uint32_t S = group_sum(il);
  if (!in || lane) return;
  uint32_t c = 0, b = 0;
  if (sel) exp_sizes(R, heap, r, sel, S, &c, &b);
  if (cnt) cnt[i] = c;
  bytes[i] = b;
}

// The largest prefix of items that fits the caller's buffers, from the exclusive scans (monotone):
// fit[0] = k, fit[1] / fit[2] = nodes / bytes of items [0, k), fit[3] / fit[4] = of item k alone.
__global__ void __launch_bounds__(BS) k_export_fit(const uint32_t* cpos, const uint32_t* bpos, uint64_t n,
                                                   const uint32_t* totn, const uint32_t* totb, uint64_t node_cap,
                                                   uint64_t rlp_cap, unsigned long long* fit) {
  const uint64_t i = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (i > n) return;
  const uint64_t n0 = i < n ? cpos[i] : *totn, b0 = i < n ? bpos[i] : *totb;
  if (n0 > node_cap || b0 > rlp_cap) return;
  uint64_t n1 = 0, b1 = 0;
  if (i < n) {
    n1 = i + 1 < n ? cpos[i + 1] : *totn;
    b1 = i + 1 < n ? bpos[i + 1] : *totb;
    if (n1 <= node_cap && b1 <= rlp_cap) return;  // item i fits as well
  }
  fit[0] = i;
  fit[1] = n0;
  fit[2] = b0;
  fit[3] = n1 - n0;
  fit[4] = b1 - b0;
}

// Write: the encodings of items [0, n) at their scanned places, cooperatively over the 16 lanes.
// Export (hashes / off non-NULL): node slot cpos[i] (+1); by hash (found non-NULL): the encoding
// of query i at bpos[i].  A list with hashes / off (a proof's hits): item i is node slot i, at
// bpos64[i] when the 64-bit scan is given (the bytes of a call's proofs may pass 2^32).
__global__ void __launch_bounds__(BS) k_export_write(Recs R, const uint8_t* heap, const uint64_t* list, uint64_t r0,
                                                     uint64_t n, uint32_t filter, const uint32_t* stash,
                                                     const uint32_t* cpos, const uint32_t* bpos, uint8_t* hashes,
                                                     uint8_t* rlp, uint64_t* off, uint8_t* found,
                                                     const uint64_t* bpos64) {
  const uint64_t i = (uint64_t)blockIdx.x * GROUPS + threadIdx.x / EXP_LANES;
  const uint32_t lane = threadIdx.x % EXP_LANES;
  const bool in = i < n;
  uint64_t r = 0;
  const uint32_t sel = in ? item_of(R, list, r0, filter, i, &r) : 0u;
  uint32_t child = NONE, il = 0;
  if (sel && exp_needs_children(R, r, sel)) {
    child = stash[i * EXP_LANES + lane];
    il = exp_item_len(R, child);
  }
  const uint32_t S = group_sum(il), pre = group_prefix(il, lane);
  if (in && found && lane == 0) found[i] = sel != 0;
  if (!sel) return;
  uint32_t len[2];
  const uint64_t at = bpos64 ? bpos64[i] : bpos[i];
  exp_write(R, heap, r, sel, lane, child, pre, S, rlp + at, len);
  if (!hashes || lane >= 2) return;
  if (list) {  // one node an item
    if (lane) return;
    const ulonglong2* h = (const ulonglong2*)exp_hash_of(R, r, sel);
    ((ulonglong2*)(hashes + 32 * i))[0] = h[0];
    ((ulonglong2*)(hashes + 32 * i))[1] = h[1];
    off[i] = at;
    return;
  }
  // lane 0 / lane 1: the hash and offset of the first / second node written
  const uint32_t first = (sel & EXP_UPPER) ? EXP_UPPER : EXP_LOWER;
  if (lane == 1 && sel != (EXP_UPPER | EXP_LOWER)) return;
  const uint64_t slot = (uint64_t)cpos[i] + lane;
  const ulonglong2* h = (const ulonglong2*)exp_hash_of(R, r, lane ? EXP_LOWER : first);
  ((ulonglong2*)(hashes + 32 * slot))[0] = h[0];
  ((ulonglong2*)(hashes + 32 * slot))[1] = h[1];
  off[slot] = at + (lane ? len[0] : 0);
}

// KH_EXPORT_VERIFY: every written node re-hashed (one thread per node); mismatches counted.
__global__ void __launch_bounds__(BS) k_export_verify(const uint8_t* hashes, const uint8_t* rlp, const uint64_t* off,
                                                      uint64_t n, unsigned long long* bad) {
  const uint64_t j = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (j >= n) return;
  if (exp_verify(hashes, rlp, off, j)) atomicAdd(bad, 1ULL);
}

// By hash: nq (<= BYHASH_MAX_Q) query hashes as an open-addressing table in LDS, then a streaming
// scan of the records (grid-stride), each testing its two references.
constexpr uint32_t BYHASH_SLOTS = 4096;  // load <= 1/2
__global__ void __launch_bounds__(BS) k_by_hash_scan(Recs R, uint64_t rn, const uint64_t* Q, uint32_t nq,
                                                     uint64_t* hits) {
  __shared__ unsigned long long tags[BYHASH_SLOTS];
  __shared__ uint16_t qidx[BYHASH_SLOTS];
  uint32_t cap = 16;
  while (cap < 2 * nq) cap <<= 1;
  if (cap > BYHASH_SLOTS) return;  // (the host sends at most BYHASH_SLOTS / 2 queries per launch)
  const uint32_t mask = cap - 1;
  for (uint32_t s = threadIdx.x; s < cap; s += BS) tags[s] = 0;
  __syncthreads();
  for (uint32_t q = threadIdx.x; q < nq; q += BS) {  // (a repeated hash takes a slot per query)
    const unsigned long long tag = exp_tag(Q[4 * q]);
    for (uint32_t s = exp_tag_slot(tag, mask);; s = (s + 1) & mask)
      if (atomicCAS(&tags[s], 0ULL, tag) == 0ULL) {
        qidx[s] = (uint16_t)q;
        break;
      }
  }
  __syncthreads();
  for (uint64_t r = (uint64_t)blockIdx.x * BS + threadIdx.x; r < rn; r += (uint64_t)gridDim.x * BS)
    exp_scan_record(R, r, (const uint64_t*)tags, qidx, mask, Q, hits);
}

// ---------------------------------------------------------------------------
// host: node export and nodes by hash (export.h)
// ---------------------------------------------------------------------------
// records sized per pass: the child stash is 64 B a record (64 MiB), and two nodes of <= 532 B a
// record keep the 32-bit scans of a pass far from overflow
constexpr uint64_t EXPORT_WINDOW = 1ULL << 20;
constexpr uint64_t BYHASH_MAX = 4096, BYHASH_PASS = 2048;  // queries a call / an LDS table takes

static int trie_export(kh_trie* h, uint32_t filter, uint32_t flags, kh_export_cursor* cur, uint8_t* hashes32,
                       uint64_t node_cap, uint8_t* rlp, uint64_t rlp_cap, uint64_t* off, uint64_t* n_nodes,
                       uint64_t* rlp_len, int* done) {
  trie_settle(h);
  kh_ctx* c = h->c;
  hipStream_t st = c->st;
  const bool fresh = cur->next == 0 && cur->epoch == 0;  // a zeroed cursor starts here
  if ((!fresh && cur->epoch != h->epoch) || cur->next > h->rn)
    throw KhError{KH_EINVAL, "export cursor from before a commit, rollback or compaction of the handle"};
  uint64_t next = cur->next, wn = 0, wb = 0, need_n = 0, need_b = 0;
  bool short_out = false;
  while (next < h->rn && !short_out) {
    const uint64_t W = std::min(h->rn - next, EXPORT_WINDOW);
    Layout L;
    uint32_t *cnt, *byt, *stash, *tot;
    unsigned long long* fit;
    char* scr;
    L.add(cnt, W + 1);
    L.add(byt, W + 1);
    L.add(stash, W * EXP_LANES);
    L.add(scr, scan_scratch_size(W + 1, 4));
    L.add(tot, 4);
    L.add(fit, 8);  // [0..4] k_export_fit, [5] the verify counter
    place(h->gbuf, L);
    const Recs R = recs_of(h);
    const uint8_t* heap = (const uint8_t*)h->heap.p;
    HIPCHK(hipMemsetAsync(fit, 0, 64, st));
    hipLaunchKernelGGL(k_export_sizes, GRID(W * EXP_LANES, BS), dim3(BS), 0, st, map_of(h), R, heap,
                       (const uint64_t*)nullptr, next, W, filter, stash, cnt, byt);
    LAUNCH_CHECK();
    scan_u32(cnt, cnt, W, tot, scr, st);
    scan_u32(byt, byt, W, tot + 1, scr, st);
    hipLaunchKernelGGL(k_export_fit, GRID(W + 1, BS), dim3(BS), 0, st, (const uint32_t*)cnt, (const uint32_t*)byt, W,
                       (const uint32_t*)tot, (const uint32_t*)(tot + 1), node_cap - wn, rlp_cap - wb, fit);
    LAUNCH_CHECK();
    HIPCHK(hipMemcpyAsync(c->h_pinned, fit, 40, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const uint64_t k = c->h_pinned[0], tn = c->h_pinned[1], tb = c->h_pinned[2];
    if (k > W || wn + tn > node_cap || wb + tb > rlp_cap) throw KhError{KH_EINTERNAL, "export: bad prefix"};
    if (k < W) {  // record next + k does not fit what is left
      short_out = true;
      need_n = c->h_pinned[3];
      need_b = c->h_pinned[4];
    }
    if (tn) {
      h->xbuf.ensure(tn * 32 + tb + (tn + 1) * 8 + 1024);
      const EmitLayout E = emit_layout(h->xbuf, tn, tb);
      hipLaunchKernelGGL(k_export_write, GRID(k * EXP_LANES, BS), dim3(BS), 0, st, R, heap, (const uint64_t*)nullptr,
                         next, k, filter, (const uint32_t*)stash, (const uint32_t*)cnt, (const uint32_t*)byt, E.hashes,
                         E.rlp, E.off, (uint8_t*)nullptr, (const uint64_t*)nullptr);
      LAUNCH_CHECK();
      c->h_pinned[8] = tb;
      HIPCHK(hipMemcpyAsync(E.off + tn, c->h_pinned + 8, 8, hipMemcpyHostToDevice, st));
      if (flags & KH_EXPORT_VERIFY) {
        hipLaunchKernelGGL(k_export_verify, GRID(tn, BS), dim3(BS), 0, st, (const uint8_t*)E.hashes,
                           (const uint8_t*)E.rlp, (const uint64_t*)E.off, tn, fit + 5);
        LAUNCH_CHECK();
        HIPCHK(hipMemcpyAsync(c->h_pinned + 9, fit + 5, 8, hipMemcpyDeviceToHost, st));
      }
      HIPCHK(hipMemcpyAsync(hashes32 + 32 * wn, E.hashes, tn * 32, hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(rlp + wb, E.rlp, tb, hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(off + wn, E.off, tn * 8, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      if ((flags & KH_EXPORT_VERIFY) && c->h_pinned[9])
        throw KhError{KH_EINTERNAL, "export verify: a re-encoded node does not hash to its cached reference"};
      for (uint64_t j = 0; j < tn; ++j) off[wn + j] += wb;
    }
    wn += tn;
    wb += tb;
    next += k;
  }
  if (wn == 0 && short_out) {  // not even the next record's nodes fit: the cursor stays
    *n_nodes = need_n;
    *rlp_len = need_b;
    return set_err(KH_ENOSPC, "output too small for the next record (*n_nodes / *rlp_len hold what it needs)");
  }
  if (off) off[wn] = wb;
  *n_nodes = wn;
  *rlp_len = wb;
  cur->next = next;
  cur->epoch = h->epoch;
  *done = next >= h->rn;
  return KH_OK;
}

static int trie_by_hash(kh_trie* h, const uint8_t* hashes32, uint64_t n, uint8_t* found, uint8_t* rlp,
                        uint64_t rlp_cap, uint64_t* off, uint64_t* rlp_len) {
  trie_settle(h);
  kh_ctx* c = h->c;
  hipStream_t st = c->st;
  Layout L;
  uint64_t *Q, *hits;
  uint32_t *byt, *stash, *tot;
  uint8_t* fnd;
  char* scr;
  L.add(Q, n * 4);
  L.add(hits, n);
  L.add(byt, n + 1);
  L.add(stash, n * EXP_LANES);
  L.add(fnd, n);
  L.add(scr, scan_scratch_size(n + 1, 4));
  L.add(tot, 4);
  place(h->gbuf, L);
  const Recs R = recs_of(h);
  const uint8_t* heap = (const uint8_t*)h->heap.p;
  HIPCHK(hipMemcpyAsync(Q, hashes32, n * 32, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(hits, 0xFF, n * 8, st));
  if (h->rn && h->mcap) {
    const uint64_t blocks = std::min<uint64_t>((h->rn + BS - 1) / BS, 1024);  // (4 blocks a CU, grid-stride)
    for (uint64_t q0 = 0; q0 < n; q0 += BYHASH_PASS) {
      hipLaunchKernelGGL(k_by_hash_scan, dim3((unsigned)blocks), dim3(BS), 0, st, R, h->rn, (const uint64_t*)Q + 4 * q0,
                         (uint32_t)std::min(n - q0, BYHASH_PASS), hits + q0);
      LAUNCH_CHECK();
    }
  }
  hipLaunchKernelGGL(k_export_sizes, GRID(n * EXP_LANES, BS), dim3(BS), 0, st, map_of(h), R, heap, (const uint64_t*)hits,
                     (uint64_t)0, n, EXP_ALL_TRIES, stash, (uint32_t*)nullptr, byt);
  LAUNCH_CHECK();
  scan_u32(byt, byt, n, tot, scr, st);
  HIPCHK(hipMemcpyAsync(byt + n, tot, 4, hipMemcpyDeviceToDevice, st));
  HIPCHK(hipMemcpyAsync(c->h_pinned, tot, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  const uint64_t total = (uint32_t)c->h_pinned[0];
  *rlp_len = total;
  if (total > rlp_cap || (total && !rlp))
    return set_err(KH_ENOSPC, "encoding output too small (*rlp_len holds the size needed)");
  h->xbuf.ensure(total + 1024);
  hipLaunchKernelGGL(k_export_write, GRID(n * EXP_LANES, BS), dim3(BS), 0, st, R, heap, (const uint64_t*)hits,
                     (uint64_t)0, n, EXP_ALL_TRIES, (const uint32_t*)stash, (const uint32_t*)nullptr,
                     (const uint32_t*)byt, (uint8_t*)nullptr, (uint8_t*)h->xbuf.p, (uint64_t*)nullptr, fnd,
                     (const uint64_t*)nullptr);
  LAUNCH_CHECK();
  std::vector<uint32_t> o32(n + 1);
  HIPCHK(hipMemcpyAsync(o32.data(), byt, (n + 1) * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(found, fnd, n, hipMemcpyDeviceToHost, st));
  if (total) HIPCHK(hipMemcpyAsync(rlp, h->xbuf.p, total, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  for (uint64_t i = 0; i <= n; ++i) off[i] = o32[i];
  return KH_OK;
}

extern "C" {

int kh_trie_export_nodes(kh_trie* h, uint32_t trie_filter, uint32_t flags, kh_export_cursor* cur, uint8_t* hashes32,
                         uint64_t node_cap, uint8_t* rlp, uint64_t rlp_cap, uint64_t* off, uint64_t* n_nodes,
                         uint64_t* rlp_len, int* done) {
  if (!h || !cur || !n_nodes || !rlp_len || !done) return set_err(KH_EINVAL, "null handle, cursor or size outputs");
  if (flags & ~KH_EXPORT_VERIFY) return set_err(KH_EINVAL, "unknown export flag");
  if ((node_cap && (!hashes32 || !off)) || (rlp_cap && !rlp)) return set_err(KH_EINVAL, "null output buffer");
  if (!node_cap) rlp_cap = 0;  // (nothing can be written: sizes only)
  API_TRY({
    HANDLE_LOCK(h);
    HIPCHK(hipSetDevice(h->c->dev));
    *n_nodes = *rlp_len = 0;
    *done = 0;
    return trie_export(h, trie_filter, flags, cur, hashes32, node_cap, rlp, rlp_cap, off, n_nodes, rlp_len, done);
  })
}

int kh_trie_nodes_by_hash(kh_trie* h, const uint8_t* hashes32, uint64_t n, uint8_t* found, uint8_t* rlp,
                          uint64_t rlp_cap, uint64_t* off, uint64_t* rlp_len) {
  if (!h || !off || !rlp_len) return set_err(KH_EINVAL, "null handle or outputs");
  if (n > BYHASH_MAX) return set_err(KH_EINVAL, "at most 4096 hashes per call");
  if (n && (!hashes32 || !found)) return set_err(KH_EINVAL, "null buffer");
  API_TRY({
    HANDLE_LOCK(h);
    HIPCHK(hipSetDevice(h->c->dev));
    *rlp_len = 0;
    if (n == 0) {
      trie_settle(h);
      off[0] = 0;
      return KH_OK;
    }
    return trie_by_hash(h, hashes32, n, found, rlp, rlp_cap, off, rlp_len);
  })
}

}  // extern "C"
