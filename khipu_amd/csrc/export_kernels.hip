// Kernels of kh_trie_export_nodes and kh_trie_nodes_by_hash (export.h holds the bodies), in a
// compilation unit of their own: a code object of its own cannot shift the placement of the hot
// kernels of khst.hip (tests/test_code_layout.py).  Kernels only: they take the POD views Recs
// and AMap and raw pointers; khst.hip declares and launches them.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "export.h"

using namespace khst;

namespace {
constexpr int BS = 256;
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
