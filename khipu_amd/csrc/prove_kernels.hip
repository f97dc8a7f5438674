// Kernels of kh_trie_prove and kh_verify_proofs (prove.h holds the bodies), a cold compilation
// unit of their own like export_kernels.hip: the hot kernels of khst.hip keep their placement
// (tests/test_code_layout.py).  Kernels only; khst.hip declares and launches them.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "prove.h"

using namespace khst;

namespace {
constexpr int BS = 256;
}  // namespace

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
