// Kernels of kh_forest_load_nodes, kh_forest_roots and kh_forest_evict (load.h holds the bodies),
// in a compilation unit of their own: a code object of its own cannot shift the placement of the
// hot kernels of khst.hip (tests/test_code_layout.py).  Kernels only: they take the POD views and
// raw pointers; khst.hip declares and launches them.  One thread per frontier node or record.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "load.h"

using namespace khst;

namespace {
constexpr int BS = 256;
}

// Round 0: the k listed tries' roots (hash references at anchor 0); a root equal to the empty
// trie's loads nothing.  flag[j] = 1 for a root to walk; pos: its exclusive scan.
__global__ void __launch_bounds__(BS) k_load_root_flags(const uint64_t* roots, uint64_t k, uint32_t* flag) {
  const uint64_t j = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (j >= k) return;
  const uint64_t E[4] = {0xa655cc1b171fe856ULL, 0x6ef8c092e64583ffULL, 0xc0ad6c991be0485bULL, 0x21b463e3b52f6201ULL};
  bool empty = true;
  for (int q = 0; q < 4; ++q) empty = empty && roots[4 * j + q] == E[q];
  flag[j] = empty ? 0u : 1u;
}
__global__ void __launch_bounds__(BS) k_load_roots(const uint64_t* roots, uint64_t k, const uint32_t* flag,
                                                   const uint32_t* pos, LItems N) {
  const uint64_t j = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (j >= k || !flag[j]) return;
  const uint64_t t = pos[j];
  if (t >= N.cap) return;
  for (int q = 0; q < 4; ++q) {
    N.pre[4 * t + q] = 0;
    N.ref[4 * t + q] = roots[4 * j + q];
    N.pref[4 * t + q] = roots[4 * j + q];
  }
  N.a[t] = 0;
  N.d[t] = 0;
  N.rl[t] = 32;
  N.prl[t] = 32;
  N.j[t] = (uint32_t)j;
}
// ids that already have a live record at anchor (t, 0)
__global__ void __launch_bounds__(BS) k_load_resident(AMap M, Recs R, const uint32_t* tries, uint64_t k,
                                                      unsigned long long* n_resident) {
  const uint64_t j = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (j >= k) return;
  const uint64_t zero[4] = {0, 0, 0, 0};
  const uint32_t r = map_find(M, R, tries[j], 0, zero);
  if (r != NONE && R.rlive[r] == REC_LIVE) atomicAdd(n_resident, 1ULL);
}

// Count pass of one round.  tot: [3] the largest error code met (OPEN_BAD / OPEN_VALUE; a missing
// node is counted, not an error code), [4] missing references, [5] keys (leaves and value-only
// branches) -- sums and a maximum, which do not depend on the order the threads run in.
__global__ void __launch_bounds__(BS) k_load_count(LItems I, uint64_t ni, NStore S, LCounts C,
                                                   unsigned long long* tot) {
  const uint64_t i = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (i >= ni) return;
  uint32_t is_key = 0;
  const unsigned long long code = load_count_item(I, i, S, C, &is_key);
  if (code == OPEN_MISSING)
    atomicAdd(tot + 4, 1ULL);
  else if (code != OPEN_OK)
    atomicMax(tot + 3, code);
  if (is_key) atomicAdd(tot + 5, 1ULL);
}
// Fill pass: C holds the scanned counts.
__global__ void __launch_bounds__(BS) k_load_fill(LItems I, uint64_t ni, NStore S, LCounts C, LItems N,
                                                  const uint32_t* tries, uint8_t* recs, uint64_t rbase, uint64_t rcap,
                                                  uint8_t* heap, uint64_t hbase, uint64_t heap_cap) {
  const uint64_t i = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (i >= ni) return;
  load_fill_item(I, i, S, C, N, tries, recs, rbase, rcap, heap, hbase, heap_cap);
}
// The missing references of a round, one entry per reference, at the scan of the miss flags
// (the first cap of them): the list index of the trie and the hash.
__global__ void __launch_bounds__(BS) k_load_missing(LItems I, uint64_t ni, const uint32_t* miss, const uint32_t* mpos,
                                                     uint64_t cap, uint32_t* out_idx, uint64_t* out_hash) {
  const uint64_t i = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (i >= ni || !miss[i]) return;
  const uint64_t t = mpos[i];
  if (t >= cap) return;
  out_idx[t] = I.j[i];
  for (int q = 0; q < 4; ++q) out_hash[4 * t + q] = I.ref[4 * i + q];
}

// kh_forest_roots: flag the root records, then write (trie id, root hash) at the scanned places
__global__ void __launch_bounds__(BS) k_roots_flags(Recs R, uint64_t n, uint32_t* flag) {
  const uint64_t r = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (r >= n) return;
  flag[r] = load_is_root(R, r) ? 1u : 0u;
}
__global__ void __launch_bounds__(BS) k_roots_write(Recs R, uint64_t n, const uint32_t* flag, const uint32_t* pos,
                                                    uint64_t cap, uint32_t* tries, uint64_t* roots) {
  const uint64_t r = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (r >= n || !flag[r]) return;
  const uint64_t t = pos[r];
  if (t >= cap) return;
  tries[t] = R.rt[r];
  for (int q = 0; q < 4; ++q) roots[4 * t + q] = R.rref[4 * r + q];
}

// kh_forest_evict: flag the live records of the nt sorted trie ids (cnt[0]: those holding a key,
// cnt[1]: the root records, i.e. the tries met), then list them at the scanned places
__global__ void __launch_bounds__(BS) k_evict_flags(Recs R, uint64_t n, const uint32_t* tries, uint32_t nt,
                                                    uint32_t* flag, unsigned long long* cnt) {
  const uint64_t r = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (r >= n) return;
  const bool in = load_in_list(R, r, tries, nt);
  flag[r] = in ? 1u : 0u;
  if (in && load_holds_key(R, r)) atomicAdd(cnt, 1ULL);
  if (in && R.rd[r] == 0) atomicAdd(cnt + 1, 1ULL);
}
__global__ void __launch_bounds__(BS) k_evict_list(uint64_t n, const uint32_t* flag, const uint32_t* pos, uint64_t cap,
                                                   uint32_t* list) {
  const uint64_t r = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (r >= n || !flag[r]) return;
  if (pos[r] < cap) list[pos[r]] = (uint32_t)r;
}
