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
// partial (kh_forest_load_partial below its roots, kh_trie_fill_nodes): an absent hash makes a
// stub, counted in tot[6]; tot[7]: the store nodes decoded (items referenced by hash and found).
__global__ void __launch_bounds__(BS) k_load_count(LItems I, uint64_t ni, NStore S, LCounts C,
                                                   unsigned long long* tot, int partial) {
  const uint64_t i = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (i >= ni) return;
  uint32_t is_key = 0;
  const unsigned long long code = load_count_item(I, i, S, C, &is_key, partial != 0);
  if (code == OPEN_MISSING)
    atomicAdd(tot + 4, 1ULL);
  else if (code != OPEN_OK)
    atomicMax(tot + 3, code);
  if (is_key) atomicAdd(tot + 5, 1ULL);
  if (partial && code == OPEN_OK && I.rl[i] == 32) atomicAdd(C.src[i] == NONE ? tot + 6 : tot + 7, 1ULL);
}
// Fill pass: C holds the scanned counts.
__global__ void __launch_bounds__(BS) k_load_fill(LItems I, uint64_t ni, NStore S, LCounts C, LItems N,
                                                  const uint32_t* tries, uint8_t* recs, uint64_t rbase, uint64_t rcap,
                                                  uint8_t* heap, uint64_t hbase, uint64_t heap_cap, int partial) {
  const uint64_t i = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (i >= ni) return;
  load_fill_item(I, i, S, C, N, tries, recs, rbase, rcap, heap, hbase, heap_cap, partial != 0);
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
// cnt[1]: the root records, i.e. the tries met, cnt[2]: the stubs), then list them at the scanned
// places
__global__ void __launch_bounds__(BS) k_evict_flags(Recs R, uint64_t n, const uint32_t* tries, uint32_t nt,
                                                    uint32_t* flag, unsigned long long* cnt) {
  const uint64_t r = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (r >= n) return;
  const bool in = load_in_list(R, r, tries, nt);
  flag[r] = in ? 1u : 0u;
  if (in && load_holds_key(R, r)) atomicAdd(cnt, 1ULL);
  if (in && R.rd[r] == 0) atomicAdd(cnt + 1, 1ULL);
  if (in && load_is_stub(R, r)) atomicAdd(cnt + 2, 1ULL);  // (a stub goes with its trie)
}
__global__ void __launch_bounds__(BS) k_evict_list(uint64_t n, const uint32_t* flag, const uint32_t* pos, uint64_t cap,
                                                   uint32_t* list) {
  const uint64_t r = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (r >= n || !flag[r]) return;
  if (pos[r] < cap) list[pos[r]] = (uint32_t)r;
}

// ---- partial handles (forest.h EL_STUB).  All of these run only on a handle that holds stubs, or
// on the refusal path of a commit; one thread per record, op or element, no LDS, no loop over
// anything but a map probe or a binary search.

// kh_trie_fill_nodes, round 0: flag the live stubs whose missing node (rbref) is in the store ...
__global__ void __launch_bounds__(BS) k_fill_flags(Recs R, uint64_t n, NStore S, uint32_t* flag) {
  const uint64_t r = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (r >= n) return;
  bool hit = false;
  if (load_is_stub(R, r) && S.m) {
    uint64_t h[4];
    for (int q = 0; q < 4; ++q) h[q] = R.rbref[4 * r + q];
    const uint64_t p = key_lower_bound(S.hash, S.m, h);
    hit = p < S.m && key_cmp(S.hash + 4 * p, h) == 0;
  }
  flag[r] = hit ? 1u : 0u;
}
// ... and make each one a frontier item at its scanned place t (record order: a fixed order); the
// item is its own entry of the call's trie list (tries[t]), list[t] the stub to swap out at the end
__global__ void __launch_bounds__(BS) k_fill_items(Recs R, uint64_t n, const uint32_t* flag, const uint32_t* pos,
                                                   LItems N, uint32_t* tries, uint32_t* list) {
  const uint64_t r = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (r >= n || !flag[r]) return;
  const uint64_t t = pos[r];
  if (t >= N.cap) return;
  load_stub_item(R, r, N, t, (uint32_t)t);
  tries[t] = R.rt[r];
  list[t] = (uint32_t)r;
}

// A refused commit: the stubs among the n records its descent marked (each is listed once), as
// (trie id, hash to fetch = rbref) at claimed places; cnt counts them all, the first cap are written.
__global__ void __launch_bounds__(BS) k_stub_missing(Recs R, const uint32_t* list, uint64_t n, uint64_t cap,
                                                     uint32_t* out_trie, uint64_t* out_hash,
                                                     unsigned long long* cnt) {
  const uint64_t i = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (i >= n) return;
  const uint32_t r = list[i];
  if (!load_is_stub(R, r)) return;
  const unsigned long long t = atomicAdd(cnt, 1ULL);
  if (t >= cap) return;
  out_trie[t] = R.rt[r];
  for (int q = 0; q < 4; ++q) out_hash[4 * t + q] = R.rbref[4ull * r + q];
}
// After the element topology, before the commit writes anything: a stub element whose anchor
// would move (sorted element i hangs at pd[i] + 1, its record at oldd) is a node the reference's
// fix would load (MerklePatriciaTrie.scala:430-477); listed like the ones above.  A missing branch
// under a present extension (STUB_BRANCH) moves freely: fix re-cuts the extension without its branch.
__global__ void __launch_bounds__(BS) k_stub_moved(Recs R, const uint32_t* sidx, const int8_t* pd, const uint32_t* src,
                                                   const uint8_t* oldd, uint64_t m, uint64_t cap, uint32_t* out_trie,
                                                   uint64_t* out_hash, unsigned long long* cnt) {
  const uint64_t i = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (i >= m) return;
  const uint32_t s = sidx[i], r = src[s];
  if (r == NONE || !load_is_stub(R, r) || (R.rmask[r] & STUB_BRANCH)) return;
  if ((uint32_t)(pd[i] + 1) == (uint32_t)oldd[s]) return;
  const unsigned long long t = atomicAdd(cnt, 1ULL);
  if (t >= cap) return;
  out_trie[t] = R.rt[r];
  for (int q = 0; q < 4; ++q) out_hash[4 * t + q] = R.rbref[4ull * r + q];
}
// kh_trie_need_host: the stub key o's walk reaches (flag 1, its rbref), or flag 0
__global__ void __launch_bounds__(BS) k_need(AMap M, Recs R, const uint64_t* K, const uint32_t* trie, uint64_t n,
                                             uint8_t* flag, uint64_t* hash) {
  const uint64_t o = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (o >= n) return;
  const uint32_t r = forest_get(M, R, trie ? trie[o] : 0u, K + 4 * o);
  const bool stub = r != NONE && R.rdb[r] == EL_STUB;
  flag[o] = stub ? 1 : 0;
  for (int q = 0; q < 4; ++q) hash[4 * o + q] = stub ? R.rbref[4ull * r + q] : 0;
}
