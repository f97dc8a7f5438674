// Kernels of kh_trie_range_host / kh_dev_trie_range and of the batched kh_trie_ranges_host /
// kh_dev_trie_ranges (k_ranges_*: range.h holds the bodies of both), a cold compilation
// unit of their own like prove_kernels.hip and load_kernels.hip: the hot kernels of khst.hip keep
// their placement (tests/test_code_layout.py).  Kernels only; khst.hip declares and launches them.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "range.h"

using namespace khst;

namespace {
constexpr int BS = 256;
constexpr uint32_t GROUPS = BS / EXP_LANES;  // frontier items per block of the fill
}  // namespace

// Round 0: the root record of trie t, or NONE (an empty trie, or a trie id the forest does not
// hold), which the first count drops.
__global__ void k_range_root(AMap M, Recs R, uint32_t t, uint32_t* items) {
  if (blockIdx.x || threadIdx.x) return;
  const uint64_t zero[4] = {0, 0, 0, 0};
  items[0] = map_find(M, R, t, 0, zero);
}

// Count: one thread an item; what takes the item's place in the next frontier (no probe: a
// popcount of the child mask restricted by the range).  *expand is set when any item is a branch
// with children to place (every writer stores the same 1).
__global__ void __launch_bounds__(BS) k_range_count(Recs R, KeyRange g, const uint32_t* items, uint64_t n,
                                                    uint64_t* cnt, unsigned long long* expand) {
  const uint64_t i = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (i >= n) return;
  const uint32_t sel = rng_select(R, items[i], g);
  cnt[i] = rng_count(sel);
  if (sel & 0xFFFFu) *expand = 1;
}

// Fill: 16 lanes an item, lane c probing child c (the dependent tag-line then record-line reads
// of 16 children in flight at once); pos is the exclusive scan of the counts, and nothing is
// probed or written at or past the cut.  *bad: a child the mask names is not in the map.
__global__ void __launch_bounds__(BS) k_range_fill(AMap M, Recs R, KeyRange g, const uint32_t* items, uint64_t n,
                                                   const uint64_t* pos, uint64_t cut, uint32_t* out,
                                                   unsigned long long* bad) {
  const uint64_t i = (uint64_t)blockIdx.x * GROUPS + threadIdx.x / EXP_LANES;
  const uint32_t lane = threadIdx.x % EXP_LANES;
  if (i >= n) return;
  const uint64_t base = pos[i];
  if (base >= cut) return;
  const uint32_t r = items[i];
  if (!rng_fill_lane(R, M, r, rng_select(R, r, g), lane, base, cut, out)) *bad = 1;
}

// After the last round, over the first n1 <= max_entries + 1 items: the value lengths of the
// first nent of them, and the lowest stub (res[0] = (index << 32 | record), ~0 when there is none).
__global__ void __launch_bounds__(BS) k_range_lens(Recs R, const uint32_t* items, uint64_t n1, uint64_t nent,
                                                   uint64_t* len, unsigned long long* res) {
  const uint64_t i = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (i >= n1) return;
  const uint32_t r = items[i];
  const bool stub = rng_is_stub(R, r);
  if (stub) atomicMin(res, (unsigned long long)((i << 32) | r));
  if (i < nent) len[i] = (stub || r == NONE) ? 0 : R.rvl[r];
}
// fit[0] = k, the entries whose values fit val_cap, fit[1] = their bytes; fit[2] = the length of
// entry k alone, and next[4] its key (the first entry not returned), when n1 > k
__global__ void __launch_bounds__(BS) k_range_fit(Recs R, const uint32_t* items, uint64_t n1, const uint64_t* pos,
                                                  uint64_t nent, const uint64_t* total, uint64_t val_cap,
                                                  unsigned long long* fit, uint64_t* next) {
  const uint64_t i = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (i > nent) return;
  unsigned long long f[2] = {~0ULL, 0};
  rng_fit(pos, nent, *total, val_cap, i, f);
  if (f[0] != i) return;
  fit[0] = i;
  fit[1] = f[1];
  fit[2] = 0;
  if (i < n1 && items[i] != NONE) {
    const uint32_t r = items[i];
    fit[2] = R.rvl[r];
    for (int q = 0; q < 4; ++q) next[q] = R.rk[4ull * r + q];
  }
}
// the k returned entries: keys, offsets (voff[k] = the bytes in all), values
__global__ void __launch_bounds__(BS) k_range_write(Recs R, const uint8_t* heap, const uint32_t* items, uint64_t k,
                                                    const uint64_t* pos, uint64_t bytes, uint8_t* keys32,
                                                    uint64_t* voff, uint8_t* vals) {
  const uint64_t i = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (i > k) return;
  if (i == k) {
    voff[k] = bytes;
    return;
  }
  rng_write(R, heap, items[i], i, pos[i], keys32, voff, vals);
}

// ---- many ranges a call (range.h "MANY RANGES A CALL"): a frontier item is (record, request)
// Round 0: request q's KeyRange into G[q] and the root record of its trie at place q -- NONE for an
// empty trie, an id the forest does not hold, or origin > limit: the first count drops it.
__global__ void __launch_bounds__(BS) k_ranges_root(AMap M, Recs R, const uint32_t* tries, const uint8_t* origins32,
                                                    const uint8_t* limits32, uint64_t nq, KeyRange* G,
                                                    uint32_t* items, uint32_t* iq) {
  const uint64_t q = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (q >= nq) return;
  KeyRange g;
  const bool ok = rng_request(origins32, limits32, q, &g);
  G[q] = g;
  const uint64_t zero[4] = {0, 0, 0, 0};
  items[q] = ok ? map_find(M, R, tries ? tries[q] : 0u, 0, zero) : NONE;
  iq[q] = (uint32_t)q;
}
// k_range_count with every item selected against its own request's range
__global__ void __launch_bounds__(BS) k_ranges_count(Recs R, const KeyRange* G, const uint32_t* items,
                                                     const uint32_t* iq, uint64_t n, uint64_t* cnt,
                                                     unsigned long long* expand) {
  const uint64_t i = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (i >= n) return;
  const uint32_t sel = rng_select(R, items[i], G[iq[i]]);
  cnt[i] = rng_count(sel);
  if (sel & 0xFFFFu) *expand = 1;
}
// k_range_fill, the item's request written beside each child placed
__global__ void __launch_bounds__(BS) k_ranges_fill(AMap M, Recs R, const KeyRange* G, const uint32_t* items,
                                                    const uint32_t* iq, uint64_t n, const uint64_t* pos, uint64_t cut,
                                                    uint32_t* out, uint32_t* outq, unsigned long long* bad) {
  const uint64_t i = (uint64_t)blockIdx.x * GROUPS + threadIdx.x / EXP_LANES;
  const uint32_t lane = threadIdx.x % EXP_LANES;
  if (i >= n) return;
  const uint64_t base = pos[i];
  if (base >= cut) return;
  const uint32_t r = items[i], q = iq[i];
  if (!rng_fill_lane(R, M, r, rng_select(R, r, G[q]), lane, base, cut, out, outq, q)) *bad = 1;
}
// k_range_fit, and fit[3] = the request of thing k, the first not returned (nq when there is none)
__global__ void __launch_bounds__(BS) k_ranges_fit(Recs R, const uint32_t* items, const uint32_t* iq, uint64_t n1,
                                                   const uint64_t* pos, uint64_t nent, const uint64_t* total,
                                                   uint64_t val_cap, uint64_t nq, unsigned long long* fit,
                                                   uint64_t* next) {
  const uint64_t i = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (i > nent) return;
  unsigned long long f[2] = {~0ULL, 0};
  rng_fit(pos, nent, *total, val_cap, i, f);
  if (f[0] != i) return;
  fit[0] = i;
  fit[1] = f[1];
  fit[2] = 0;
  fit[3] = i < n1 ? iq[i] : nq;
  if (i < n1 && items[i] != NONE) {
    const uint32_t r = items[i];
    fit[2] = R.rvl[r];
    for (int q = 0; q < 4; ++q) next[q] = R.rk[4ull * r + q];
  }
}
// the k returned entries (k_range_write) and the nq + 1 request offsets: ent_off[q] = the first
// returned item of request q or later (ent_off[nq] = k)
__global__ void __launch_bounds__(BS) k_ranges_write(Recs R, const uint8_t* heap, const uint32_t* items,
                                                     const uint32_t* iq, uint64_t k, const uint64_t* pos,
                                                     uint64_t bytes, uint64_t nq, uint8_t* keys32, uint64_t* voff,
                                                     uint8_t* vals, uint64_t* ent_off) {
  const uint64_t i = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (i <= nq) ent_off[i] = rng_ent_off(iq, k, i);
  if (i > k) return;
  if (i == k) {
    voff[k] = bytes;
    return;
  }
  rng_write(R, heap, items[i], i, pos[i], keys32, voff, vals);
}
