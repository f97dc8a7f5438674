// kh_trie_range_host / kh_dev_trie_range and the batched kh_trie_ranges_host / kh_dev_trie_ranges:
// their kernels (k_ranges_*: range.h holds the bodies of both); kh_trie_diff_host / kh_dev_trie_diff,
// the same ordered frontier run over two tries in lockstep (diff.h: k_diff_*), and the batched
// kh_trie_diffs_host / kh_dev_trie_diffs (k_diffs_*); kh_trie_changes_since_host /
// kh_dev_trie_changes_since (changes.h: k_chg_*, changes_scan), which finds its differences in the
// journal and pages them with the diff's tail.  Every call launches kernels of its own; the
// host code that sequences them is one driver: run_rounds (the round loop), fit_page (the tail) and
// page_to_host / page_in_place (the two forms of an entry point), the 16 words they share named by
// TotWord.  range_scan, ranges_scan, diff_scan and diffs_scan hold what differs: the workspace,
// round 0 and the launches.  Then the C entry points (host.h).
// A cold compilation unit of its own like prove_kernels.hip and load_kernels.hip: the hot kernels
// of khst.hip keep their placement (tests/test_code_layout.py).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "changes.h"
#include "host.h"

using namespace khst;

namespace {
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

// ---- trie diff (diff.h): a frontier item is (record of a, record of b, depth)
// Round 0: the two root records (NONE: an empty side, or a trie id the forest does not hold); n[0] =
// 0 when there is nothing to walk: both sides empty, or the root pair skipped (equal tries).
__global__ void k_diff_root(DSide A, uint32_t ta, uint32_t has_a, DSide B, uint32_t tb, uint32_t has_b,
                            uint32_t* ia, uint32_t* ib, uint32_t* id, unsigned long long* n) {
  if (blockIdx.x || threadIdx.x) return;
  const uint64_t zero[4] = {0, 0, 0, 0};
  const uint32_t ra = has_a ? map_find(A.M, A.R, ta, 0, zero) : NONE;
  const uint32_t rb = has_b ? map_find(B.M, B.R, tb, 0, zero) : NONE;
  ia[0] = ra;
  ib[0] = rb;
  id[0] = 0;
  n[0] = ((ra == NONE && rb == NONE) || df_skip(A, ra, B, rb, 0)) ? 0 : 1;
}
// Select and count: 16 lanes an item, lane c forming the child pair at nibble c and testing it for
// the skip (the probes of both sides' 16 children in flight at once); the surviving lanes are the
// item's selection (sel) and their number its count.  *expand: an item expanded or split.
__global__ void __launch_bounds__(BS) k_diff_select(DSide A, DSide B, KeyRange g, const uint32_t* ia,
                                                    const uint32_t* ib, uint64_t n, uint32_t* sel, uint64_t* cnt,
                                                    unsigned long long* expand) {
  const uint64_t i = (uint64_t)blockIdx.x * GROUPS + threadIdx.x / EXP_LANES;
  const uint32_t lane = threadIdx.x % EXP_LANES, gbase = (threadIdx.x & 63u) & ~(EXP_LANES - 1u);
  const bool valid = i < n;
  uint32_t plan = 0;
  bool alive = false;
  if (valid) {
    const uint32_t ra = ia[i], rb = ib[i];
    plan = df_plan(A, ra, B, rb, g);
    alive = df_lane_alive(A, ra, B, rb, plan, lane);
  }
  const uint32_t kids = (uint32_t)(__ballot(alive) >> gbase) & 0xFFFFu;
  if (!valid || lane) return;
  const uint32_t s = (plan & ~0xFFFFu) | kids;
  sel[i] = s;
  cnt[i] = df_count(s);
  if (df_expands(s)) *expand = 1;
}
// Fill: 16 lanes an item; pos is the exclusive scan of the counts, and nothing is probed or written
// at or past the cut.  *bad: a child a mask names is not in its side's map.
__global__ void __launch_bounds__(BS) k_diff_fill(DSide A, DSide B, const uint32_t* ia, const uint32_t* ib,
                                                  const uint32_t* id, const uint32_t* sel, uint64_t n,
                                                  const uint64_t* pos, uint64_t cut, uint32_t* oa, uint32_t* ob,
                                                  uint32_t* od, unsigned long long* bad) {
  const uint64_t i = (uint64_t)blockIdx.x * GROUPS + threadIdx.x / EXP_LANES;
  const uint32_t lane = threadIdx.x % EXP_LANES;
  if (i >= n) return;
  const uint64_t base = pos[i];
  if (base >= cut) return;
  if (!df_fill_lane(A, ia[i], B, ib[i], id[i], sel[i], lane, base, cut, oa, ob, od)) *bad = 1;
}
// After the last round, over the first n1 <= max_entries + 1 items: the lengths of side b's values
// of the first nent of them, and the lowest item with a stub (res[0] = index << 33 | (1: the stub is
// b's) << 32 | record, ~0 when there is none)
__global__ void __launch_bounds__(BS) k_diff_lens(DSide A, DSide B, const uint32_t* ia, const uint32_t* ib,
                                                  uint64_t n1, uint64_t nent, uint64_t* len,
                                                  unsigned long long* res) {
  const uint64_t i = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (i >= n1) return;
  const uint32_t ra = ia[i], rb = ib[i];
  if (df_missing(A, ra, B, rb)) {
    const bool of_a = ra != NONE && df_stub(A.R, ra);
    atomicMin(res, (unsigned long long)((i << 33) | (of_a ? 0ULL : 1ULL << 32) | (of_a ? ra : rb)));
  }
  if (i < nent) len[i] = df_len(A, ra, B, rb);
}
// k_range_fit over the differences: fit[2] = the bytes of difference k alone, next[4] its key
__global__ void __launch_bounds__(BS) k_diff_fit(DSide A, DSide B, const uint32_t* ia, const uint32_t* ib,
                                                 uint64_t n1, const uint64_t* pos, uint64_t nent,
                                                 const uint64_t* total, uint64_t val_cap, unsigned long long* fit,
                                                 uint64_t* next) {
  const uint64_t i = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (i > nent) return;
  unsigned long long f[2] = {~0ULL, 0};
  rng_fit(pos, nent, *total, val_cap, i, f);
  if (f[0] != i) return;
  fit[0] = i;
  fit[1] = f[1];
  fit[2] = 0;
  if (i < n1 && (ia[i] != NONE || ib[i] != NONE)) {  // (both NONE: a corrupt map, flagged by the fill)
    const uint32_t ra = ia[i], rb = ib[i];
    fit[2] = df_len(A, ra, B, rb);
    const uint64_t* k = df_key(A, ra, B, rb);
    for (int q = 0; q < 4; ++q) next[q] = k[q];
  }
}
// the k returned differences: keys, kinds, offsets (voff[k] = the bytes in all), side b's values
__global__ void __launch_bounds__(BS) k_diff_write(DSide A, DSide B, const uint32_t* ia, const uint32_t* ib,
                                                   uint64_t k, const uint64_t* pos, uint64_t bytes, uint8_t* keys32,
                                                   uint8_t* kinds, uint64_t* voff, uint8_t* vals) {
  const uint64_t i = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (i > k) return;
  if (i == k) {
    voff[k] = bytes;
    return;
  }
  df_write(A, ia[i], B, ib[i], i, pos[i], keys32, kinds, voff, vals);
}

// ---- many pairs a call (diff.h "MANY PAIRS A CALL"): a frontier item is (record of a, record of b,
// depth, request)
// Round 0: one thread a request (df_request); *live counts the requests with something to walk
__global__ void __launch_bounds__(BS) k_diffs_root(DSide A, const uint32_t* ta, uint32_t has_a, DSide B,
                                                   const uint32_t* tb, uint32_t has_b, uint32_t same,
                                                   const uint8_t* origins32, const uint8_t* limits32, uint64_t nq,
                                                   KeyRange* G, uint32_t* ia, uint32_t* ib, uint32_t* id, uint32_t* iq,
                                                   unsigned long long* live) {
  const uint64_t q = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (q >= nq) return;
  if (df_request(A, ta, has_a != 0, B, tb, has_b != 0, same != 0, origins32, limits32, q, G, ia, ib, id, iq))
    atomicAdd(live, 1ULL);
}
// k_diff_select with every item selected against its own request's range
__global__ void __launch_bounds__(BS) k_diffs_select(DSide A, DSide B, const KeyRange* G, const uint32_t* ia,
                                                     const uint32_t* ib, const uint32_t* iq, uint64_t n,
                                                     uint32_t* sel, uint64_t* cnt, unsigned long long* expand) {
  const uint64_t i = (uint64_t)blockIdx.x * GROUPS + threadIdx.x / EXP_LANES;
  const uint32_t lane = threadIdx.x % EXP_LANES, gbase = (threadIdx.x & 63u) & ~(EXP_LANES - 1u);
  const bool valid = i < n;
  uint32_t plan = 0;
  bool alive = false;
  if (valid) {
    const uint32_t ra = ia[i], rb = ib[i];
    plan = df_plan(A, ra, B, rb, G[iq[i]]);
    alive = df_lane_alive(A, ra, B, rb, plan, lane);
  }
  const uint32_t kids = (uint32_t)(__ballot(alive) >> gbase) & 0xFFFFu;
  if (!valid || lane) return;
  const uint32_t s = (plan & ~0xFFFFu) | kids;
  sel[i] = s;
  cnt[i] = df_count(s);
  if (df_expands(s)) *expand = 1;
}
// k_diff_fill, the item's request written beside each item placed
__global__ void __launch_bounds__(BS) k_diffs_fill(DSide A, DSide B, const uint32_t* ia, const uint32_t* ib,
                                                   const uint32_t* id, const uint32_t* iq, const uint32_t* sel,
                                                   uint64_t n, const uint64_t* pos, uint64_t cut, uint32_t* oa,
                                                   uint32_t* ob, uint32_t* od, uint32_t* oq, unsigned long long* bad) {
  const uint64_t i = (uint64_t)blockIdx.x * GROUPS + threadIdx.x / EXP_LANES;
  const uint32_t lane = threadIdx.x % EXP_LANES;
  if (i >= n) return;
  const uint64_t base = pos[i];
  if (base >= cut) return;
  if (!df_fill_lane(A, ia[i], B, ib[i], id[i], sel[i], lane, base, cut, oa, ob, od, oq, iq[i])) *bad = 1;
}
// k_diff_fit, and fit[3] = the request of thing k, the first not returned (nq when there is none)
__global__ void __launch_bounds__(BS) k_diffs_fit(DSide A, DSide B, const uint32_t* ia, const uint32_t* ib,
                                                  const uint32_t* iq, uint64_t n1, const uint64_t* pos, uint64_t nent,
                                                  const uint64_t* total, uint64_t val_cap, uint64_t nq,
                                                  unsigned long long* fit, uint64_t* next) {
  const uint64_t i = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (i > nent) return;
  unsigned long long f[2] = {~0ULL, 0};
  rng_fit(pos, nent, *total, val_cap, i, f);
  if (f[0] != i) return;
  fit[0] = i;
  fit[1] = f[1];
  fit[2] = 0;
  fit[3] = i < n1 ? iq[i] : nq;
  if (i < n1 && (ia[i] != NONE || ib[i] != NONE)) {  // (both NONE: a corrupt map, flagged by the fill)
    const uint32_t ra = ia[i], rb = ib[i];
    fit[2] = df_len(A, ra, B, rb);
    const uint64_t* k = df_key(A, ra, B, rb);
    for (int w = 0; w < 4; ++w) next[w] = k[w];
  }
}
// the k returned differences (k_diff_write) and the nq + 1 request offsets: ent_off[q] = the first
// returned item of request q or later (ent_off[nq] = k)
__global__ void __launch_bounds__(BS) k_diffs_write(DSide A, DSide B, const uint32_t* ia, const uint32_t* ib,
                                                    const uint32_t* iq, uint64_t k, const uint64_t* pos,
                                                    uint64_t bytes, uint64_t nq, uint8_t* keys32, uint8_t* kinds,
                                                    uint64_t* voff, uint8_t* vals, uint64_t* ent_off) {
  const uint64_t i = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (i <= nq) ent_off[i] = rng_ent_off(iq, k, i);
  if (i > k) return;
  if (i == k) {
    voff[k] = bytes;
    return;
  }
  df_write(A, ia[i], B, ib[i], i, pos[i], keys32, kinds, voff, vals);
}

// ---- changes since a savepoint (changes.h): candidates from the journal and the appended records,
// sorted by (trie, key), joined a run a thread; the page is the trie diff's (k_diff_lens / _fit / _write)
// Collect: one thread a journal position (its saved copy and the current record at its index) or an
// appended record.  What decides -- live, db -- lies in ONE 16-byte word of a record (bytes 32..47),
// so a thread loads that word and touches one line a record, as a record read whole would a lane;
// the keys are read later, of the kept candidates only.
__global__ void __launch_bounds__(BS) k_chg_collect(ChgSrc S, uint32_t* keep) {
  const uint64_t g = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (g >= S.jn + S.an) return;
  if (g < S.jn) {
    const uint64_t p = S.j0 + g;
    const uint32_t idx = S.jidx[p];
    const ulonglong2 cw = *(const ulonglong2*)(S.J.rk.b + p * REC_BYTES + 32);
    const bool old = chg_keep_old(idx, S.rn0, chg_entry_words(cw.x, cw.y));
    bool cur = false;
    if (old) {
      const ulonglong2 rw = *(const ulonglong2*)(S.R.rk.b + (uint64_t)idx * REC_BYTES + 32);
      cur = chg_keep_new(idx, S.rn0, true, chg_entry_words(rw.x, rw.y));
    }
    keep[g] = old ? 1u : 0u;
    keep[S.jn + g] = cur ? 1u : 0u;
  } else {
    const uint64_t a = g - S.jn;
    const ulonglong2 rw = *(const ulonglong2*)(S.R.rk.b + (S.rn0 + a) * REC_BYTES + 32);
    keep[2 * S.jn + a] = chg_entry_words(rw.x, rw.y) ? 1u : 0u;
  }
}
// the kept slots, in slot order (pos: the exclusive scan of keep)
__global__ void __launch_bounds__(BS) k_chg_compact(const uint32_t* keep, const uint32_t* pos, uint64_t n,
                                                    uint32_t* sv) {
  const uint64_t i = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (i < n && keep[i]) sv[pos[i]] = (uint32_t)i;
}
// word w of every slot's sort key, in the slots' present order (one stable radix sort a word)
__global__ void __launch_bounds__(BS) k_chg_sortkey(ChgSrc S, const uint32_t* sv, uint64_t n, uint32_t w,
                                                    uint64_t* ck) {
  const uint64_t j = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (j < n) ck[j] = chg_sort_word(S, sv[j], w);
}
// Join: one thread a sorted place; the head of a run of equal (trie, key) classifies the run, and a
// difference at or after the resume point (from.o; has_from) is flagged with its item.  *tie: the
// order cannot be trusted (chg_head).
__global__ void __launch_bounds__(BS) k_chg_join(ChgSrc S, const uint32_t* sv, uint64_t n, uint32_t reverse,
                                                 uint32_t has_from, uint32_t from_trie, KeyRange from, uint32_t* ja,
                                                 uint32_t* jb, uint32_t* flag, unsigned long long* tie) {
  const uint64_t j = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (j >= n) return;
  bool t = false;
  uint32_t po, rn, f = 0;
  if (chg_head(S, sv, j, &t) && chg_join(S, sv, n, j, &po, &rn) &&
      (!has_from || chg_from(S, sv[j], from_trie, from.o))) {
    chg_item(po, rn, reverse != 0, &ja[j], &jb[j]);
    f = 1;
  }
  if (t) *tie = 1;
  flag[j] = f;
}
// the first `cut` differences as items (dpos: the exclusive scan of flag)
__global__ void __launch_bounds__(BS) k_chg_list(const uint32_t* flag, const uint32_t* dpos, uint64_t n, uint64_t cut,
                                                 const uint32_t* ja, const uint32_t* jb, uint32_t* ia, uint32_t* ib) {
  const uint64_t j = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (j >= n || !flag[j] || dpos[j] >= cut) return;
  ia[dpos[j]] = ja[j];
  ib[dpos[j]] = jb[j];
}
// the trie ids of the n1 items looked at
__global__ void __launch_bounds__(BS) k_chg_tries(DSide A, DSide B, const uint32_t* ia, const uint32_t* ib,
                                                  uint64_t n1, uint32_t* out) {
  const uint64_t i = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (i < n1) out[i] = chg_item_trie(A, ia[i], B, ib[i]);
}

// ---------------------------------------------------------------------------
// host: the frontier driver the four services share (range.h, diff.h)
// ---------------------------------------------------------------------------
// The 16 device words every call keeps at `tot`; a round reads the first three back into
// c->h_pinned, the tail all sixteen, at the same indices.
enum TotWord : uint32_t {
  T_NEXT = 0,    // the items of the next frontier (the total of the counts, before the cut)
  T_EXPAND = 1,  // an item of this round has children to place (range), expanded or split (diff)
  T_BAD = 2,     // a child a mask names is not in its side's map
  T_STUB = 3,    // the lowest stub among the things looked at (k_*_lens), ~0: none
  T_K = 4,       // k_*_fit: the things whose values fit val_cap,
  T_BYTES = 5,   //   their bytes,
  T_ALONE = 6,   //   the bytes of thing k alone, the first not returned,
  T_REQ = 7,     //   its request (the batched calls),
  T_KEY = 8,     //   and [8..12) its key
  T_VALS = 12,   // the value bytes of all the things asked for (the total of the lengths)
  T_ROOT = 15,   // round 0 of a diff: something to walk (k_diff_root), the live requests (k_diffs_root)
  T_WORDS = 16,
};
// c->h_pinned past them, when a stub refuses the call: its node's hash, then its request
enum PinWord : uint32_t { PIN_MISSING = 16, PIN_REQUEST = 20 };

// a service's texts and its round cap (a sound trie of 64 nibbles ends well below it)
struct Service {
  const char* name;
  uint32_t round_cap;
  const char *enode, *enospc;
};
static const char ENOSPC_ENTRY[] = "value output too small for the first entry (*val_bytes holds its size)";
static const char ENOSPC_DIFF[] = "value output too small for the first difference (*val_bytes holds its size)";
static const Service RANGE = {
    "range scan", 66, "the range meets a subtree the handle does not hold (missing32 names its node)", ENOSPC_ENTRY};
static const Service RANGES = {"range scan", 66,
                               "a range meets a subtree the handle does not hold (missing32 names its node, "
                               "*n_done the request)",
                               ENOSPC_ENTRY};
static const Service DIFF = {
    "trie diff", 68, "the diff meets a subtree a handle does not hold (missing32 names its node)", ENOSPC_DIFF};
static const Service DIFFS = {"trie diff", 68,
                              "a diff meets a subtree a handle does not hold (missing32 names its node, *n_done "
                              "the request)",
                              ENOSPC_DIFF};

// the scratch every service carves out of its handle's gbuf beside its own frontier columns
struct Work {
  uint64_t* cnt = nullptr;            // a round's counts, then their scan; the tail's value offsets
  char* scr = nullptr;                // the scratch of their scan
  unsigned long long* tot = nullptr;  // TotWord
  uint64_t F = 0;                     // the cut: no frontier grows past F items
};
// What the rounds and the tail leave for the write: the final frontier's columns (ia alone on a
// range: its records; iq on the batched calls), the scanned value offsets, what fits.
struct Page {
  const uint32_t *ia = nullptr, *ib = nullptr, *iq = nullptr;
  const uint64_t* pos = nullptr;
  const DSide *A = nullptr, *B = nullptr;  // a diff over other record arrays than the handles' (changes_scan)
  uint64_t nq = 0;            // the requests of a batched call (0: a single call)
  uint64_t k = 0, bytes = 0;  // the things returned and their value bytes (k = 0: an empty answer)
  uint64_t n1 = 0;            // the things looked at: k < n1 when the answer is cut
  uint64_t req = 0;           // the cut request, or the refusing stub's; nq when every request is answered
};
struct PageOut {  // the caller's outputs every call has
  uint64_t *n_entries, *val_bytes;
  uint8_t *next32, *missing32;
};
struct Walk {
  uint64_t ni = 0, visited = 0;  // the final frontier's items; the items selected in all rounds
  uint32_t rounds = 0;
  int cur = 0;  // the side of the two frontiers that holds the final one
};

static KeyRange key_range(const uint8_t* origin32, const uint8_t* limit32) {
  KeyRange g;
  memset(g.o, 0, 32);
  memset(g.l, 0xFF, 32);
  if (origin32) memcpy(g.o, origin32, 32);
  if (limit32) memcpy(g.l, limit32, 32);
  return g;
}

// The rounds past round 0, from a frontier of ni items on side 0: select(cur, ni) launches the
// count of the ni items on side cur, fill(cur, ni) places their children on side cur ^ 1.  One sync
// of a pinned word triple a round; the round that expands nothing closes the walk.
template <class Select, class Fill>
static Walk run_rounds(kh_ctx* c, const Service& sv, const Work& w, uint64_t ni, Select select, Fill fill) {
  hipStream_t st = c->st;
  Walk r;
  for (r.ni = ni; r.ni; ++r.rounds) {
    if (r.rounds > sv.round_cap) throw KhError{KH_EINTERNAL, std::string(sv.name) + ": the rounds do not end"};
    r.visited += r.ni;
    HIPCHK(hipMemsetAsync(w.tot, 0, 16, st));  // T_NEXT, T_EXPAND
    select(r.cur, r.ni);
    LAUNCH_CHECK();
    scan_u64(w.cnt, w.cnt, r.ni, (uint64_t*)(w.tot + T_NEXT), w.scr, st);
    HIPCHK(hipMemcpyAsync(c->h_pinned, w.tot, 24, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const uint64_t total = c->h_pinned[T_NEXT], expand = c->h_pinned[T_EXPAND];
    if (c->h_pinned[T_BAD]) throw KhError{KH_EINTERNAL, std::string(sv.name) + ": corrupt anchor map"};
    const uint64_t nn = std::min(total, w.F);  // the cut
    if (nn) {
      fill(r.cur, r.ni);
      LAUNCH_CHECK();
    }
    r.cur ^= 1;
    r.ni = nn;
    if (!expand) {
      ++r.rounds;
      break;
    }
  }
  return r;
}

// After the rounds: the fit of the first me things of the final frontier (P.ia / ib / iq, P.pos
// set by the caller) to val_cap.  lens(n1, nent) launches k_*_lens, fit(n1, nent) k_*_fit.  b is the
// second handle of a diff (its stub word carries a side bit below the index), NULL on a range.
// KH_OK with P.k, P.bytes, P.n1, P.req and *n_entries, *val_bytes, next32 set; KH_ENOSPC with
// *val_bytes; KH_ENODE with missing32 and P.req.
template <class Lens, class Fit>
static int fit_page(kh_ctx* c, const Service& sv, const Work& w, uint64_t ni, uint64_t me, kh_trie* a, kh_trie* b,
                    Page& P, const PageOut& o, Lens lens, Fit fit) {
  hipStream_t st = c->st;
  P.k = P.bytes = 0;
  P.req = P.nq;
  const uint64_t n1 = P.n1 = std::min(ni, me + 1), nent = std::min(ni, me);
  if (n1 == 0) {
    *o.n_entries = *o.val_bytes = 0;
    return KH_OK;
  }
  HIPCHK(hipMemsetAsync(w.tot + T_STUB, 0xFF, 8, st));
  lens(n1, nent);
  LAUNCH_CHECK();
  scan_u64(w.cnt, w.cnt, nent, (uint64_t*)(w.tot + T_VALS), w.scr, st);
  fit(n1, nent);
  LAUNCH_CHECK();
  HIPCHK(hipMemcpyAsync(c->h_pinned, w.tot, T_WORDS * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (c->h_pinned[T_BAD]) throw KhError{KH_EINTERNAL, std::string(sv.name) + ": corrupt anchor map"};
  const uint64_t stub = c->h_pinned[T_STUB];
  if (stub != ~0ULL) {  // a missing subtree among the first max_entries + 1 things of the answer
    const uint64_t r = (uint32_t)stub, at = stub >> (b ? 33 : 32);
    kh_trie* of = (b && ((stub >> 32) & 1)) ? b : a;
    HIPCHK(hipMemcpyAsync(c->h_pinned + PIN_MISSING, (const uint8_t*)of->recs.p + r * REC_BYTES + 96, 32,
                          hipMemcpyDeviceToHost, st));
    if (P.iq) HIPCHK(hipMemcpyAsync(c->h_pinned + PIN_REQUEST, P.iq + at, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (o.missing32) memcpy(o.missing32, c->h_pinned + PIN_MISSING, 32);
    if (P.iq) P.req = (uint32_t)c->h_pinned[PIN_REQUEST];
    return set_err(KH_ENODE, sv.enode);
  }
  const uint64_t k = c->h_pinned[T_K];
  if (k == 0) {
    *o.val_bytes = c->h_pinned[T_ALONE];
    return set_err(KH_ENOSPC, sv.enospc);
  }
  P.k = k;
  P.bytes = c->h_pinned[T_BYTES];
  *o.n_entries = k;
  *o.val_bytes = P.bytes;
  if (k < n1) {
    memcpy(o.next32, c->h_pinned + T_KEY, 32);
    if (P.iq) P.req = c->h_pinned[T_REQ];
  }
  return KH_OK;
}

static DSide side_of(kh_trie* h) {
  return DSide{recs_of(h), h->mcap ? map_of(h) : AMap{{nullptr}, {nullptr}, 0}, (const uint8_t*)h->heap.p};
}

// the page's keys, kinds (a diff), offsets, values and request offsets (a batched call) into device
// buffers (P.k > 0): the one write kernel of the service, b NULL on a range
static void page_write(kh_trie* a, kh_trie* b, const Page& P, uint8_t* d_keys32, uint8_t* d_kinds, uint8_t* d_vals,
                       uint64_t* d_voff, uint64_t* d_ent_off) {
  hipStream_t st = a->c->st;
  const dim3 grid = GRID(std::max(P.k, P.nq) + 1, BS);
  if (!b && !P.iq)
    hipLaunchKernelGGL(k_range_write, grid, dim3(BS), 0, st, recs_of(a), (const uint8_t*)a->heap.p, P.ia, P.k, P.pos,
                       P.bytes, d_keys32, d_voff, d_vals);
  else if (!b)
    hipLaunchKernelGGL(k_ranges_write, grid, dim3(BS), 0, st, recs_of(a), (const uint8_t*)a->heap.p, P.ia, P.iq, P.k,
                       P.pos, P.bytes, P.nq, d_keys32, d_voff, d_vals, d_ent_off);
  else if (!P.iq)
    hipLaunchKernelGGL(k_diff_write, grid, dim3(BS), 0, st, P.A ? *P.A : side_of(a), P.B ? *P.B : side_of(b), P.ia,
                       P.ib, P.k, P.pos, P.bytes, d_keys32, d_kinds, d_voff, d_vals);
  else
    hipLaunchKernelGGL(k_diffs_write, grid, dim3(BS), 0, st, side_of(a), side_of(b), P.ia, P.ib, P.iq, P.k, P.pos,
                       P.bytes, P.nq, d_keys32, d_kinds, d_voff, d_vals, d_ent_off);
  LAUNCH_CHECK();
}
// The host form of a call, after its scan: the page written into a staging of its exact sizes and
// copied to the caller's arrays (kinds on a diff, ent_off on a batched call, else NULL).
static void page_to_host(kh_trie* a, kh_trie* b, const Page& P, uint8_t* keys32, uint8_t* kinds, uint8_t* vals,
                         uint64_t* voff, uint64_t* ent_off) {
  kh_ctx* c = a->c;
  hipStream_t st = c->st;
  if (P.k == 0) {
    voff[0] = 0;
    if (ent_off) memset(ent_off, 0, (P.nq + 1) * 8);
    return;
  }
  if (P.bytes && !vals) throw KhError{KH_EINVAL, "null value buffer"};
  Layout Lo;
  uint8_t *dk, *dkind = nullptr, *dv;
  uint64_t *dvo, *deo = nullptr;
  Lo.add(dk, P.k * 32 + 64);
  Lo.add(dvo, P.k + 1);
  if (ent_off) Lo.add(deo, P.nq + 1);
  if (kinds) Lo.add(dkind, P.k + 64);
  Lo.add(dv, P.bytes + 64);
  place(c->out_emit, Lo);
  page_write(a, b, P, dk, dkind, dv, dvo, deo);
  HIPCHK(hipMemcpyAsync(keys32, dk, P.k * 32, hipMemcpyDeviceToHost, st));
  if (kinds) HIPCHK(hipMemcpyAsync(kinds, dkind, P.k, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(voff, dvo, (P.k + 1) * 8, hipMemcpyDeviceToHost, st));
  if (ent_off) HIPCHK(hipMemcpyAsync(ent_off, deo, (P.nq + 1) * 8, hipMemcpyDeviceToHost, st));
  if (P.bytes) HIPCHK(hipMemcpyAsync(vals, dv, P.bytes, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
}
// the device form: the page written in place, or the offsets of an empty answer
static void page_in_place(kh_trie* a, kh_trie* b, const Page& P, uint8_t* d_keys32, uint8_t* d_kinds, uint8_t* d_vals,
                          uint64_t* d_voff, uint64_t* d_ent_off) {
  hipStream_t st = a->c->st;
  if (P.k == 0) {
    HIPCHK(hipMemsetAsync(d_voff, 0, 8, st));
    if (d_ent_off) HIPCHK(hipMemsetAsync(d_ent_off, 0, (P.nq + 1) * 8, st));
  } else {
    if (P.bytes && !d_vals) throw KhError{KH_EINVAL, "null value buffer"};
    page_write(a, b, P, d_keys32, d_kinds, d_vals, d_voff, d_ent_off);
  }
  HIPCHK(hipStreamSynchronize(st));
}
// the request arrays of a batched host form into the context's in_keys: a trie id column per side
// that needs one (pair: a diff, with a column for b), the origins and limits that are given
struct Requests {
  uint32_t *ta = nullptr, *tb = nullptr;
  uint8_t *o = nullptr, *l = nullptr;
};
static void stage_requests(kh_ctx* c, Requests& d, uint64_t nq, const uint32_t* tries_a, bool want_a, bool pair,
                           const uint32_t* tries_b, bool want_b, const uint8_t* origins32, const uint8_t* limits32) {
  hipStream_t st = c->st;
  Layout Li;
  Li.add(d.ta, nq, want_a);
  if (pair) Li.add(d.tb, nq, want_b);
  Li.add(d.o, nq * 32, origins32 != nullptr);
  Li.add(d.l, nq * 32, limits32 != nullptr);
  place(c->in_keys, Li);
  if (d.ta) HIPCHK(hipMemcpyAsync(d.ta, tries_a, nq * 4, hipMemcpyHostToDevice, st));
  if (d.tb) HIPCHK(hipMemcpyAsync(d.tb, tries_b, nq * 4, hipMemcpyHostToDevice, st));
  if (d.o) HIPCHK(hipMemcpyAsync(d.o, origins32, nq * 32, hipMemcpyHostToDevice, st));
  if (d.l) HIPCHK(hipMemcpyAsync(d.l, limits32, nq * 32, hipMemcpyHostToDevice, st));
}

static bool refuse(const char* msg) {
  set_err(KH_EINVAL, msg);
  return false;
}
// the argument checks every call shares (ptrs: the handles and outputs it needs are there), then
// what a pair of handles and a batch over a forest add
static bool page_args_ok(bool ptrs, bool batched, uint64_t nq, uint64_t max_entries) {
  if (!ptrs) return refuse("null handle or outputs");
  if (!batched) return (max_entries != 0 && max_entries < (1ULL << 31)) || refuse("max_entries must be in [1, 2^31)");
  return (nq != 0 && max_entries != 0 && nq < (1ULL << 31) && max_entries < (1ULL << 31) &&
          nq + max_entries < (1ULL << 31)) ||
         refuse("nq and max_entries must be at least 1 and nq + max_entries < 2^31");
}
static bool pair_ok(kh_trie* a, kh_trie* b) {
  return a->c->dev == b->c->dev || refuse("the two handles live on different devices");
}
static bool ranges_ids_ok(kh_trie* h, const uint32_t* tries) {
  return !(h->forest && !tries) || refuse("a forest needs a trie id per request");
}
static bool diffs_ids_ok(kh_trie* a, const uint32_t* tries_a, kh_trie* b, const uint32_t* tries_b) {
  return !((a->forest && !tries_a) || (b->forest && !tries_b && !tries_a)) ||
         refuse("a forest side needs a trie id per request");
}

// ---------------------------------------------------------------------------
// host: range scan (range.h)
// ---------------------------------------------------------------------------
static uint32_t g_range_rounds = 0;  // rounds of the last scan (khst_range_rounds: measurements only)
extern "C" uint32_t khst_range_rounds() { return g_range_rounds; }

// A range scan (range.h) and the fit to val_cap: two frontiers of max_entries + 2 items.  KH_OK with
// the page described in P (P.k = 0: an empty answer) and *n_entries, *val_bytes, *more, next32 set;
// KH_ENOSPC with *val_bytes; KH_ENODE with missing32.
static int range_scan(kh_trie* h, uint32_t trie, const uint8_t* origin32, const uint8_t* limit32, uint64_t max_entries,
                      uint64_t val_cap, Page& P, const PageOut& o, int* more) {
  trie_settle(h);
  kh_ctx* c = h->c;
  hipStream_t st = c->st;
  const KeyRange g = key_range(origin32, limit32);
  const uint32_t t = h->forest ? trie : 0u;
  // (no more entries than records: the frontiers of a call asking for 2^31 - 1 stay the trie's size)
  const uint64_t me = std::min<uint64_t>(max_entries, std::max<uint64_t>(h->rn, 1));
  Layout L;
  uint32_t* f[2];
  Work w;
  const uint64_t F = w.F = me + 2;
  L.add(f[0], F + 1);
  L.add(f[1], F + 1);
  L.add(w.cnt, F + 1);
  L.add(w.scr, scan_scratch_size(F + 1, 8));
  L.add(w.tot, T_WORDS);
  place(h->gbuf, L);
  const Recs R = recs_of(h);
  Walk r;
  if (h->rn && h->mcap && key_cmp(g.o, g.l) <= 0) {
    const AMap M = map_of(h);
    HIPCHK(hipMemsetAsync(w.tot, 0, T_WORDS * 8, st));
    // (an empty trie, or an id the forest does not hold: the item is NONE and the first count drops it)
    hipLaunchKernelGGL(k_range_root, dim3(1), dim3(1), 0, st, M, R, t, f[0]);
    LAUNCH_CHECK();
    r = run_rounds(
        c, RANGE, w, 1,
        [&](int cur, uint64_t ni) {
          hipLaunchKernelGGL(k_range_count, GRID(ni, BS), dim3(BS), 0, st, R, g, f[cur], ni, w.cnt,
                             w.tot + T_EXPAND);
        },
        [&](int cur, uint64_t ni) {
          hipLaunchKernelGGL(k_range_fill, GRID(ni * EXP_LANES, BS), dim3(BS), 0, st, M, R, g, f[cur], ni, w.cnt, F,
                             f[cur ^ 1], w.tot + T_BAD);
        });
  }
  g_range_rounds = r.rounds;
  P.ia = f[r.cur];
  P.pos = w.cnt;
  const int rc = fit_page(
      c, RANGE, w, r.ni, me, h, nullptr, P, o,
      [&](uint64_t n1, uint64_t nent) {
        hipLaunchKernelGGL(k_range_lens, GRID(n1, BS), dim3(BS), 0, st, R, P.ia, n1, nent, w.cnt, w.tot + T_STUB);
      },
      [&](uint64_t n1, uint64_t nent) {
        hipLaunchKernelGGL(k_range_fit, GRID(nent + 1, BS), dim3(BS), 0, st, R, P.ia, n1, w.cnt, nent,
                           (const uint64_t*)(w.tot + T_VALS), val_cap, w.tot + T_K, (uint64_t*)(w.tot + T_KEY));
      });
  if (rc == KH_OK) *more = P.k < P.n1;
  return rc;
}

// ---- many ranges a call (range.h "MANY RANGES A CALL")
// nq range scans moving together and the fit to val_cap: the requests (device arrays; d_tries NULL
// on a single trie, d_origins / d_limits nullable) through two segmented frontiers of max_entries +
// 2 * nq items (range.h derives the cut).  KH_OK with the answer described in P (P.k = 0: nothing in
// any range) and *n_entries, *val_bytes, *n_done, next32 set; KH_ENOSPC with *val_bytes; KH_ENODE
// with missing32 and *n_done.
static int ranges_scan(kh_trie* h, const uint32_t* d_tries, const uint8_t* d_origins, const uint8_t* d_limits,
                       uint64_t nq, uint64_t max_entries, uint64_t val_cap, Page& P, const PageOut& o,
                       uint64_t* n_done) {
  trie_settle(h);
  kh_ctx* c = h->c;
  hipStream_t st = c->st;
  // (a request returns no more entries than the handle has records: the frontiers of a call asking
  // for 2^31 - 1 follow the handle and nq)
  const uint64_t me = std::min<uint64_t>(max_entries, nq * std::max<uint64_t>(h->rn, 1));
  Layout L;
  uint32_t *f[2], *fq[2];
  Work w;
  KeyRange* G;
  const uint64_t F = w.F = me + 2 * nq;
  L.add(f[0], F + 1);
  L.add(f[1], F + 1);
  L.add(fq[0], F + 1);
  L.add(fq[1], F + 1);
  L.add(w.cnt, F + 1);
  L.add(G, nq);
  L.add(w.scr, scan_scratch_size(F + 1, 8));
  L.add(w.tot, T_WORDS);
  place(h->gbuf, L);
  const Recs R = recs_of(h);
  Walk r;
  if (h->rn && h->mcap) {
    const AMap M = map_of(h);
    HIPCHK(hipMemsetAsync(w.tot, 0, T_WORDS * 8, st));
    hipLaunchKernelGGL(k_ranges_root, GRID(nq, BS), dim3(BS), 0, st, M, R, d_tries, d_origins, d_limits, nq, G, f[0],
                       fq[0]);
    LAUNCH_CHECK();
    r = run_rounds(
        c, RANGES, w, nq,
        [&](int cur, uint64_t ni) {
          hipLaunchKernelGGL(k_ranges_count, GRID(ni, BS), dim3(BS), 0, st, R, G, f[cur], fq[cur], ni, w.cnt,
                             w.tot + T_EXPAND);
        },
        [&](int cur, uint64_t ni) {
          hipLaunchKernelGGL(k_ranges_fill, GRID(ni * EXP_LANES, BS), dim3(BS), 0, st, M, R, G, f[cur], fq[cur], ni,
                             w.cnt, F, f[cur ^ 1], fq[cur ^ 1], w.tot + T_BAD);
        });
  }
  g_range_rounds = r.rounds;
  P.ia = f[r.cur];
  P.iq = fq[r.cur];
  P.nq = nq;
  P.pos = w.cnt;
  const int rc = fit_page(
      c, RANGES, w, r.ni, me, h, nullptr, P, o,
      [&](uint64_t n1, uint64_t nent) {
        hipLaunchKernelGGL(k_range_lens, GRID(n1, BS), dim3(BS), 0, st, R, P.ia, n1, nent, w.cnt, w.tot + T_STUB);
      },
      [&](uint64_t n1, uint64_t nent) {
        hipLaunchKernelGGL(k_ranges_fit, GRID(nent + 1, BS), dim3(BS), 0, st, R, P.ia, P.iq, n1, w.cnt, nent,
                           (const uint64_t*)(w.tot + T_VALS), val_cap, nq, w.tot + T_K, (uint64_t*)(w.tot + T_KEY));
      });
  if (rc != KH_ENOSPC) *n_done = P.req;
  return rc;
}

// ---------------------------------------------------------------------------
// host: trie diff (diff.h)
// ---------------------------------------------------------------------------
static uint32_t g_diff_rounds = 0;   // rounds of the last diff past the root pair, and the frontier
static uint64_t g_diff_visited = 0;  // items it selected in them (khst_diff_*: measurements only)
extern "C" uint32_t khst_diff_rounds() { return g_diff_rounds; }
extern "C" uint64_t khst_diff_visited() { return g_diff_visited; }

// A diff (diff.h) and the fit to val_cap, on a's stream with the scratch in a's gbuf (both handles
// locked and settled by the caller, b's stream drained): two frontiers of max_entries + 2 items.
// KH_OK with the page described in P (P.k = 0: no difference) and *n_entries, *val_bytes, *more,
// next32 set; KH_ENOSPC with *val_bytes; KH_ENODE with missing32.
static int diff_scan(kh_trie* a, uint32_t trie_a, kh_trie* b, uint32_t trie_b, const uint8_t* origin32,
                     const uint8_t* limit32, uint64_t max_entries, uint64_t val_cap, Page& P, const PageOut& o,
                     int* more) {
  kh_ctx* c = a->c;
  hipStream_t st = c->st;
  const KeyRange g = key_range(origin32, limit32);
  const uint32_t ta = a->forest ? trie_a : 0u, tb = b->forest ? trie_b : 0u;
  const bool has_a = a->rn && a->mcap, has_b = b->rn && b->mcap;
  // (no more differences than records: the frontiers of a call asking for 2^31 - 1 stay the tries' size)
  const uint64_t me = std::min<uint64_t>(max_entries, std::max<uint64_t>(a->rn + b->rn, 1));
  Layout L;
  uint32_t *fa[2], *fb[2], *fd[2], *sel;
  Work w;
  const uint64_t F = w.F = me + 2;
  for (int s = 0; s < 2; ++s) {
    L.add(fa[s], F + 1);
    L.add(fb[s], F + 1);
    L.add(fd[s], F + 1);
  }
  L.add(sel, F + 1);
  L.add(w.cnt, F + 1);
  L.add(w.scr, scan_scratch_size(F + 1, 8));
  L.add(w.tot, T_WORDS);
  place(a->gbuf, L);
  const DSide A = side_of(a), B = side_of(b);
  Walk r;
  if ((has_a || has_b) && !(a == b && ta == tb) && key_cmp(g.o, g.l) <= 0) {
    HIPCHK(hipMemsetAsync(w.tot, 0, T_WORDS * 8, st));
    hipLaunchKernelGGL(k_diff_root, dim3(1), dim3(1), 0, st, A, ta, (uint32_t)has_a, B, tb, (uint32_t)has_b, fa[0],
                       fb[0], fd[0], w.tot + T_ROOT);
    LAUNCH_CHECK();
    HIPCHK(hipMemcpyAsync(c->h_pinned, w.tot + T_ROOT, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    r = run_rounds(
        c, DIFF, w, c->h_pinned[0],
        [&](int cur, uint64_t ni) {
          hipLaunchKernelGGL(k_diff_select, GRID(ni * EXP_LANES, BS), dim3(BS), 0, st, A, B, g, fa[cur], fb[cur], ni,
                             sel, w.cnt, w.tot + T_EXPAND);
        },
        [&](int cur, uint64_t ni) {
          hipLaunchKernelGGL(k_diff_fill, GRID(ni * EXP_LANES, BS), dim3(BS), 0, st, A, B, fa[cur], fb[cur], fd[cur],
                             sel, ni, w.cnt, F, fa[cur ^ 1], fb[cur ^ 1], fd[cur ^ 1], w.tot + T_BAD);
        });
  }
  g_diff_rounds = r.rounds;
  g_diff_visited = r.visited;
  P.ia = fa[r.cur];
  P.ib = fb[r.cur];
  P.pos = w.cnt;
  const int rc = fit_page(
      c, DIFF, w, r.ni, me, a, b, P, o,
      [&](uint64_t n1, uint64_t nent) {
        hipLaunchKernelGGL(k_diff_lens, GRID(n1, BS), dim3(BS), 0, st, A, B, P.ia, P.ib, n1, nent, w.cnt,
                           w.tot + T_STUB);
      },
      [&](uint64_t n1, uint64_t nent) {
        hipLaunchKernelGGL(k_diff_fit, GRID(nent + 1, BS), dim3(BS), 0, st, A, B, P.ia, P.ib, n1, w.cnt, nent,
                           (const uint64_t*)(w.tot + T_VALS), val_cap, w.tot + T_K, (uint64_t*)(w.tot + T_KEY));
      });
  if (rc == KH_OK) *more = P.k < P.n1;
  return rc;
}
// both handles locked, settled and on a's device; b's work drained when it runs on another stream
#define DIFF_ENTER(a, b)                                      \
  PairLock pair_lock_((a)->lk, (b)->lk);                      \
  HIPCHK(hipSetDevice((a)->c->dev));                          \
  trie_settle(a);                                             \
  if ((b) != (a)) trie_settle(b);                             \
  if ((b)->c != (a)->c) HIPCHK(hipStreamSynchronize((b)->c->st))

// ---- many pairs a call (diff.h "MANY PAIRS A CALL")
static uint32_t g_diffs_rounds = 0;   // rounds of the last batched diff past the root pairs, and the
static uint64_t g_diffs_visited = 0;  // frontier items it selected in them (khst_diffs_*: measurements only)
extern "C" uint32_t khst_diffs_rounds() { return g_diffs_rounds; }
extern "C" uint64_t khst_diffs_visited() { return g_diffs_visited; }

// nq diffs moving together and the fit to val_cap, on a's stream with the scratch in a's gbuf (both
// handles locked and settled by the caller, b's stream drained): the requests (device arrays; d_ta /
// d_tb NULL on a single trie, d_origins / d_limits nullable) through two segmented frontiers of
// max_entries + 2 * nq items (diff.h derives the cut).  KH_OK with the answer described in P (P.k =
// 0: no difference in any request) and *n_entries, *val_bytes, *n_done, next32 set; KH_ENOSPC with
// *val_bytes; KH_ENODE with missing32 and *n_done.
static int diffs_scan(kh_trie* a, const uint32_t* d_ta, kh_trie* b, const uint32_t* d_tb, const uint8_t* d_origins,
                      const uint8_t* d_limits, uint64_t nq, uint64_t max_entries, uint64_t val_cap, Page& P,
                      const PageOut& o, uint64_t* n_done) {
  kh_ctx* c = a->c;
  hipStream_t st = c->st;
  const bool has_a = a->rn && a->mcap, has_b = b->rn && b->mcap;
  // (a request returns no more differences than the two handles have records: the frontiers of a
  // call asking for 2^31 - 1 follow the handles and nq)
  const uint64_t me = std::min<uint64_t>(max_entries, nq * std::max<uint64_t>(a->rn + b->rn, 1));
  Layout L;
  uint32_t *fa[2], *fb[2], *fd[2], *fq[2], *sel;
  Work w;
  KeyRange* G;
  const uint64_t F = w.F = me + 2 * nq;
  for (int s = 0; s < 2; ++s) {
    L.add(fa[s], F + 1);
    L.add(fb[s], F + 1);
    L.add(fd[s], F + 1);
    L.add(fq[s], F + 1);
  }
  L.add(sel, F + 1);
  L.add(w.cnt, F + 1);
  L.add(G, nq);
  L.add(w.scr, scan_scratch_size(F + 1, 8));
  L.add(w.tot, T_WORDS);
  place(a->gbuf, L);
  const DSide A = side_of(a), B = side_of(b);
  Walk r;
  if (has_a || has_b) {
    HIPCHK(hipMemsetAsync(w.tot, 0, T_WORDS * 8, st));
    hipLaunchKernelGGL(k_diffs_root, GRID(nq, BS), dim3(BS), 0, st, A, d_ta, (uint32_t)has_a, B, d_tb, (uint32_t)has_b,
                       (uint32_t)(a == b), d_origins, d_limits, nq, G, fa[0], fb[0], fd[0], fq[0], w.tot + T_ROOT);
    LAUNCH_CHECK();
    HIPCHK(hipMemcpyAsync(c->h_pinned, w.tot + T_ROOT, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const uint64_t live = c->h_pinned[0];  // (none: every request is empty or its roots are equal -- no round)
    r = run_rounds(
        c, DIFFS, w, live ? nq : 0,
        [&](int cur, uint64_t ni) {
          hipLaunchKernelGGL(k_diffs_select, GRID(ni * EXP_LANES, BS), dim3(BS), 0, st, A, B, G, fa[cur], fb[cur],
                             fq[cur], ni, sel, w.cnt, w.tot + T_EXPAND);
        },
        [&](int cur, uint64_t ni) {
          hipLaunchKernelGGL(k_diffs_fill, GRID(ni * EXP_LANES, BS), dim3(BS), 0, st, A, B, fa[cur], fb[cur], fd[cur],
                             fq[cur], sel, ni, w.cnt, F, fa[cur ^ 1], fb[cur ^ 1], fd[cur ^ 1], fq[cur ^ 1],
                             w.tot + T_BAD);
        });
    if (live) r.visited -= nq - live;  // (the first frontier holds every request; only the live ones are visited)
  }
  g_diffs_rounds = r.rounds;
  g_diffs_visited = r.visited;
  P.ia = fa[r.cur];
  P.ib = fb[r.cur];
  P.iq = fq[r.cur];
  P.nq = nq;
  P.pos = w.cnt;
  const int rc = fit_page(
      c, DIFFS, w, r.ni, me, a, b, P, o,
      [&](uint64_t n1, uint64_t nent) {
        hipLaunchKernelGGL(k_diff_lens, GRID(n1, BS), dim3(BS), 0, st, A, B, P.ia, P.ib, n1, nent, w.cnt,
                           w.tot + T_STUB);
      },
      [&](uint64_t n1, uint64_t nent) {
        hipLaunchKernelGGL(k_diffs_fit, GRID(nent + 1, BS), dim3(BS), 0, st, A, B, P.ia, P.ib, P.iq, n1, w.cnt, nent,
                           (const uint64_t*)(w.tot + T_VALS), val_cap, nq, w.tot + T_K, (uint64_t*)(w.tot + T_KEY));
      });
  if (rc != KH_ENOSPC) *n_done = P.req;
  return rc;
}

// ---------------------------------------------------------------------------
// host: changes since a savepoint (changes.h)
// ---------------------------------------------------------------------------
static const Service CHANGES = {"changes since a savepoint", 0, "", ENOSPC_DIFF};
// c->h_pinned past TotWord and PinWord: the call's own three words (ChgWord), the next pair's trie
enum ChgPin : uint32_t { PIN_CHG = 24, PIN_NEXT_TRIE = 28 };
enum ChgWord : uint32_t { CW_KEPT = 0, CW_TOTAL = 1, CW_TIE = 2, CW_WORDS = 4 };
// the page of a call: the diff's page over the two record arrays, and the items' trie ids
struct ChgPage {
  Page P;
  DSide A, B;
  const uint32_t* d_tr = nullptr;
  uint32_t next_trie = 0;
};
static uint32_t g_chg_sorts = 0;  // radix sorts of the last call (khst_changes_sorts: measurements and tests only)
extern "C" uint32_t khst_changes_sorts() { return g_chg_sorts; }

// The changes (changes.h) and the fit to val_cap, in the handle's gbuf on its stream: nothing but
// that scratch is written.  KH_OK with the page in Q (Q.P.k = 0: no difference) and *n_entries,
// *val_bytes, *n_total, *more, next32, Q.next_trie set; KH_ENOSPC with *val_bytes and *n_total.
static int changes_scan(kh_trie* h, uint32_t level, bool reverse, uint32_t from_trie, const uint8_t* from32,
                        uint64_t max_entries, uint64_t val_cap, ChgPage& Q, const PageOut& o, uint64_t* n_total,
                        int* more) {
  trie_settle(h);
  if (h->sps.empty()) throw KhError{KH_EINVAL, "kh_trie_changes_since: no open savepoint"};
  if (level > h->sps.size()) throw KhError{KH_EINVAL, "kh_trie_changes_since: level beyond the open savepoints"};
  const Savepoint& sp = level ? *h->sps[level - 1] : *h->sps.back();
  kh_ctx* c = h->c;
  hipStream_t st = c->st;
  const ChgSrc S{recs_at((uint8_t*)h->jrec.p), (const uint32_t*)h->jidx.p, recs_of(h), (const uint8_t*)h->heap.p,
                 sp.jrec0,                     h->jrec_n - sp.jrec0,       sp.rn,      h->rn - sp.rn};
  const uint64_t N = chg_slots(S);
  if (N >= 0xFFFFFFFFull) throw KhError{KH_EINTERNAL, "kh_trie_changes_since: 2^32 candidates"};
  Page& P = Q.P;
  Q.A = chg_side(S, !reverse);
  Q.B = chg_side(S, reverse);
  P.A = &Q.A;
  P.B = &Q.B;
  g_chg_sorts = 0;
  if (N == 0) {
    *more = 0;
    if (n_total) *n_total = 0;
    *o.n_entries = *o.val_bytes = 0;
    return KH_OK;
  }
  const uint64_t me = std::min(max_entries, N);  // (no more differences than candidates)
  Layout L;
  uint32_t *keep, *pos, *sv[2], *ja, *jb, *flag, *dpos, *ia, *ib, *tr;
  uint64_t* ck[2];
  void* rs;
  unsigned long long* cw;
  Work w;
  L.add_all(N, keep, pos, sv[0], sv[1], ja, jb, flag, dpos, ck[0], ck[1]);
  // (the sort is of the kept slots: fewer keys may take smaller tiles, and so more of them, than
  // N would -- at most at 65536 keys, the largest sort with small tiles, prims.h RS_SMALL_N)
  L.add(rs, std::max(radix_scratch_size(N), radix_scratch_size(std::min<uint64_t>(N, 65536))));
  L.add_all(me + 2, ia, ib, tr, w.cnt);
  L.add(w.scr, scan_scratch_size(std::max(N, me + 2) + 1, 8));
  L.add(w.tot, T_WORDS);
  L.add(cw, CW_WORDS);
  place(h->gbuf, L);
  // ---- collect, compact
  HIPCHK(hipMemsetAsync(cw, 0, CW_WORDS * 8, st));
  HIPCHK(hipMemsetAsync(w.tot, 0, T_WORDS * 8, st));
  hipLaunchKernelGGL(k_chg_collect, GRID(S.jn + S.an, BS), dim3(BS), 0, st, S, keep);
  LAUNCH_CHECK();
  scan_u32(keep, pos, N, (uint32_t*)(cw + CW_KEPT), w.scr, st);
  HIPCHK(hipMemcpyAsync(c->h_pinned + PIN_CHG, cw, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  const uint64_t nc = c->h_pinned[PIN_CHG + CW_KEPT];
  KeyRange from;
  memset(&from, 0, sizeof(from));
  if (from32) memcpy(from.o, from32, 32);
  const bool has_from = from32 != nullptr;
  const uint32_t ft = h->forest ? from_trie : 0u;
  uint64_t nd = 0;
  // ---- order, join: on the key's first word (and the trie id), again on all four after a tie
  for (int full = 0; nc && full < 2; ++full) {
    hipLaunchKernelGGL(k_chg_compact, GRID(N, BS), dim3(BS), 0, st, (const uint32_t*)keep, (const uint32_t*)pos, N,
                       sv[0]);
    LAUNCH_CHECK();
    int cur = 0;
    const uint32_t words[5] = {3, 2, 1, 0, CHG_WORD_TRIE};
    for (int i = full ? 0 : 3; i < (h->forest ? 5 : 4); ++i) {
      hipLaunchKernelGGL(k_chg_sortkey, GRID(nc, BS), dim3(BS), 0, st, S, (const uint32_t*)sv[cur], nc, words[i],
                         ck[cur]);
      LAUNCH_CHECK();
      if (sort_pairs_u64(ck[cur], sv[cur], ck[cur ^ 1], sv[cur ^ 1], nc, 0, words[i] == CHG_WORD_TRIE ? 32 : 64, rs, st))
        cur ^= 1;
      ++g_chg_sorts;
    }
    hipLaunchKernelGGL(k_chg_join, GRID(nc, BS), dim3(BS), 0, st, S, (const uint32_t*)sv[cur], nc,
                       (uint32_t)reverse, (uint32_t)has_from, ft, from, ja, jb, flag, cw + CW_TIE);
    LAUNCH_CHECK();
    scan_u32(flag, dpos, nc, (uint32_t*)(cw + CW_TOTAL), w.scr, st);
    hipLaunchKernelGGL(k_chg_list, GRID(nc, BS), dim3(BS), 0, st, (const uint32_t*)flag, (const uint32_t*)dpos, nc,
                       me + 1, (const uint32_t*)ja, (const uint32_t*)jb, ia, ib);
    LAUNCH_CHECK();
    HIPCHK(hipMemcpyAsync(c->h_pinned + PIN_CHG, cw, CW_WORDS * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    nd = c->h_pinned[PIN_CHG + CW_TOTAL];
    if (full || !c->h_pinned[PIN_CHG + CW_TIE]) break;  // (all four words sorted: neighbours may share the first)
  }
  if (n_total) *n_total = nd;
  // ---- page: the trie diff's tail over the items
  const DSide &A = Q.A, &B = Q.B;
  const uint64_t ni = std::min(nd, me + 1);
  if (ni) hipLaunchKernelGGL(k_chg_tries, GRID(ni, BS), dim3(BS), 0, st, A, B, (const uint32_t*)ia, (const uint32_t*)ib, ni, tr);
  LAUNCH_CHECK();
  P.ia = ia;
  P.ib = ib;
  P.pos = w.cnt;
  Q.d_tr = tr;
  const int rc = fit_page(
      c, CHANGES, w, ni, me, h, h, P, o,
      [&](uint64_t n1, uint64_t nent) {
        hipLaunchKernelGGL(k_diff_lens, GRID(n1, BS), dim3(BS), 0, st, A, B, P.ia, P.ib, n1, nent, w.cnt,
                           w.tot + T_STUB);
      },
      [&](uint64_t n1, uint64_t nent) {
        hipLaunchKernelGGL(k_diff_fit, GRID(nent + 1, BS), dim3(BS), 0, st, A, B, P.ia, P.ib, n1, w.cnt, nent,
                           (const uint64_t*)(w.tot + T_VALS), val_cap, w.tot + T_K, (uint64_t*)(w.tot + T_KEY));
      });
  if (rc != KH_OK) return rc;
  *more = P.k < P.n1;
  if (*more) {  // (the next pair's key came with the fit; its trie id is item k's)
    HIPCHK(hipMemcpyAsync(c->h_pinned + PIN_NEXT_TRIE, tr + P.k, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    Q.next_trie = (uint32_t)c->h_pinned[PIN_NEXT_TRIE];
  }
  return rc;
}
static bool changes_args_ok(kh_trie* h, uint32_t flags, bool ptrs, uint64_t max_entries) {
  if (!page_args_ok(h && ptrs, false, 0, max_entries)) return false;
  return !(flags & ~(uint32_t)KH_CHANGES_REVERSE) || refuse("kh_trie_changes_since: unknown flags");
}

extern "C" {

int kh_trie_changes_since_host(kh_trie* h, uint32_t level, uint32_t flags, uint32_t from_trie, const uint8_t from32[32],
                               uint64_t max_entries, uint64_t val_cap, uint32_t* tries, uint8_t* keys32, uint8_t* kinds,
                               uint8_t* vals, uint64_t* voff, uint64_t* n_entries, uint64_t* val_bytes,
                               uint64_t* n_total, int* more, uint32_t* next_trie, uint8_t next32[32]) {
  if (!changes_args_ok(h, flags, keys32 && kinds && voff && n_entries && val_bytes && more && next_trie && next32,
                       max_entries))
    return KH_EINVAL;
  if (h->forest && !tries) return set_err(KH_EINVAL, "kh_trie_changes_since: a forest needs the tries output");
  API_TRY({
    HANDLE_LOCK(h);
    HIPCHK(hipSetDevice(h->c->dev));
    ChgPage Q;
    const int rc = changes_scan(h, level, (flags & KH_CHANGES_REVERSE) != 0, from_trie, from32, max_entries, val_cap, Q,
                                {n_entries, val_bytes, next32, nullptr}, n_total, more);
    if (rc != KH_OK) return rc;
    if (*more) *next_trie = Q.next_trie;
    if (tries && Q.P.k)
      HIPCHK(hipMemcpyAsync(tries, Q.d_tr, Q.P.k * 4, hipMemcpyDeviceToHost, h->c->st));  // (page_to_host syncs)
    page_to_host(h, h, Q.P, keys32, kinds, vals, voff, nullptr);
  })
}

int kh_dev_trie_changes_since(kh_trie* h, uint32_t level, uint32_t flags, uint32_t from_trie, const uint8_t from32[32],
                              uint64_t max_entries, uint64_t val_cap, uint32_t* d_tries, uint8_t* d_keys32,
                              uint8_t* d_kinds, uint8_t* d_vals, uint64_t* d_voff, uint64_t* n_entries,
                              uint64_t* val_bytes, uint64_t* n_total, int* more, uint32_t* next_trie,
                              uint8_t next32[32]) {
  if (!changes_args_ok(h, flags, d_keys32 && d_kinds && d_voff && n_entries && val_bytes && more && next_trie && next32,
                       max_entries))
    return KH_EINVAL;
  if (h->forest && !d_tries) return set_err(KH_EINVAL, "kh_trie_changes_since: a forest needs the tries output");
  if (((uintptr_t)d_voff) & 7) return set_err(KH_EINVAL, "voff must be 8-byte aligned");
  API_TRY({
    HANDLE_LOCK(h);
    HIPCHK(hipSetDevice(h->c->dev));
    ChgPage Q;
    const int rc = changes_scan(h, level, (flags & KH_CHANGES_REVERSE) != 0, from_trie, from32, max_entries, val_cap, Q,
                                {n_entries, val_bytes, next32, nullptr}, n_total, more);
    if (rc != KH_OK) return rc;
    if (*more) *next_trie = Q.next_trie;
    if (d_tries && Q.P.k)
      HIPCHK(hipMemcpyAsync(d_tries, Q.d_tr, Q.P.k * 4, hipMemcpyDeviceToDevice, h->c->st));  // (page_in_place syncs)
    page_in_place(h, h, Q.P, d_keys32, d_kinds, d_vals, d_voff, nullptr);
  })
}

int kh_trie_diffs_host(kh_trie* a, const uint32_t* tries_a, kh_trie* b, const uint32_t* tries_b,
                       const uint8_t* origins32, const uint8_t* limits32, uint64_t nq, uint64_t max_entries,
                       uint64_t val_cap, uint8_t* keys32, uint8_t* kinds, uint8_t* vals, uint64_t* voff,
                       uint64_t* ent_off, uint64_t* n_entries, uint64_t* val_bytes, uint64_t* n_done,
                       uint8_t next32[32], uint8_t missing32[32]) {
  if (!page_args_ok(a && b && keys32 && kinds && voff && ent_off && n_entries && val_bytes && n_done && next32, true,
                    nq, max_entries) ||
      !diffs_ids_ok(a, tries_a, b, tries_b) || !pair_ok(a, b))
    return KH_EINVAL;
  API_TRY({
    DIFF_ENTER(a, b);
    const bool own_b = b->forest && tries_b && tries_b != tries_a;  // (else b's ids are a's array)
    Requests d;
    stage_requests(a->c, d, nq, tries_a, tries_a != nullptr && (a->forest || (b->forest && !own_b)), true, tries_b,
                   own_b, origins32, limits32);
    Page P;
    const int rc = diffs_scan(a, a->forest ? d.ta : nullptr, b, b->forest ? (own_b ? d.tb : d.ta) : nullptr, d.o, d.l,
                              nq, max_entries, val_cap, P, {n_entries, val_bytes, next32, missing32}, n_done);
    if (rc != KH_OK) return rc;
    page_to_host(a, b, P, keys32, kinds, vals, voff, ent_off);
  })
}

int kh_dev_trie_diffs(kh_trie* a, const uint32_t* d_tries_a, kh_trie* b, const uint32_t* d_tries_b,
                      const uint8_t* d_origins32, const uint8_t* d_limits32, uint64_t nq, uint64_t max_entries,
                      uint64_t val_cap, uint8_t* d_keys32, uint8_t* d_kinds, uint8_t* d_vals, uint64_t* d_voff,
                      uint64_t* d_ent_off, uint64_t* n_entries, uint64_t* val_bytes, uint64_t* n_done,
                      uint8_t next32[32], uint8_t missing32[32]) {
  if (!page_args_ok(a && b && d_keys32 && d_kinds && d_voff && d_ent_off && n_entries && val_bytes && n_done && next32,
                    true, nq, max_entries) ||
      !diffs_ids_ok(a, d_tries_a, b, d_tries_b) || !pair_ok(a, b))
    return KH_EINVAL;
  if ((((uintptr_t)d_voff) | ((uintptr_t)d_ent_off)) & 7) return set_err(KH_EINVAL, "voff and ent_off must be 8-byte aligned");
  API_TRY({
    DIFF_ENTER(a, b);
    Page P;
    const int rc = diffs_scan(a, a->forest ? d_tries_a : nullptr, b,
                              b->forest ? (d_tries_b ? d_tries_b : d_tries_a) : nullptr, d_origins32, d_limits32, nq,
                              max_entries, val_cap, P, {n_entries, val_bytes, next32, missing32}, n_done);
    if (rc != KH_OK) return rc;
    page_in_place(a, b, P, d_keys32, d_kinds, d_vals, d_voff, d_ent_off);
  })
}

int kh_trie_diff_host(kh_trie* a, uint32_t trie_a, kh_trie* b, uint32_t trie_b, const uint8_t origin32[32],
                      const uint8_t limit32[32], uint64_t max_entries, uint64_t val_cap, uint8_t* keys32,
                      uint8_t* kinds, uint8_t* vals, uint64_t* voff, uint64_t* n_entries, uint64_t* val_bytes,
                      int* more, uint8_t next32[32], uint8_t missing32[32]) {
  if (!page_args_ok(a && b && keys32 && kinds && voff && n_entries && val_bytes && more && next32, false, 0,
                    max_entries) ||
      !pair_ok(a, b))
    return KH_EINVAL;
  API_TRY({
    DIFF_ENTER(a, b);
    Page P;
    const int rc = diff_scan(a, trie_a, b, trie_b, origin32, limit32, max_entries, val_cap, P,
                             {n_entries, val_bytes, next32, missing32}, more);
    if (rc != KH_OK) return rc;
    page_to_host(a, b, P, keys32, kinds, vals, voff, nullptr);
  })
}

int kh_dev_trie_diff(kh_trie* a, uint32_t trie_a, kh_trie* b, uint32_t trie_b, const uint8_t origin32[32],
                     const uint8_t limit32[32], uint64_t max_entries, uint64_t val_cap, uint8_t* d_keys32,
                     uint8_t* d_kinds, uint8_t* d_vals, uint64_t* d_voff, uint64_t* n_entries, uint64_t* val_bytes,
                     int* more, uint8_t next32[32], uint8_t missing32[32]) {
  if (!page_args_ok(a && b && d_keys32 && d_kinds && d_voff && n_entries && val_bytes && more && next32, false, 0,
                    max_entries) ||
      !pair_ok(a, b))
    return KH_EINVAL;
  if (((uintptr_t)d_voff) & 7) return set_err(KH_EINVAL, "voff must be 8-byte aligned");
  API_TRY({
    DIFF_ENTER(a, b);
    Page P;
    const int rc = diff_scan(a, trie_a, b, trie_b, origin32, limit32, max_entries, val_cap, P,
                             {n_entries, val_bytes, next32, missing32}, more);
    if (rc != KH_OK) return rc;
    page_in_place(a, b, P, d_keys32, d_kinds, d_vals, d_voff, nullptr);
  })
}

int kh_trie_ranges_host(kh_trie* h, const uint32_t* tries, const uint8_t* origins32, const uint8_t* limits32,
                        uint64_t nq, uint64_t max_entries, uint8_t* keys32, uint8_t* vals, uint64_t val_cap,
                        uint64_t* voff, uint64_t* ent_off, uint64_t* n_entries, uint64_t* val_bytes, uint64_t* n_done,
                        uint8_t next32[32], uint8_t missing32[32]) {
  if (!page_args_ok(h && keys32 && voff && ent_off && n_entries && val_bytes && n_done && next32, true, nq,
                    max_entries) ||
      !ranges_ids_ok(h, tries))
    return KH_EINVAL;
  API_TRY({
    HANDLE_LOCK(h);
    HIPCHK(hipSetDevice(h->c->dev));
    Requests d;
    stage_requests(h->c, d, nq, tries, h->forest, false, nullptr, false, origins32, limits32);
    Page P;
    const int rc = ranges_scan(h, d.ta, d.o, d.l, nq, max_entries, val_cap, P,
                               {n_entries, val_bytes, next32, missing32}, n_done);
    if (rc != KH_OK) return rc;
    page_to_host(h, nullptr, P, keys32, nullptr, vals, voff, ent_off);
  })
}

int kh_dev_trie_ranges(kh_trie* h, const uint32_t* d_tries, const uint8_t* d_origins32, const uint8_t* d_limits32,
                       uint64_t nq, uint64_t max_entries, uint8_t* d_keys32, uint8_t* d_vals, uint64_t val_cap,
                       uint64_t* d_voff, uint64_t* d_ent_off, uint64_t* n_entries, uint64_t* val_bytes,
                       uint64_t* n_done, uint8_t next32[32], uint8_t missing32[32]) {
  if (!page_args_ok(h && d_keys32 && d_voff && d_ent_off && n_entries && val_bytes && n_done && next32, true, nq,
                    max_entries) ||
      !ranges_ids_ok(h, d_tries))
    return KH_EINVAL;
  if ((((uintptr_t)d_voff) | ((uintptr_t)d_ent_off)) & 7) return set_err(KH_EINVAL, "voff and ent_off must be 8-byte aligned");
  API_TRY({
    HANDLE_LOCK(h);
    HIPCHK(hipSetDevice(h->c->dev));
    Page P;
    const int rc = ranges_scan(h, h->forest ? d_tries : nullptr, d_origins32, d_limits32, nq, max_entries, val_cap, P,
                               {n_entries, val_bytes, next32, missing32}, n_done);
    if (rc != KH_OK) return rc;
    page_in_place(h, nullptr, P, d_keys32, nullptr, d_vals, d_voff, d_ent_off);
  })
}

int kh_trie_range_host(kh_trie* h, uint32_t trie, const uint8_t origin32[32], const uint8_t limit32[32],
                       uint64_t max_entries, uint8_t* keys32, uint8_t* vals, uint64_t val_cap, uint64_t* voff,
                       uint64_t* n_entries, uint64_t* val_bytes, int* more, uint8_t next32[32], uint8_t missing32[32]) {
  if (!page_args_ok(h && keys32 && voff && n_entries && val_bytes && more && next32, false, 0, max_entries))
    return KH_EINVAL;
  API_TRY({
    HANDLE_LOCK(h);
    HIPCHK(hipSetDevice(h->c->dev));
    Page P;
    const int rc = range_scan(h, trie, origin32, limit32, max_entries, val_cap, P,
                              {n_entries, val_bytes, next32, missing32}, more);
    if (rc != KH_OK) return rc;
    page_to_host(h, nullptr, P, keys32, nullptr, vals, voff, nullptr);
  })
}

int kh_dev_trie_range(kh_trie* h, uint32_t trie, const uint8_t origin32[32], const uint8_t limit32[32],
                      uint64_t max_entries, uint8_t* d_keys32, uint8_t* d_vals, uint64_t val_cap, uint64_t* d_voff,
                      uint64_t* n_entries, uint64_t* val_bytes, int* more, uint8_t next32[32], uint8_t missing32[32]) {
  if (!page_args_ok(h && d_keys32 && d_voff && n_entries && val_bytes && more && next32, false, 0, max_entries))
    return KH_EINVAL;
  API_TRY({
    HANDLE_LOCK(h);
    HIPCHK(hipSetDevice(h->c->dev));
    Page P;
    const int rc = range_scan(h, trie, origin32, limit32, max_entries, val_cap, P,
                              {n_entries, val_bytes, next32, missing32}, more);
    if (rc != KH_OK) return rc;
    page_in_place(h, nullptr, P, d_keys32, nullptr, d_vals, d_voff, nullptr);
  })
}

}  // extern "C"

