// kh_trie_range_host / kh_dev_trie_range and the batched kh_trie_ranges_host / kh_dev_trie_ranges:
// their kernels (k_ranges_*: range.h holds the bodies of both), then the host drivers range_scan and
// ranges_scan and the C entry points (host.h).  kh_trie_diff_host / kh_dev_trie_diff, the same
// ordered frontier run over two tries in lockstep (diff.h: k_diff_*, diff_scan), and the batched
// kh_trie_diffs_host / kh_dev_trie_diffs (k_diffs_*, diffs_scan) live here too.
// A cold compilation unit of its own like prove_kernels.hip and load_kernels.hip: the hot kernels
// of khst.hip keep their placement (tests/test_code_layout.py).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "diff.h"
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

// ---------------------------------------------------------------------------
// host: range scan (range.h)
// ---------------------------------------------------------------------------
// what the rounds leave in the handle's gbuf for the write: the final frontier, the scanned value
// offsets, the entries that fit
struct RangePage {
  const uint32_t* items = nullptr;
  const uint64_t* pos = nullptr;
  uint64_t k = 0, bytes = 0;
  uint32_t rounds = 0;
};
static uint32_t g_range_rounds = 0;  // rounds of the last scan (khst_range_rounds: measurements only)
extern "C" uint32_t khst_range_rounds() { return g_range_rounds; }

// The rounds of a range scan (range.h) and the fit to val_cap.  Two frontiers of max_entries + 2
// items, one sync of a pinned word triple a round.  KH_OK with the page described in P (P.k = 0:
// an empty answer) and *n_entries, *val_bytes, *more, next32 set; KH_ENOSPC with *val_bytes;
// KH_ENODE with missing32.
static int range_scan(kh_trie* h, uint32_t trie, const uint8_t* origin32, const uint8_t* limit32, uint64_t max_entries,
                      uint64_t val_cap, RangePage& P, uint64_t* n_entries, uint64_t* val_bytes, int* more,
                      uint8_t* next32, uint8_t* missing32) {
  trie_settle(h);
  kh_ctx* c = h->c;
  hipStream_t st = c->st;
  KeyRange g;
  memset(g.o, 0, 32);
  memset(g.l, 0xFF, 32);
  if (origin32) memcpy(g.o, origin32, 32);
  if (limit32) memcpy(g.l, limit32, 32);
  const uint32_t t = h->forest ? trie : 0u;
  // (no more entries than records: the frontiers of a call asking for 2^31 - 1 stay the trie's size)
  const uint64_t me = std::min<uint64_t>(max_entries, std::max<uint64_t>(h->rn, 1));
  const uint64_t F = me + 2;
  Layout L;
  uint32_t *fa, *fb;
  uint64_t* cnt;
  unsigned long long* tot;
  char* scr;
  L.add(fa, F + 1);
  L.add(fb, F + 1);
  L.add(cnt, F + 1);
  L.add(scr, scan_scratch_size(F + 1, 8));
  L.add(tot, 16);
  place(h->gbuf, L);
  uint64_t ni = 0;
  uint32_t rounds = 0;
  uint32_t *cur = fa, *nxt = fb;
  if (h->rn && h->mcap && key_cmp(g.o, g.l) <= 0) {
    const Recs R = recs_of(h);
    const AMap M = map_of(h);
    HIPCHK(hipMemsetAsync(tot, 0, 16 * 8, st));
    // (an empty trie, or an id the forest does not hold: the item is NONE and the first count drops it)
    hipLaunchKernelGGL(k_range_root, dim3(1), dim3(1), 0, st, M, R, t, fa);
    LAUNCH_CHECK();
    for (ni = 1; ni; ++rounds) {
      if (rounds > 66) throw KhError{KH_EINTERNAL, "range scan: the rounds do not end"};
      HIPCHK(hipMemsetAsync(tot, 0, 16, st));  // [0] the items of the next frontier, [1] any branch among these
      hipLaunchKernelGGL(k_range_count, GRID(ni, BS), dim3(BS), 0, st, R, g, cur, ni, cnt, tot + 1);
      LAUNCH_CHECK();
      scan_u64(cnt, cnt, ni, (uint64_t*)tot, scr, st);
      HIPCHK(hipMemcpyAsync(c->h_pinned, tot, 24, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      const uint64_t total = c->h_pinned[0], expand = c->h_pinned[1];
      if (c->h_pinned[2]) throw KhError{KH_EINTERNAL, "range scan: corrupt anchor map"};
      const uint64_t nn = std::min(total, F);  // the cut
      if (nn) {
        hipLaunchKernelGGL(k_range_fill, GRID(ni * EXP_LANES, BS), dim3(BS), 0, st, M, R, g, cur, ni,
                           (const uint64_t*)cnt, F, nxt, tot + 2);
        LAUNCH_CHECK();
      }
      std::swap(cur, nxt);
      ni = nn;
      if (!expand) {
        ++rounds;
        break;
      }
    }
  }
  P.rounds = g_range_rounds = rounds;
  P.items = cur;
  P.pos = cnt;
  P.k = P.bytes = 0;
  const uint64_t n1 = std::min(ni, me + 1), nent = std::min(ni, me);
  if (n1 == 0) {
    *n_entries = *val_bytes = 0;
    *more = 0;
    return KH_OK;
  }
  const Recs R = recs_of(h);
  HIPCHK(hipMemsetAsync(tot + 3, 0xFF, 8, st));
  hipLaunchKernelGGL(k_range_lens, GRID(n1, BS), dim3(BS), 0, st, R, cur, n1, nent, cnt, tot + 3);
  LAUNCH_CHECK();
  scan_u64(cnt, cnt, nent, (uint64_t*)(tot + 12), scr, st);
  hipLaunchKernelGGL(k_range_fit, GRID(nent + 1, BS), dim3(BS), 0, st, R, cur, n1, (const uint64_t*)cnt, nent,
                     (const uint64_t*)(tot + 12), val_cap, tot + 4, (uint64_t*)(tot + 8));
  LAUNCH_CHECK();
  HIPCHK(hipMemcpyAsync(c->h_pinned, tot, 16 * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (c->h_pinned[2]) throw KhError{KH_EINTERNAL, "range scan: corrupt anchor map"};
  if (c->h_pinned[3] != ~0ULL) {  // a missing subtree among the first max_entries + 1 things in range
    const uint64_t r = (uint32_t)c->h_pinned[3];
    HIPCHK(hipMemcpyAsync(c->h_pinned + 16, (const uint8_t*)h->recs.p + r * REC_BYTES + 96, 32, hipMemcpyDeviceToHost,
                          st));
    HIPCHK(hipStreamSynchronize(st));
    if (missing32) memcpy(missing32, c->h_pinned + 16, 32);
    return set_err(KH_ENODE, "the range meets a subtree the handle does not hold (missing32 names its node)");
  }
  const uint64_t k = c->h_pinned[4];
  if (k == 0) {
    *val_bytes = c->h_pinned[6];
    return set_err(KH_ENOSPC, "value output too small for the first entry (*val_bytes holds its size)");
  }
  P.k = k;
  P.bytes = c->h_pinned[5];
  *n_entries = k;
  *val_bytes = P.bytes;
  *more = k < n1;
  if (k < n1) memcpy(next32, c->h_pinned + 8, 32);
  return KH_OK;
}
// the page's keys, offsets and values into device buffers (P.k > 0)
static void range_emit(kh_trie* h, const RangePage& P, uint8_t* d_keys32, uint8_t* d_vals, uint64_t* d_voff) {
  hipLaunchKernelGGL(k_range_write, GRID(P.k + 1, BS), dim3(BS), 0, h->c->st, recs_of(h), (const uint8_t*)h->heap.p,
                     P.items, P.k, P.pos, P.bytes, d_keys32, d_voff, d_vals);
  LAUNCH_CHECK();
}
static bool range_args_ok(kh_trie* h, uint64_t max_entries, const void* keys32, const void* voff,
                          const uint64_t* n_entries, const uint64_t* val_bytes, const int* more, const uint8_t* next32) {
  if (!h || !keys32 || !voff || !n_entries || !val_bytes || !more || !next32) {
    set_err(KH_EINVAL, "null handle or outputs");
    return false;
  }
  if (max_entries == 0 || max_entries >= (1ULL << 31)) {
    set_err(KH_EINVAL, "max_entries must be in [1, 2^31)");
    return false;
  }
  return true;
}

// ---- many ranges a call (range.h "MANY RANGES A CALL")
// The rounds of nq range scans moving together and the fit to val_cap: the requests (device
// arrays; d_tries NULL on a single trie, d_origins / d_limits nullable) through two segmented
// frontiers of max_entries + 2 * nq items (range.h derives the cut), one sync of a pinned word
// triple a round.  KH_OK with the answer described in P (P.k = 0: nothing in any range) and
// *n_entries, *val_bytes, *n_done, next32 set; KH_ENOSPC with *val_bytes; KH_ENODE with missing32
// and *n_done.
static int ranges_scan(kh_trie* h, const uint32_t* d_tries, const uint8_t* d_origins, const uint8_t* d_limits,
                       uint64_t nq, uint64_t max_entries, uint64_t val_cap, RangePage& P, const uint32_t*& P_iq,
                       uint64_t* n_entries, uint64_t* val_bytes, uint64_t* n_done, uint8_t* next32,
                       uint8_t* missing32) {
  trie_settle(h);
  kh_ctx* c = h->c;
  hipStream_t st = c->st;
  // (a request returns no more entries than the handle has records: the frontiers of a call asking
  // for 2^31 - 1 follow the handle and nq)
  const uint64_t me = std::min<uint64_t>(max_entries, nq * std::max<uint64_t>(h->rn, 1));
  const uint64_t F = me + 2 * nq;
  Layout L;
  uint32_t *fa, *fb, *qa, *qb;
  uint64_t* cnt;
  unsigned long long* tot;
  KeyRange* G;
  char* scr;
  L.add(fa, F + 1);
  L.add(fb, F + 1);
  L.add(qa, F + 1);
  L.add(qb, F + 1);
  L.add(cnt, F + 1);
  L.add(G, nq);
  L.add(scr, scan_scratch_size(F + 1, 8));
  L.add(tot, 16);
  place(h->gbuf, L);
  uint64_t ni = 0;
  uint32_t rounds = 0;
  uint32_t *cur = fa, *nxt = fb, *curq = qa, *nxtq = qb;
  if (h->rn && h->mcap) {
    const Recs R = recs_of(h);
    const AMap M = map_of(h);
    HIPCHK(hipMemsetAsync(tot, 0, 16 * 8, st));
    hipLaunchKernelGGL(k_ranges_root, GRID(nq, BS), dim3(BS), 0, st, M, R, d_tries, d_origins, d_limits, nq, G, fa, qa);
    LAUNCH_CHECK();
    for (ni = nq; ni; ++rounds) {
      if (rounds > 66) throw KhError{KH_EINTERNAL, "range scan: the rounds do not end"};
      HIPCHK(hipMemsetAsync(tot, 0, 16, st));  // [0] the items of the next frontier, [1] any branch among these
      hipLaunchKernelGGL(k_ranges_count, GRID(ni, BS), dim3(BS), 0, st, R, (const KeyRange*)G, cur, curq, ni, cnt,
                         tot + 1);
      LAUNCH_CHECK();
      scan_u64(cnt, cnt, ni, (uint64_t*)tot, scr, st);
      HIPCHK(hipMemcpyAsync(c->h_pinned, tot, 24, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      const uint64_t total = c->h_pinned[0], expand = c->h_pinned[1];
      if (c->h_pinned[2]) throw KhError{KH_EINTERNAL, "range scan: corrupt anchor map"};
      const uint64_t nn = std::min(total, F);  // the cut
      if (nn) {
        hipLaunchKernelGGL(k_ranges_fill, GRID(ni * EXP_LANES, BS), dim3(BS), 0, st, M, R, (const KeyRange*)G, cur, curq,
                           ni, (const uint64_t*)cnt, F, nxt, nxtq, tot + 2);
        LAUNCH_CHECK();
      }
      std::swap(cur, nxt);
      std::swap(curq, nxtq);
      ni = nn;
      if (!expand) {
        ++rounds;
        break;
      }
    }
  }
  P.rounds = g_range_rounds = rounds;
  P.items = cur;
  P_iq = curq;
  P.pos = cnt;
  P.k = P.bytes = 0;
  const uint64_t n1 = std::min(ni, me + 1), nent = std::min(ni, me);
  if (n1 == 0) {
    *n_entries = *val_bytes = 0;
    *n_done = nq;
    return KH_OK;
  }
  const Recs R = recs_of(h);
  HIPCHK(hipMemsetAsync(tot + 3, 0xFF, 8, st));
  hipLaunchKernelGGL(k_range_lens, GRID(n1, BS), dim3(BS), 0, st, R, cur, n1, nent, cnt, tot + 3);
  LAUNCH_CHECK();
  scan_u64(cnt, cnt, nent, (uint64_t*)(tot + 12), scr, st);
  // fit: [4] k, [5] its bytes, [6] the length of entry k alone, [7] the request of thing k; [8..12) its key
  hipLaunchKernelGGL(k_ranges_fit, GRID(nent + 1, BS), dim3(BS), 0, st, R, cur, curq, n1, (const uint64_t*)cnt, nent,
                     (const uint64_t*)(tot + 12), val_cap, nq, tot + 4, (uint64_t*)(tot + 8));
  LAUNCH_CHECK();
  HIPCHK(hipMemcpyAsync(c->h_pinned, tot, 16 * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (c->h_pinned[2]) throw KhError{KH_EINTERNAL, "range scan: corrupt anchor map"};
  if (c->h_pinned[3] != ~0ULL) {  // a missing subtree among the first max_entries + 1 things of the answer
    const uint64_t r = (uint32_t)c->h_pinned[3], at = c->h_pinned[3] >> 32;
    HIPCHK(hipMemcpyAsync(c->h_pinned + 16, (const uint8_t*)h->recs.p + r * REC_BYTES + 96, 32, hipMemcpyDeviceToHost,
                          st));
    HIPCHK(hipMemcpyAsync(c->h_pinned + 20, curq + at, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (missing32) memcpy(missing32, c->h_pinned + 16, 32);
    *n_done = (uint32_t)c->h_pinned[20];
    return set_err(KH_ENODE, "a range meets a subtree the handle does not hold (missing32 names its node, "
                             "*n_done the request)");
  }
  const uint64_t k = c->h_pinned[4];
  if (k == 0) {
    *val_bytes = c->h_pinned[6];
    return set_err(KH_ENOSPC, "value output too small for the first entry (*val_bytes holds its size)");
  }
  P.k = k;
  P.bytes = c->h_pinned[5];
  *n_entries = k;
  *val_bytes = P.bytes;
  *n_done = k < n1 ? c->h_pinned[7] : nq;
  if (k < n1) memcpy(next32, c->h_pinned + 8, 32);
  return KH_OK;
}
// the answer's keys, value offsets, values and request offsets into device buffers (P.k > 0)
static void ranges_emit(kh_trie* h, const RangePage& P, const uint32_t* iq, uint64_t nq, uint8_t* d_keys32,
                        uint8_t* d_vals, uint64_t* d_voff, uint64_t* d_ent_off) {
  hipLaunchKernelGGL(k_ranges_write, GRID(std::max(P.k, nq) + 1, BS), dim3(BS), 0, h->c->st, recs_of(h),
                     (const uint8_t*)h->heap.p, P.items, iq, P.k, P.pos, P.bytes, nq, d_keys32, d_voff, d_vals,
                     d_ent_off);
  LAUNCH_CHECK();
}
static bool ranges_args_ok(kh_trie* h, const uint32_t* tries, uint64_t nq, uint64_t max_entries, const void* keys32,
                           const void* voff, const void* ent_off, const uint64_t* n_entries, const uint64_t* val_bytes,
                           const uint64_t* n_done, const uint8_t* next32) {
  if (!h || !keys32 || !voff || !ent_off || !n_entries || !val_bytes || !n_done || !next32) {
    set_err(KH_EINVAL, "null handle or outputs");
    return false;
  }
  if (nq == 0 || max_entries == 0 || nq >= (1ULL << 31) || max_entries >= (1ULL << 31) ||
      nq + max_entries >= (1ULL << 31)) {
    set_err(KH_EINVAL, "nq and max_entries must be at least 1 and nq + max_entries < 2^31");
    return false;
  }
  if (h->forest && !tries) {
    set_err(KH_EINVAL, "a forest needs a trie id per request");
    return false;
  }
  return true;
}

// ---------------------------------------------------------------------------
// host: trie diff (diff.h)
// ---------------------------------------------------------------------------
// what the rounds leave in a's gbuf for the write: the final frontier's two record columns, the
// scanned value offsets, the differences that fit
struct DiffPage {
  const uint32_t *ia = nullptr, *ib = nullptr;
  const uint64_t* pos = nullptr;
  uint64_t k = 0, bytes = 0;
};
static uint32_t g_diff_rounds = 0;   // rounds of the last diff past the root pair, and the frontier
static uint64_t g_diff_visited = 0;  // items it selected in them (khst_diff_*: measurements only)
extern "C" uint32_t khst_diff_rounds() { return g_diff_rounds; }
extern "C" uint64_t khst_diff_visited() { return g_diff_visited; }

static DSide side_of(kh_trie* h) {
  return DSide{recs_of(h), h->mcap ? map_of(h) : AMap{{nullptr}, {nullptr}, 0}, (const uint8_t*)h->heap.p};
}

// The rounds of a diff (diff.h) and the fit to val_cap, on a's stream with the scratch in a's gbuf
// (both handles locked and settled by the caller, b's stream drained).  Two frontiers of
// max_entries + 2 items, one sync of a pinned word triple a round.  KH_OK with the page described
// in P (P.k = 0: no difference) and *n_entries, *val_bytes, *more, next32 set; KH_ENOSPC with
// *val_bytes; KH_ENODE with missing32.
static int diff_scan(kh_trie* a, uint32_t trie_a, kh_trie* b, uint32_t trie_b, const uint8_t* origin32,
                     const uint8_t* limit32, uint64_t max_entries, uint64_t val_cap, DiffPage& P, uint64_t* n_entries,
                     uint64_t* val_bytes, int* more, uint8_t* next32, uint8_t* missing32) {
  kh_ctx* c = a->c;
  hipStream_t st = c->st;
  KeyRange g;
  memset(g.o, 0, 32);
  memset(g.l, 0xFF, 32);
  if (origin32) memcpy(g.o, origin32, 32);
  if (limit32) memcpy(g.l, limit32, 32);
  const uint32_t ta = a->forest ? trie_a : 0u, tb = b->forest ? trie_b : 0u;
  const bool has_a = a->rn && a->mcap, has_b = b->rn && b->mcap;
  // (no more differences than records: the frontiers of a call asking for 2^31 - 1 stay the tries' size)
  const uint64_t me = std::min<uint64_t>(max_entries, std::max<uint64_t>(a->rn + b->rn, 1));
  const uint64_t F = me + 2;
  Layout L;
  uint32_t *fa[2], *fb[2], *fd[2], *sel;
  uint64_t* cnt;
  unsigned long long* tot;
  char* scr;
  for (int s = 0; s < 2; ++s) {
    L.add(fa[s], F + 1);
    L.add(fb[s], F + 1);
    L.add(fd[s], F + 1);
  }
  L.add(sel, F + 1);
  L.add(cnt, F + 1);
  L.add(scr, scan_scratch_size(F + 1, 8));
  L.add(tot, 16);
  place(a->gbuf, L);
  const DSide A = side_of(a), B = side_of(b);
  uint64_t ni = 0, visited = 0;
  uint32_t rounds = 0;
  int cur = 0;
  if ((has_a || has_b) && !(a == b && ta == tb) && key_cmp(g.o, g.l) <= 0) {
    HIPCHK(hipMemsetAsync(tot, 0, 16 * 8, st));
    hipLaunchKernelGGL(k_diff_root, dim3(1), dim3(1), 0, st, A, ta, (uint32_t)has_a, B, tb, (uint32_t)has_b, fa[0],
                       fb[0], fd[0], tot + 15);
    LAUNCH_CHECK();
    HIPCHK(hipMemcpyAsync(c->h_pinned, tot + 15, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (ni = c->h_pinned[0]; ni; ++rounds) {
      if (rounds > 68) throw KhError{KH_EINTERNAL, "trie diff: the rounds do not end"};
      visited += ni;
      HIPCHK(hipMemsetAsync(tot, 0, 16, st));  // [0] the items of the next frontier, [1] any item expanded or split
      hipLaunchKernelGGL(k_diff_select, GRID(ni * EXP_LANES, BS), dim3(BS), 0, st, A, B, g, (const uint32_t*)fa[cur],
                         (const uint32_t*)fb[cur], ni, sel, cnt, tot + 1);
      LAUNCH_CHECK();
      scan_u64(cnt, cnt, ni, (uint64_t*)tot, scr, st);
      HIPCHK(hipMemcpyAsync(c->h_pinned, tot, 24, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      const uint64_t total = c->h_pinned[0], expand = c->h_pinned[1];
      if (c->h_pinned[2]) throw KhError{KH_EINTERNAL, "trie diff: corrupt anchor map"};
      const uint64_t nn = std::min(total, F);  // the cut
      if (nn) {
        hipLaunchKernelGGL(k_diff_fill, GRID(ni * EXP_LANES, BS), dim3(BS), 0, st, A, B, (const uint32_t*)fa[cur],
                           (const uint32_t*)fb[cur], (const uint32_t*)fd[cur], (const uint32_t*)sel, ni,
                           (const uint64_t*)cnt, F, fa[cur ^ 1], fb[cur ^ 1], fd[cur ^ 1], tot + 2);
        LAUNCH_CHECK();
      }
      cur ^= 1;
      ni = nn;
      if (!expand) {
        ++rounds;
        break;
      }
    }
  }
  g_diff_rounds = rounds;
  g_diff_visited = visited;
  P.ia = fa[cur];
  P.ib = fb[cur];
  P.pos = cnt;
  P.k = P.bytes = 0;
  const uint64_t n1 = std::min(ni, me + 1), nent = std::min(ni, me);
  if (n1 == 0) {
    *n_entries = *val_bytes = 0;
    *more = 0;
    return KH_OK;
  }
  HIPCHK(hipMemsetAsync(tot + 3, 0xFF, 8, st));
  hipLaunchKernelGGL(k_diff_lens, GRID(n1, BS), dim3(BS), 0, st, A, B, P.ia, P.ib, n1, nent, cnt, tot + 3);
  LAUNCH_CHECK();
  scan_u64(cnt, cnt, nent, (uint64_t*)(tot + 12), scr, st);
  // fit: [4] k, [5] its bytes, [6] the bytes of difference k alone; [8..12) its key
  hipLaunchKernelGGL(k_diff_fit, GRID(nent + 1, BS), dim3(BS), 0, st, A, B, P.ia, P.ib, n1, (const uint64_t*)cnt, nent,
                     (const uint64_t*)(tot + 12), val_cap, tot + 4, (uint64_t*)(tot + 8));
  LAUNCH_CHECK();
  HIPCHK(hipMemcpyAsync(c->h_pinned, tot, 16 * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (c->h_pinned[2]) throw KhError{KH_EINTERNAL, "trie diff: corrupt anchor map"};
  if (c->h_pinned[3] != ~0ULL) {  // a missing thing among the first max_entries + 1 things in range
    const uint64_t r = (uint32_t)c->h_pinned[3];
    kh_trie* of = ((c->h_pinned[3] >> 32) & 1) ? b : a;
    HIPCHK(hipMemcpyAsync(c->h_pinned + 16, (const uint8_t*)of->recs.p + r * REC_BYTES + 96, 32, hipMemcpyDeviceToHost,
                          st));
    HIPCHK(hipStreamSynchronize(st));
    if (missing32) memcpy(missing32, c->h_pinned + 16, 32);
    return set_err(KH_ENODE, "the diff meets a subtree a handle does not hold (missing32 names its node)");
  }
  const uint64_t k = c->h_pinned[4];
  if (k == 0) {
    *val_bytes = c->h_pinned[6];
    return set_err(KH_ENOSPC, "value output too small for the first difference (*val_bytes holds its size)");
  }
  P.k = k;
  P.bytes = c->h_pinned[5];
  *n_entries = k;
  *val_bytes = P.bytes;
  *more = k < n1;
  if (k < n1) memcpy(next32, c->h_pinned + 8, 32);
  return KH_OK;
}
// the page's keys, kinds, offsets and values into device buffers (P.k > 0)
static void diff_emit(kh_trie* a, kh_trie* b, const DiffPage& P, uint8_t* d_keys32, uint8_t* d_kinds, uint8_t* d_vals,
                      uint64_t* d_voff) {
  hipLaunchKernelGGL(k_diff_write, GRID(P.k + 1, BS), dim3(BS), 0, a->c->st, side_of(a), side_of(b), P.ia, P.ib, P.k,
                     P.pos, P.bytes, d_keys32, d_kinds, d_voff, d_vals);
  LAUNCH_CHECK();
}
static bool diff_args_ok(kh_trie* a, kh_trie* b, uint64_t max_entries, const void* keys32, const void* kinds,
                         const void* voff, const uint64_t* n_entries, const uint64_t* val_bytes, const int* more,
                         const uint8_t* next32) {
  if (!a || !b || !keys32 || !kinds || !voff || !n_entries || !val_bytes || !more || !next32) {
    set_err(KH_EINVAL, "null handle or outputs");
    return false;
  }
  if (max_entries == 0 || max_entries >= (1ULL << 31)) {
    set_err(KH_EINVAL, "max_entries must be in [1, 2^31)");
    return false;
  }
  if (a->c->dev != b->c->dev) {
    set_err(KH_EINVAL, "the two handles live on different devices");
    return false;
  }
  return true;
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

// The rounds of nq diffs moving together and the fit to val_cap, on a's stream with the scratch in
// a's gbuf (both handles locked and settled by the caller, b's stream drained): the requests (device
// arrays; d_ta / d_tb NULL on a single trie, d_origins / d_limits nullable) through two segmented
// frontiers of max_entries + 2 * nq items (diff.h derives the cut), one sync of the pinned words a
// round.  KH_OK with the answer described in P and P_iq (P.k = 0: no difference in any request) and
// *n_entries, *val_bytes, *n_done, next32 set; KH_ENOSPC with *val_bytes; KH_ENODE with missing32
// and *n_done.
static int diffs_scan(kh_trie* a, const uint32_t* d_ta, kh_trie* b, const uint32_t* d_tb, const uint8_t* d_origins,
                      const uint8_t* d_limits, uint64_t nq, uint64_t max_entries, uint64_t val_cap, DiffPage& P,
                      const uint32_t*& P_iq, uint64_t* n_entries, uint64_t* val_bytes, uint64_t* n_done,
                      uint8_t* next32, uint8_t* missing32) {
  kh_ctx* c = a->c;
  hipStream_t st = c->st;
  const bool has_a = a->rn && a->mcap, has_b = b->rn && b->mcap;
  // (a request returns no more differences than the two handles have records: the frontiers of a
  // call asking for 2^31 - 1 follow the handles and nq)
  const uint64_t me = std::min<uint64_t>(max_entries, nq * std::max<uint64_t>(a->rn + b->rn, 1));
  const uint64_t F = me + 2 * nq;
  Layout L;
  uint32_t *fa[2], *fb[2], *fd[2], *fq[2], *sel;
  uint64_t* cnt;
  unsigned long long* tot;
  KeyRange* G;
  char* scr;
  for (int s = 0; s < 2; ++s) {
    L.add(fa[s], F + 1);
    L.add(fb[s], F + 1);
    L.add(fd[s], F + 1);
    L.add(fq[s], F + 1);
  }
  L.add(sel, F + 1);
  L.add(cnt, F + 1);
  L.add(G, nq);
  L.add(scr, scan_scratch_size(F + 1, 8));
  L.add(tot, 16);
  place(a->gbuf, L);
  const DSide A = side_of(a), B = side_of(b);
  uint64_t ni = 0, visited = 0;
  uint32_t rounds = 0;
  int cur = 0;
  if (has_a || has_b) {
    HIPCHK(hipMemsetAsync(tot, 0, 16 * 8, st));
    hipLaunchKernelGGL(k_diffs_root, GRID(nq, BS), dim3(BS), 0, st, A, d_ta, (uint32_t)has_a, B, d_tb, (uint32_t)has_b,
                       (uint32_t)(a == b), d_origins, d_limits, nq, G, fa[0], fb[0], fd[0], fq[0], tot + 15);
    LAUNCH_CHECK();
    HIPCHK(hipMemcpyAsync(c->h_pinned, tot + 15, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const uint64_t live = c->h_pinned[0];  // (none: every request is empty or its roots are equal -- no round)
    for (ni = live ? nq : 0; ni; ++rounds) {
      if (rounds > 68) throw KhError{KH_EINTERNAL, "trie diff: the rounds do not end"};
      visited += rounds ? ni : live;
      HIPCHK(hipMemsetAsync(tot, 0, 16, st));  // [0] the items of the next frontier, [1] any item expanded or split
      hipLaunchKernelGGL(k_diffs_select, GRID(ni * EXP_LANES, BS), dim3(BS), 0, st, A, B, (const KeyRange*)G,
                         (const uint32_t*)fa[cur], (const uint32_t*)fb[cur], (const uint32_t*)fq[cur], ni, sel, cnt,
                         tot + 1);
      LAUNCH_CHECK();
      scan_u64(cnt, cnt, ni, (uint64_t*)tot, scr, st);
      HIPCHK(hipMemcpyAsync(c->h_pinned, tot, 24, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      const uint64_t total = c->h_pinned[0], expand = c->h_pinned[1];
      if (c->h_pinned[2]) throw KhError{KH_EINTERNAL, "trie diff: corrupt anchor map"};
      const uint64_t nn = std::min(total, F);  // the cut
      if (nn) {
        hipLaunchKernelGGL(k_diffs_fill, GRID(ni * EXP_LANES, BS), dim3(BS), 0, st, A, B, (const uint32_t*)fa[cur],
                           (const uint32_t*)fb[cur], (const uint32_t*)fd[cur], (const uint32_t*)fq[cur],
                           (const uint32_t*)sel, ni, (const uint64_t*)cnt, F, fa[cur ^ 1], fb[cur ^ 1], fd[cur ^ 1],
                           fq[cur ^ 1], tot + 2);
        LAUNCH_CHECK();
      }
      cur ^= 1;
      ni = nn;
      if (!expand) {
        ++rounds;
        break;
      }
    }
  }
  g_diffs_rounds = rounds;
  g_diffs_visited = visited;
  P.ia = fa[cur];
  P.ib = fb[cur];
  P_iq = fq[cur];
  P.pos = cnt;
  P.k = P.bytes = 0;
  const uint64_t n1 = std::min(ni, me + 1), nent = std::min(ni, me);
  if (n1 == 0) {
    *n_entries = *val_bytes = 0;
    *n_done = nq;
    return KH_OK;
  }
  HIPCHK(hipMemsetAsync(tot + 3, 0xFF, 8, st));
  hipLaunchKernelGGL(k_diff_lens, GRID(n1, BS), dim3(BS), 0, st, A, B, P.ia, P.ib, n1, nent, cnt, tot + 3);
  LAUNCH_CHECK();
  scan_u64(cnt, cnt, nent, (uint64_t*)(tot + 12), scr, st);
  // fit: [4] k, [5] its bytes, [6] the bytes of difference k alone, [7] the request of thing k; [8..12) its key
  hipLaunchKernelGGL(k_diffs_fit, GRID(nent + 1, BS), dim3(BS), 0, st, A, B, P.ia, P.ib, P_iq, n1, (const uint64_t*)cnt,
                     nent, (const uint64_t*)(tot + 12), val_cap, nq, tot + 4, (uint64_t*)(tot + 8));
  LAUNCH_CHECK();
  HIPCHK(hipMemcpyAsync(c->h_pinned, tot, 16 * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (c->h_pinned[2]) throw KhError{KH_EINTERNAL, "trie diff: corrupt anchor map"};
  if (c->h_pinned[3] != ~0ULL) {  // a missing thing among the first max_entries + 1 things of the answer
    const uint64_t r = (uint32_t)c->h_pinned[3], at = c->h_pinned[3] >> 33;
    kh_trie* of = ((c->h_pinned[3] >> 32) & 1) ? b : a;
    HIPCHK(hipMemcpyAsync(c->h_pinned + 16, (const uint8_t*)of->recs.p + r * REC_BYTES + 96, 32, hipMemcpyDeviceToHost,
                          st));
    HIPCHK(hipMemcpyAsync(c->h_pinned + 20, P_iq + at, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (missing32) memcpy(missing32, c->h_pinned + 16, 32);
    *n_done = (uint32_t)c->h_pinned[20];
    return set_err(KH_ENODE, "a diff meets a subtree a handle does not hold (missing32 names its node, *n_done "
                             "the request)");
  }
  const uint64_t k = c->h_pinned[4];
  if (k == 0) {
    *val_bytes = c->h_pinned[6];
    return set_err(KH_ENOSPC, "value output too small for the first difference (*val_bytes holds its size)");
  }
  P.k = k;
  P.bytes = c->h_pinned[5];
  *n_entries = k;
  *val_bytes = P.bytes;
  *n_done = k < n1 ? c->h_pinned[7] : nq;
  if (k < n1) memcpy(next32, c->h_pinned + 8, 32);
  return KH_OK;
}
// the answer's keys, kinds, value offsets, values and request offsets into device buffers (P.k > 0)
static void diffs_emit(kh_trie* a, kh_trie* b, const DiffPage& P, const uint32_t* iq, uint64_t nq, uint8_t* d_keys32,
                       uint8_t* d_kinds, uint8_t* d_vals, uint64_t* d_voff, uint64_t* d_ent_off) {
  hipLaunchKernelGGL(k_diffs_write, GRID(std::max(P.k, nq) + 1, BS), dim3(BS), 0, a->c->st, side_of(a), side_of(b),
                     P.ia, P.ib, iq, P.k, P.pos, P.bytes, nq, d_keys32, d_kinds, d_voff, d_vals, d_ent_off);
  LAUNCH_CHECK();
}
static bool diffs_args_ok(kh_trie* a, const uint32_t* tries_a, kh_trie* b, const uint32_t* tries_b, uint64_t nq,
                          uint64_t max_entries, const void* keys32, const void* kinds, const void* voff,
                          const void* ent_off, const uint64_t* n_entries, const uint64_t* val_bytes,
                          const uint64_t* n_done, const uint8_t* next32) {
  if (!a || !b || !keys32 || !kinds || !voff || !ent_off || !n_entries || !val_bytes || !n_done || !next32) {
    set_err(KH_EINVAL, "null handle or outputs");
    return false;
  }
  if (nq == 0 || max_entries == 0 || nq >= (1ULL << 31) || max_entries >= (1ULL << 31) ||
      nq + max_entries >= (1ULL << 31)) {
    set_err(KH_EINVAL, "nq and max_entries must be at least 1 and nq + max_entries < 2^31");
    return false;
  }
  if ((a->forest && !tries_a) || (b->forest && !tries_b && !tries_a)) {
    set_err(KH_EINVAL, "a forest side needs a trie id per request");
    return false;
  }
  if (a->c->dev != b->c->dev) {
    set_err(KH_EINVAL, "the two handles live on different devices");
    return false;
  }
  return true;
}

extern "C" {

int kh_trie_diffs_host(kh_trie* a, const uint32_t* tries_a, kh_trie* b, const uint32_t* tries_b,
                       const uint8_t* origins32, const uint8_t* limits32, uint64_t nq, uint64_t max_entries,
                       uint64_t val_cap, uint8_t* keys32, uint8_t* kinds, uint8_t* vals, uint64_t* voff,
                       uint64_t* ent_off, uint64_t* n_entries, uint64_t* val_bytes, uint64_t* n_done,
                       uint8_t next32[32], uint8_t missing32[32]) {
  if (!diffs_args_ok(a, tries_a, b, tries_b, nq, max_entries, keys32, kinds, voff, ent_off, n_entries, val_bytes,
                     n_done, next32))
    return KH_EINVAL;
  API_TRY({
    DIFF_ENTER(a, b);
    kh_ctx* c = a->c;
    hipStream_t st = c->st;
    const bool own_b = b->forest && tries_b && tries_b != tries_a;  // (else b's ids are a's array)
    Layout Li;
    uint32_t *dta, *dtb;
    uint8_t *dor, *dli;
    Li.add(dta, nq, tries_a != nullptr && (a->forest || (b->forest && !own_b)));
    Li.add(dtb, nq, own_b);
    Li.add(dor, nq * 32, origins32 != nullptr);
    Li.add(dli, nq * 32, limits32 != nullptr);
    place(c->in_keys, Li);
    if (dta) HIPCHK(hipMemcpyAsync(dta, tries_a, nq * 4, hipMemcpyHostToDevice, st));
    if (dtb) HIPCHK(hipMemcpyAsync(dtb, tries_b, nq * 4, hipMemcpyHostToDevice, st));
    if (dor) HIPCHK(hipMemcpyAsync(dor, origins32, nq * 32, hipMemcpyHostToDevice, st));
    if (dli) HIPCHK(hipMemcpyAsync(dli, limits32, nq * 32, hipMemcpyHostToDevice, st));
    DiffPage P;
    const uint32_t* iq = nullptr;
    const int rc = diffs_scan(a, a->forest ? dta : nullptr, b, b->forest ? (own_b ? dtb : dta) : nullptr, dor, dli, nq,
                              max_entries, val_cap, P, iq, n_entries, val_bytes, n_done, next32, missing32);
    if (rc != KH_OK) return rc;
    if (P.k == 0) {
      voff[0] = 0;
      memset(ent_off, 0, (nq + 1) * 8);
      return KH_OK;
    }
    if (P.bytes && !vals) throw KhError{KH_EINVAL, "null value buffer"};
    Layout Lo;
    uint8_t *dk, *dkind, *dv;
    uint64_t *dvo, *deo;
    Lo.add(dk, P.k * 32 + 64);
    Lo.add(dvo, P.k + 1);
    Lo.add(deo, nq + 1);
    Lo.add(dkind, P.k + 64);
    Lo.add(dv, P.bytes + 64);
    place(c->out_emit, Lo);
    diffs_emit(a, b, P, iq, nq, dk, dkind, dv, dvo, deo);
    HIPCHK(hipMemcpyAsync(keys32, dk, P.k * 32, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(kinds, dkind, P.k, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(voff, dvo, (P.k + 1) * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(ent_off, deo, (nq + 1) * 8, hipMemcpyDeviceToHost, st));
    if (P.bytes) HIPCHK(hipMemcpyAsync(vals, dv, P.bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  })
}

int kh_dev_trie_diffs(kh_trie* a, const uint32_t* d_tries_a, kh_trie* b, const uint32_t* d_tries_b,
                      const uint8_t* d_origins32, const uint8_t* d_limits32, uint64_t nq, uint64_t max_entries,
                      uint64_t val_cap, uint8_t* d_keys32, uint8_t* d_kinds, uint8_t* d_vals, uint64_t* d_voff,
                      uint64_t* d_ent_off, uint64_t* n_entries, uint64_t* val_bytes, uint64_t* n_done,
                      uint8_t next32[32], uint8_t missing32[32]) {
  if (!diffs_args_ok(a, d_tries_a, b, d_tries_b, nq, max_entries, d_keys32, d_kinds, d_voff, d_ent_off, n_entries,
                     val_bytes, n_done, next32))
    return KH_EINVAL;
  if ((((uintptr_t)d_voff) | ((uintptr_t)d_ent_off)) & 7) return set_err(KH_EINVAL, "voff and ent_off must be 8-byte aligned");
  API_TRY({
    DIFF_ENTER(a, b);
    kh_ctx* c = a->c;
    DiffPage P;
    const uint32_t* iq = nullptr;
    const int rc = diffs_scan(a, a->forest ? d_tries_a : nullptr, b,
                              b->forest ? (d_tries_b ? d_tries_b : d_tries_a) : nullptr, d_origins32, d_limits32, nq,
                              max_entries, val_cap, P, iq, n_entries, val_bytes, n_done, next32, missing32);
    if (rc != KH_OK) return rc;
    if (P.k == 0) {
      HIPCHK(hipMemsetAsync(d_voff, 0, 8, c->st));
      HIPCHK(hipMemsetAsync(d_ent_off, 0, (nq + 1) * 8, c->st));
    } else {
      if (P.bytes && !d_vals) throw KhError{KH_EINVAL, "null value buffer"};
      diffs_emit(a, b, P, iq, nq, d_keys32, d_kinds, d_vals, d_voff, d_ent_off);
    }
    HIPCHK(hipStreamSynchronize(c->st));
  })
}

int kh_trie_diff_host(kh_trie* a, uint32_t trie_a, kh_trie* b, uint32_t trie_b, const uint8_t origin32[32],
                      const uint8_t limit32[32], uint64_t max_entries, uint64_t val_cap, uint8_t* keys32,
                      uint8_t* kinds, uint8_t* vals, uint64_t* voff, uint64_t* n_entries, uint64_t* val_bytes,
                      int* more, uint8_t next32[32], uint8_t missing32[32]) {
  if (!diff_args_ok(a, b, max_entries, keys32, kinds, voff, n_entries, val_bytes, more, next32)) return KH_EINVAL;
  API_TRY({
    DIFF_ENTER(a, b);
    kh_ctx* c = a->c;
    hipStream_t st = c->st;
    DiffPage P;
    const int rc = diff_scan(a, trie_a, b, trie_b, origin32, limit32, max_entries, val_cap, P, n_entries, val_bytes,
                             more, next32, missing32);
    if (rc != KH_OK) return rc;
    voff[0] = 0;
    if (P.k == 0) return KH_OK;
    if (P.bytes && !vals) throw KhError{KH_EINVAL, "null value buffer"};
    Layout Lo;
    uint8_t *dk, *dkind, *dv;
    uint64_t* dvo;
    Lo.add(dk, P.k * 32 + 64);
    Lo.add(dvo, P.k + 1);
    Lo.add(dkind, P.k + 64);
    Lo.add(dv, P.bytes + 64);
    place(c->out_emit, Lo);
    diff_emit(a, b, P, dk, dkind, dv, dvo);
    HIPCHK(hipMemcpyAsync(keys32, dk, P.k * 32, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(kinds, dkind, P.k, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(voff, dvo, (P.k + 1) * 8, hipMemcpyDeviceToHost, st));
    if (P.bytes) HIPCHK(hipMemcpyAsync(vals, dv, P.bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  })
}

int kh_dev_trie_diff(kh_trie* a, uint32_t trie_a, kh_trie* b, uint32_t trie_b, const uint8_t origin32[32],
                     const uint8_t limit32[32], uint64_t max_entries, uint64_t val_cap, uint8_t* d_keys32,
                     uint8_t* d_kinds, uint8_t* d_vals, uint64_t* d_voff, uint64_t* n_entries, uint64_t* val_bytes,
                     int* more, uint8_t next32[32], uint8_t missing32[32]) {
  if (!diff_args_ok(a, b, max_entries, d_keys32, d_kinds, d_voff, n_entries, val_bytes, more, next32)) return KH_EINVAL;
  if (((uintptr_t)d_voff) & 7) return set_err(KH_EINVAL, "voff must be 8-byte aligned");
  API_TRY({
    DIFF_ENTER(a, b);
    kh_ctx* c = a->c;
    DiffPage P;
    const int rc = diff_scan(a, trie_a, b, trie_b, origin32, limit32, max_entries, val_cap, P, n_entries, val_bytes,
                             more, next32, missing32);
    if (rc != KH_OK) return rc;
    if (P.k == 0) {
      HIPCHK(hipMemsetAsync(d_voff, 0, 8, c->st));
    } else {
      if (P.bytes && !d_vals) throw KhError{KH_EINVAL, "null value buffer"};
      diff_emit(a, b, P, d_keys32, d_kinds, d_vals, d_voff);
    }
    HIPCHK(hipStreamSynchronize(c->st));
  })
}

int kh_trie_ranges_host(kh_trie* h, const uint32_t* tries, const uint8_t* origins32, const uint8_t* limits32,
                        uint64_t nq, uint64_t max_entries, uint8_t* keys32, uint8_t* vals, uint64_t val_cap,
                        uint64_t* voff, uint64_t* ent_off, uint64_t* n_entries, uint64_t* val_bytes, uint64_t* n_done,
                        uint8_t next32[32], uint8_t missing32[32]) {
  if (!ranges_args_ok(h, tries, nq, max_entries, keys32, voff, ent_off, n_entries, val_bytes, n_done, next32))
    return KH_EINVAL;
  API_TRY({
    HANDLE_LOCK(h);
    kh_ctx* c = h->c;
    HIPCHK(hipSetDevice(c->dev));
    hipStream_t st = c->st;
    Layout Li;
    uint32_t* dt;
    uint8_t *dor, *dli;
    Li.add(dt, nq, h->forest);
    Li.add(dor, nq * 32, origins32 != nullptr);
    Li.add(dli, nq * 32, limits32 != nullptr);
    place(c->in_keys, Li);
    if (dt) HIPCHK(hipMemcpyAsync(dt, tries, nq * 4, hipMemcpyHostToDevice, st));
    if (dor) HIPCHK(hipMemcpyAsync(dor, origins32, nq * 32, hipMemcpyHostToDevice, st));
    if (dli) HIPCHK(hipMemcpyAsync(dli, limits32, nq * 32, hipMemcpyHostToDevice, st));
    RangePage P;
    const uint32_t* iq = nullptr;
    const int rc = ranges_scan(h, dt, dor, dli, nq, max_entries, val_cap, P, iq, n_entries, val_bytes, n_done, next32,
                               missing32);
    if (rc != KH_OK) return rc;
    if (P.k == 0) {
      voff[0] = 0;
      memset(ent_off, 0, (nq + 1) * 8);
      return KH_OK;
    }
    if (P.bytes && !vals) throw KhError{KH_EINVAL, "null value buffer"};
    Layout Lo;
    uint8_t *dk, *dv;
    uint64_t *dvo, *deo;
    Lo.add(dk, P.k * 32 + 64);
    Lo.add(dvo, P.k + 1);
    Lo.add(deo, nq + 1);
    Lo.add(dv, P.bytes + 64);
    place(c->out_emit, Lo);
    ranges_emit(h, P, iq, nq, dk, dv, dvo, deo);
    HIPCHK(hipMemcpyAsync(keys32, dk, P.k * 32, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(voff, dvo, (P.k + 1) * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(ent_off, deo, (nq + 1) * 8, hipMemcpyDeviceToHost, st));
    if (P.bytes) HIPCHK(hipMemcpyAsync(vals, dv, P.bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  })
}

int kh_dev_trie_ranges(kh_trie* h, const uint32_t* d_tries, const uint8_t* d_origins32, const uint8_t* d_limits32,
                       uint64_t nq, uint64_t max_entries, uint8_t* d_keys32, uint8_t* d_vals, uint64_t val_cap,
                       uint64_t* d_voff, uint64_t* d_ent_off, uint64_t* n_entries, uint64_t* val_bytes,
                       uint64_t* n_done, uint8_t next32[32], uint8_t missing32[32]) {
  if (!ranges_args_ok(h, d_tries, nq, max_entries, d_keys32, d_voff, d_ent_off, n_entries, val_bytes, n_done, next32))
    return KH_EINVAL;
  if ((((uintptr_t)d_voff) | ((uintptr_t)d_ent_off)) & 7) return set_err(KH_EINVAL, "voff and ent_off must be 8-byte aligned");
  API_TRY({
    HANDLE_LOCK(h);
    kh_ctx* c = h->c;
    HIPCHK(hipSetDevice(c->dev));
    RangePage P;
    const uint32_t* iq = nullptr;
    const int rc = ranges_scan(h, h->forest ? d_tries : nullptr, d_origins32, d_limits32, nq, max_entries, val_cap, P,
                               iq, n_entries, val_bytes, n_done, next32, missing32);
    if (rc != KH_OK) return rc;
    if (P.k == 0) {
      HIPCHK(hipMemsetAsync(d_voff, 0, 8, c->st));
      HIPCHK(hipMemsetAsync(d_ent_off, 0, (nq + 1) * 8, c->st));
    } else {
      if (P.bytes && !d_vals) throw KhError{KH_EINVAL, "null value buffer"};
      ranges_emit(h, P, iq, nq, d_keys32, d_vals, d_voff, d_ent_off);
    }
    HIPCHK(hipStreamSynchronize(c->st));
  })
}

int kh_trie_range_host(kh_trie* h, uint32_t trie, const uint8_t origin32[32], const uint8_t limit32[32],
                       uint64_t max_entries, uint8_t* keys32, uint8_t* vals, uint64_t val_cap, uint64_t* voff,
                       uint64_t* n_entries, uint64_t* val_bytes, int* more, uint8_t next32[32], uint8_t missing32[32]) {
  if (!range_args_ok(h, max_entries, keys32, voff, n_entries, val_bytes, more, next32)) return KH_EINVAL;
  API_TRY({
    HANDLE_LOCK(h);
    kh_ctx* c = h->c;
    HIPCHK(hipSetDevice(c->dev));
    hipStream_t st = c->st;
    RangePage P;
    const int rc = range_scan(h, trie, origin32, limit32, max_entries, val_cap, P, n_entries, val_bytes, more, next32,
                              missing32);
    if (rc != KH_OK) return rc;
    voff[0] = 0;
    if (P.k == 0) return KH_OK;
    if (P.bytes && !vals) throw KhError{KH_EINVAL, "null value buffer"};
    Layout Lo;
    uint8_t *dk, *dv;
    uint64_t* dvo;
    Lo.add(dk, P.k * 32 + 64);
    Lo.add(dvo, P.k + 1);
    Lo.add(dv, P.bytes + 64);
    place(c->out_emit, Lo);
    range_emit(h, P, dk, dv, dvo);
    HIPCHK(hipMemcpyAsync(keys32, dk, P.k * 32, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(voff, dvo, (P.k + 1) * 8, hipMemcpyDeviceToHost, st));
    if (P.bytes) HIPCHK(hipMemcpyAsync(vals, dv, P.bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  })
}

int kh_dev_trie_range(kh_trie* h, uint32_t trie, const uint8_t origin32[32], const uint8_t limit32[32],
                      uint64_t max_entries, uint8_t* d_keys32, uint8_t* d_vals, uint64_t val_cap, uint64_t* d_voff,
                      uint64_t* n_entries, uint64_t* val_bytes, int* more, uint8_t next32[32], uint8_t missing32[32]) {
  if (!range_args_ok(h, max_entries, d_keys32, d_voff, n_entries, val_bytes, more, next32)) return KH_EINVAL;
  API_TRY({
    HANDLE_LOCK(h);
    kh_ctx* c = h->c;
    HIPCHK(hipSetDevice(c->dev));
    RangePage P;
    const int rc = range_scan(h, trie, origin32, limit32, max_entries, val_cap, P, n_entries, val_bytes, more, next32,
                              missing32);
    if (rc != KH_OK) return rc;
    if (P.k == 0) {
      HIPCHK(hipMemsetAsync(d_voff, 0, 8, c->st));
    } else {
      if (P.bytes && !d_vals) throw KhError{KH_EINVAL, "null value buffer"};
      range_emit(h, P, d_keys32, d_vals, d_voff);
    }
    HIPCHK(hipStreamSynchronize(c->st));
  })
}

}  // extern "C"
