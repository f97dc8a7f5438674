// Range scan: the entries of a resident trie in key order (kh_trie_range_host, kh_dev_trie_range),
// read from the records alone.  Every node is a record found by its anchor (forest.h) and a
// branch's record carries its child mask, so the entries at and after a key are reached by
// walking down from the root, a level a round, keeping an ORDERED FRONTIER of record indices:
//
//   round 0   the root record of the trie, map_find(M, R, t, 0, any key)
//   a round   every item of the frontier is SELECTED against [origin, limit]:
//               a leaf or a value-only branch stays iff origin <= key <= limit;
//               a stub (a subtree a partial handle lacks) stays iff its prefix meets the range;
//               a branch whose db-nibble prefix lies outside the range's prefixes goes (with its
//               extension); else it is replaced by its children c, in nibble order, whose
//               (db + 1)-nibble prefix P.c lies within [prefix(origin), prefix(limit)]
//             count (a popcount of the restricted mask: no probe), exclusive scan, fill (child c
//             lands at the item's base plus the selected children below c; only a child placed
//             before the cut is probed)
//   the cut   the new frontier is the first max_entries + 2 items: subtrees are disjoint, at most
//             one item lies on origin's path and may turn out empty, the item on limit's path is
//             the last in order, and every other item holds an entry in range -- so the first
//             max_entries + 1 entries lie under the first max_entries + 2 items
//   the end   a round in which no item was a branch leaves the answer: entries and stubs in
//             range, in key order (at most 64 branch depths and the closing round)
//
// MANY RANGES A CALL (kh_trie_ranges_host, kh_dev_trie_ranges): nq requests (trie, origin, limit)
// answered in request order under one entry and byte budget.  The frontier is SEGMENTED: an item
// is (record, request), ordered by (request, key).  Round 0 holds the root record of every request
// (NONE for an empty one), request q at place q; a round selects every item against ITS OWN
// request's KeyRange (an nq-long array), and the fill writes the item's request beside each child
// it places, so a segment's children stay together, in key order, between those of the requests
// either side: the order holds by construction, with no atomic claiming a slot.  All requests move
// through the rounds together, so a call takes the rounds of its deepest request.
//   the cut   the new frontier is the first max_entries + 2 * nq items.  Subtrees are disjoint and
//             ordered.  Per request at most one item lies on origin's path and at most one on
//             limit's, either may turn out empty, and limit's is the last of its segment; every
//             other item holds an entry (or a stub: one thing).  Let X be the item that holds thing
//             max_entries + 1 of the concatenated answer, in request x.  The empty items before X
//             are at most two for each of the x <= nq - 1 requests before x and the origin item of
//             x (its limit item is X or lies after X): 2 * nq - 1.  The items up to X that hold a
//             thing are at most max_entries + 1.  So X is among the first max_entries + 2 * nq
//             items, and what lies past them is never needed.  One item fewer can lose X: the cut
//             in the last request, both boundary items of every request empty, every other item
//             one entry (tests/test_ranges_host.py builds that input).
//   the end   a round in which no item of any request was a branch: at most 64 branch depths and
//             the closing round, whatever nq is.  Then the first max_entries + 1 things, the
//             lowest stub, the fit to val_cap and the write are the single call's; ent_off[q] is
//             the lower bound of q in the returned items' (non-decreasing) requests, and the cut
//             request is that of thing k, the first not returned.
//
// KH_HD bodies only, shared by range_kernels.hip (16 lanes an item, lane c owning child c, as
// export.h) and the host replays of tests/range_host and tests/ranges_host.
#pragma once
#include "export.h"

namespace khst {

struct KeyRange {
  uint64_t o[4], l[4];  // origin and limit (keys: 4 little-endian words)
};
constexpr uint32_t RNG_SELF = 0x10000u;  // selection: the item itself stays (the low 16 bits: its children)

// the first d nibbles of a against those of b, big-endian
KH_HD int prefix_cmp(const uint64_t* a, const uint64_t* b, uint32_t d) {
  for (int q = 0; q < 4; ++q) {
    const uint64_t x = bswap64(prefix_word(a, d, q)), y = bswap64(prefix_word(b, d, q));
    if (x != y) return x < y ? -1 : 1;
  }
  return 0;
}
KH_HD uint32_t rng_nibble(const uint64_t* key, uint32_t i) {
  const uint8_t b = ((const uint8_t*)key)[i >> 1];
  return (i & 1) ? (b & 0xFu) : (uint32_t)(b >> 4);
}

// the selection of frontier item r: 0 (it goes), RNG_SELF (it stays and is final), or the child
// nibbles of a branch that take its place (possibly none: 0 as well)
KH_HD uint32_t rng_select(const Recs& R, uint32_t r, const KeyRange& g) {
  if (r == NONE) return 0u;  // (a child a corrupt map lacked: the fill flagged it)
  const uint64_t* k = R.key(r);
  const uint32_t db = R.rdb[r];
  if (db == EL_LEAF || db == VB_DEPTH) return (key_cmp(g.o, k) <= 0 && key_cmp(k, g.l) <= 0) ? RNG_SELF : 0u;
  const uint32_t dp = exp_db(R, r);  // (a stub: the depth at which the missing node starts)
  const int co = prefix_cmp(k, g.o, dp), cl = prefix_cmp(k, g.l, dp);
  if (co < 0 || cl > 0) return 0u;
  if (db == EL_STUB) return RNG_SELF;
  const uint32_t lo = co == 0 ? rng_nibble(g.o, db) : 0u, hi = cl == 0 ? rng_nibble(g.l, db) : 15u;
  if (lo > hi) return 0u;
  return (uint32_t)R.rmask[r] & (0xFFFFu >> (15u - hi)) & (0xFFFFu << lo) & 0xFFFFu;
}
KH_HD uint32_t rng_count(uint32_t sel) { return kh_popc(sel & 0xFFFFu) + (sel >> 16); }

// lane c of item r (selection sel, scanned base): the item itself (lane 0) or child c goes to its
// place in the next frontier when that place lies before the cut; false: the anchor map lacks a
// child the mask names (a corrupt map).  outq (a segmented frontier): the item's request q is
// written beside what is placed.
KH_HD bool rng_fill_lane(const Recs& R, const AMap& M, uint32_t r, uint32_t sel, uint32_t c, uint64_t base,
                         uint64_t cut, uint32_t* out, uint32_t* outq = nullptr, uint32_t q = 0) {
  if (sel & RNG_SELF) {
    if (c == 0 && base < cut) {
      out[base] = r;
      if (outq) outq[base] = q;
    }
    return true;
  }
  if (!((sel >> c) & 1)) return true;
  const uint64_t at = base + kh_popc(sel & ((1u << c) - 1u));
  if (at >= cut) return true;
  const uint32_t child = exp_child(R, M, r, c);
  out[at] = child;
  if (outq) outq[at] = q;
  return child != NONE;
}

// ---- many ranges a call
// request q's range from the packed origins and limits (either NULL: all zero / all 0xFF; byte
// reads, so the arrays need no alignment); false: origin > limit, an empty request
KH_HD bool rng_request(const uint8_t* origins32, const uint8_t* limits32, uint64_t q, KeyRange* g) {
  uint8_t *o = (uint8_t*)g->o, *l = (uint8_t*)g->l;
  for (int b = 0; b < 32; ++b) {
    o[b] = origins32 ? origins32[32 * q + b] : (uint8_t)0;
    l[b] = limits32 ? limits32[32 * q + b] : (uint8_t)0xFF;
  }
  return key_cmp(g->o, g->l) <= 0;
}
// the first of the n returned items whose request is q or later (iq does not decrease): where
// request q's entries start
KH_HD uint64_t rng_ent_off(const uint32_t* iq, uint64_t n, uint64_t q) {
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (iq[mid] < q)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// ---- after the last round: the frontier's items are entries (leaves, value-only branches) or stubs
KH_HD bool rng_is_stub(const Recs& R, uint32_t r) { return r != NONE && R.rdb[r] == EL_STUB; }
// The largest prefix of entries whose values fit val_cap, from the exclusive 64-bit scan pos of
// the n value lengths (monotone; total its sum): candidate i in [0, n] writes fit[0] = i and
// fit[1] = the bytes of entries [0, i) iff it is that prefix.
KH_HD void rng_fit(const uint64_t* pos, uint64_t n, uint64_t total, uint64_t val_cap, uint64_t i,
                   unsigned long long* fit) {
  const uint64_t b0 = i < n ? pos[i] : total;
  if (b0 > val_cap) return;
  if (i < n && (i + 1 < n ? pos[i + 1] : total) <= val_cap) return;  // entry i fits as well
  fit[0] = i;
  fit[1] = b0;
}
// entry i of the answer: its key, its offset, its value
KH_HD void rng_write(const Recs& R, const uint8_t* heap, uint32_t r, uint64_t i, uint64_t at, uint8_t* keys32,
                     uint64_t* voff, uint8_t* vals) {
  const uint8_t* k = (const uint8_t*)R.key(r);
  for (int b = 0; b < 32; ++b) keys32[32 * i + b] = k[b];
  voff[i] = at;
  const uint8_t* src = heap + R.rvo[r];
  for (uint32_t b = 0, L = R.rvl[r]; b < L; ++b) vals[at + b] = src[b];
}

}  // namespace khst
