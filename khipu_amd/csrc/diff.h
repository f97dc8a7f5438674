// Trie diff: the keys whose entries differ between two resident tries, in key order
// (kh_trie_diff_host, kh_dev_trie_diff), read from the two sides' records alone.  The walk is the
// ordered frontier of range.h run over two tries in lockstep: every record caches the reference
// its parent sees (rref) and a branch's own (rbref), so two subtrees that start at the same nibble
// path with the same reference are identical and are never entered.
//
//   an item   (ra, rb, D): a record of side a, one of side b (either may be NONE) and the depth at
//             which the item stands; both sides cover the same D-nibble prefix.  A record may stand
//             below its own anchor (D > rd): the other side branched inside its extension.
//   round 0   the two root records; nothing at all when the pair is skipped (equal roots)
//   a round   every item is SELECTED.  With m the smaller of the sides' branch depths (a leaf or a
//             value-only branch: 64; a stub: the depth at which the missing node starts):
//               the key prefixes differ before m: the subtrees are disjoint, the item SPLITS into
//                 its two one-sided items in key order (each kept iff range.h would keep it);
//               both sides are entries at one key: the item stays and is final (kind 3);
//               a side is a stub at m: the item stays and is final (a missing thing);
//               else lane c of the item's 16 forms the child pair at nibble c -- a side that
//                 branches at m gives its child c (a probe), a side whose branch lies deeper acts
//                 as a node with the single child nibble of its key at m and is carried down
//                 unchanged -- for the nibbles c inside [origin, limit] (rng_select's interval),
//                 and the pair SURVIVES unless it is skipped;
//               a one-sided item is selected as range.h selects it (no probe, no skip).
//             count (the surviving lanes), exclusive scan, fill (only what lands before the cut is
//             probed again and written)
//   the skip  a pair (ra, rb, D) is skipped iff both sides have a node that starts at the same
//             path with the same reference:
//               both anchors equal D and rref with its length is equal (the upper nodes);
//               both branch depths are equal non-leaf depths, the prefixes agree to it, and rbref
//                 with its length is equal (the lower nodes: equal branches under different
//                 extensions, or a record carried down beside the other side's child);
//               both are entries with equal keys, equal value bytes and equal value-only-branch
//                 status (a leaf carried down beside a leaf).
//             A stub enters these tests with what it keeps: its extension starts at its anchor
//             with rref, the missing node at the depth in rmask's low byte with rbref.
//   the cut   the skip test is made BEFORE the cut, so every item of the next frontier is an
//             unskipped pair or a one-sided item.  The store is canonical: the shape of a subtree
//             is a function of its keys, its references of its keys and values -- with one
//             exception, khipu's value-only branch, which holds the keys of a leaf in another node,
//             and that is why a leaf against a value-only branch of equal value is a difference.
//             So two subtrees at one prefix whose content (keys, values, value-only-branch status)
//             is equal have the same first branch depth and the same branch reference there, or are
//             the same entry: they are skipped by the second or the third test.  An unskipped pair
//             therefore holds a difference, a one-sided item holds a key, and only the range can
//             empty an item: at most one on origin's path and one on limit's (the last in order).
//             The first max_entries + 2 items hold the first max_entries + 1 things.
//   the end   a round in which no item expanded or split: at most 64 branch depths, one split
//             round on a path and the closing round.  The items are then one-sided entries (kinds
//             1 and 2), pairs of entries at one key (kind 3) and items with a stub (missing).
//
// MANY PAIRS A CALL (kh_trie_diffs_host, kh_dev_trie_diffs): nq requests (trie of a, trie of b,
// origin, limit) answered in request order under one entry and byte budget -- range.h's segmented
// frontier run over two tries.  An item is (ra, rb, D, q), ordered by (request, key).  Round 0 has
// one thread a request: its KeyRange into an nq-long array, its root pair at place q, (NONE, NONE)
// when the request is empty or its root pair is skipped (df_plan drops that item: no compaction).
// A round is the round above with every item selected against ITS OWN request's range, and the fill
// writes the item's request beside each item it places (both halves of a split): a request's items
// stay between its neighbours', so the order holds by construction and no slot is claimed with an
// atomic.  All requests move together: a call takes the rounds of its deepest request.
//   the cut   the new frontier is the first max_entries + 2 * nq items.  Per request at most the
//             item on origin's path and the item on limit's path can turn out empty, and limit's is
//             the last of its segment; every other item holds a thing (the argument above, per
//             segment).  Let X be the item that holds thing max_entries + 1 of the concatenated
//             answer, in request x.  The empty items before X are at most two for each of the
//             x <= nq - 1 requests before x and the origin item of x: 2 * nq - 1.  The items up to X
//             that hold a thing are at most max_entries + 1.  So X is among the first
//             max_entries + 2 * nq items, and one item fewer can lose it (tests/test_diffs_host.py
//             builds that input).
//   the end   a round in which no item of any request expanded or split.  Then the first
//             max_entries + 1 things, the lowest stub, the fit to val_cap and the write are the
//             single call's; ent_off[q] is rng_ent_off over the returned items' requests, and the
//             cut request is that of thing k, the first not returned.
//
// KH_HD bodies only, shared by range_kernels.hip (16 lanes an item, lane c owning child c) and the
// host replays of tests/diff_host and tests/diffs_host.
#pragma once
#include "range.h"

namespace khst {

constexpr uint32_t DF_SELF = RNG_SELF;                          // the item stays and is final
constexpr uint32_t DF_SPLIT_A = 0x20000u, DF_SPLIT_B = 0x40000u;  // a split: the one-sided item of a / of b is kept
constexpr uint32_t DF_ONLY_A = 1, DF_ONLY_B = 2, DF_CHANGED = 3;  // (KH_DIFF_*)

// one side of the walk: a handle's records, anchor map and value heap
struct DSide {
  Recs R;
  AMap M;
  const uint8_t* heap;
};

KH_HD bool df_entry(const Recs& R, uint32_t r) {
  const uint32_t db = R.rdb[r];
  return db == EL_LEAF || db == VB_DEPTH;
}
KH_HD bool df_stub(const Recs& R, uint32_t r) { return R.rdb[r] == EL_STUB; }
// the depth at which the side acts: its branch's, 64 for an entry, the missing node's for a stub
KH_HD uint32_t df_db(const Recs& R, uint32_t r) { return df_entry(R, r) ? 64u : exp_db(R, r); }
// two capped references (32 bytes of record each, the first al / bl of them used)
KH_HD bool df_ref_eq(const uint64_t* a, uint32_t al, const uint64_t* b, uint32_t bl) {
  if (al != bl) return false;
  if (al == 32) return a[0] == b[0] && a[1] == b[1] && a[2] == b[2] && a[3] == b[3];
  const uint8_t *x = (const uint8_t*)a, *y = (const uint8_t*)b;
  for (uint32_t i = 0; i < al; ++i)
    if (x[i] != y[i]) return false;
  return true;
}

// "the skip": both sides of the pair (ra, rb, D) have a node that starts at the same path with the
// same reference
KH_HD bool df_skip(const DSide& A, uint32_t ra, const DSide& B, uint32_t rb, uint32_t D) {
  if (ra == NONE || rb == NONE) return false;
  const Recs &Ra = A.R, &Rb = B.R;
  if (Ra.rd[ra] == D && Rb.rd[rb] == D &&
      df_ref_eq(&Ra.rref[4ull * ra], Ra.rrl[ra], &Rb.rref[4ull * rb], Rb.rrl[rb]))
    return true;
  const bool ea = df_entry(Ra, ra), eb = df_entry(Rb, rb);
  if (ea != eb) return false;
  const uint64_t *ka = Ra.key(ra), *kb = Rb.key(rb);
  if (ea) {
    if (ka[0] != kb[0] || ka[1] != kb[1] || ka[2] != kb[2] || ka[3] != kb[3]) return false;
    if (Ra.rdb[ra] != Rb.rdb[rb] || Ra.rvl[ra] != Rb.rvl[rb]) return false;
    const uint8_t *va = A.heap + Ra.rvo[ra], *vb = B.heap + Rb.rvo[rb];
    for (uint32_t i = 0, L = Ra.rvl[ra]; i < L; ++i)
      if (va[i] != vb[i]) return false;
    return true;
  }
  const uint32_t da = exp_db(Ra, ra);
  return da == exp_db(Rb, rb) && prefix_eq(ka, kb, da) &&
         df_ref_eq(&Ra.rbref[4ull * ra], Ra.rbrl[ra], &Rb.rbref[4ull * rb], Rb.rbrl[rb]);
}

// the depth at which item (ra, rb) acts (not both NONE)
KH_HD uint32_t df_m(const DSide& A, uint32_t ra, const DSide& B, uint32_t rb) {
  if (rb == NONE) return df_db(A.R, ra);
  if (ra == NONE) return df_db(B.R, rb);
  const uint32_t da = df_db(A.R, ra), dbb = df_db(B.R, rb);
  return da < dbb ? da : dbb;
}
// the child nibbles of one side at depth m: its branch's mask, or the nibble its key takes there
KH_HD uint32_t df_side_mask(const Recs& R, uint32_t r, uint32_t m) {
  return df_db(R, r) == m ? (uint32_t)R.rmask[r] : 1u << rng_nibble(R.key(r), m);
}

// The plan of item (ra, rb): 0 (it goes), DF_SELF, DF_SPLIT_* bits, or the child nibbles inside
// the range at which a pair is formed (the pairs' skip tests are the lanes': df_lane_alive).
KH_HD uint32_t df_plan(const DSide& A, uint32_t ra, const DSide& B, uint32_t rb, const KeyRange& g) {
  if (ra == NONE && rb == NONE) return 0u;
  if (rb == NONE) return rng_select(A.R, ra, g);
  if (ra == NONE) return rng_select(B.R, rb, g);
  const uint32_t m = df_m(A, ra, B, rb);
  const uint64_t *ka = A.R.key(ra), *kb = B.R.key(rb);
  if (!prefix_eq(ka, kb, m))
    return (rng_select(A.R, ra, g) ? DF_SPLIT_A : 0u) | (rng_select(B.R, rb, g) ? DF_SPLIT_B : 0u);
  const int co = prefix_cmp(ka, g.o, m), cl = prefix_cmp(ka, g.l, m);
  if (co < 0 || cl > 0) return 0u;
  if ((df_stub(A.R, ra) && exp_db(A.R, ra) == m) || (df_stub(B.R, rb) && exp_db(B.R, rb) == m)) return DF_SELF;
  if (m == 64) return DF_SELF;  // both are entries at one key (an equal pair was skipped when it was formed)
  const uint32_t lo = co == 0 ? rng_nibble(g.o, m) : 0u, hi = cl == 0 ? rng_nibble(g.l, m) : 15u;
  if (lo > hi) return 0u;
  return (df_side_mask(A.R, ra, m) | df_side_mask(B.R, rb, m)) & (0xFFFFu >> (15u - hi)) & (0xFFFFu << lo) & 0xFFFFu;
}
// lane c: the child pair of item (ra, rb) at nibble c of depth m (plan bit c is set)
KH_HD uint32_t df_side_child(const DSide& S, uint32_t r, uint32_t m, uint32_t c) {
  if (r == NONE) return NONE;
  if (df_db(S.R, r) == m) return exp_child(S.R, S.M, r, c);
  return rng_nibble(S.R.key(r), m) == c ? r : NONE;
}
// lane c of the select: does the lane place something in the next frontier?  (A one-sided item's
// children are not probed: its mask names them.)
KH_HD bool df_lane_alive(const DSide& A, uint32_t ra, const DSide& B, uint32_t rb, uint32_t plan, uint32_t c) {
  if (!((plan >> c) & 1)) return false;
  if (ra == NONE || rb == NONE) return true;
  const uint32_t m = df_m(A, ra, B, rb);
  return !df_skip(A, df_side_child(A, ra, m, c), B, df_side_child(B, rb, m, c), m + 1);
}
KH_HD uint32_t df_count(uint32_t sel) { return kh_popc(sel & 0x7FFFFu); }
KH_HD bool df_expands(uint32_t sel) { return (sel & (0xFFFFu | DF_SPLIT_A | DF_SPLIT_B)) != 0; }

// lane c of item (ra, rb, D) with selection sel (the plan with the skipped lanes cleared) and scanned
// base: what the lane owns goes to its place in the next frontier when that lies before the cut;
// false: the anchor map lacks a child a mask names (a corrupt map).  oq (a segmented frontier): the
// item's request q is written beside what is placed, both halves of a split included.
KH_HD bool df_fill_lane(const DSide& A, uint32_t ra, const DSide& B, uint32_t rb, uint32_t D, uint32_t sel,
                        uint32_t c, uint64_t base, uint64_t cut, uint32_t* oa, uint32_t* ob, uint32_t* od,
                        uint32_t* oq = nullptr, uint32_t q = 0) {
  if (sel & DF_SELF) {
    if (c == 0 && base < cut) {
      oa[base] = ra;
      ob[base] = rb;
      od[base] = D;
      if (oq) oq[base] = q;
    }
    return true;
  }
  if (sel & (DF_SPLIT_A | DF_SPLIT_B)) {
    if (c != 0) return true;
    const bool a_first = key_cmp(A.R.key(ra), B.R.key(rb)) < 0;
    uint64_t at = base;
    for (int s = 0; s < 2; ++s) {
      const bool a_now = (s == 0) == a_first;
      if (!(sel & (a_now ? DF_SPLIT_A : DF_SPLIT_B))) continue;
      if (at < cut) {
        oa[at] = a_now ? ra : NONE;
        ob[at] = a_now ? NONE : rb;
        od[at] = D;
        if (oq) oq[at] = q;
      }
      ++at;
    }
    return true;
  }
  if (!((sel >> c) & 1)) return true;
  const uint64_t at = base + kh_popc(sel & ((1u << c) - 1u));
  if (at >= cut) return true;
  const uint32_t m = df_m(A, ra, B, rb);
  const uint32_t ca = df_side_child(A, ra, m, c), cb = df_side_child(B, rb, m, c);
  oa[at] = ca;
  ob[at] = cb;
  od[at] = m + 1;
  if (oq) oq[at] = q;
  return ca != NONE || cb != NONE;
}

// ---- many pairs a call: round 0 of request q.  Its KeyRange goes to G[q] and its root pair to place
// q: (NONE, NONE), which df_plan drops, for an empty request (origin > limit, the same (handle, id)
// on both sides, no root on either side) and for a root pair that is skipped (equal tries).  ta / tb:
// the requests' trie ids (NULL: a single trie, id 0); has_a / has_b: the side has records at all;
// same: both sides are one handle.  true: the request has something to walk.
KH_HD bool df_request(const DSide& A, const uint32_t* ta, bool has_a, const DSide& B, const uint32_t* tb, bool has_b,
                      bool same, const uint8_t* origins32, const uint8_t* limits32, uint64_t q, KeyRange* G,
                      uint32_t* ia, uint32_t* ib, uint32_t* id, uint32_t* iq) {
  KeyRange g;
  const bool ok = rng_request(origins32, limits32, q, &g);
  G[q] = g;
  const uint32_t ida = ta ? ta[q] : 0u, idb = tb ? tb[q] : 0u;
  uint32_t ra = NONE, rb = NONE;
  if (ok && !(same && ida == idb)) {
    const uint64_t zero[4] = {0, 0, 0, 0};
    if (has_a) ra = map_find(A.M, A.R, ida, 0, zero);
    if (has_b) rb = map_find(B.M, B.R, idb, 0, zero);
    if (df_skip(A, ra, B, rb, 0)) ra = rb = NONE;
  }
  ia[q] = ra;
  ib[q] = rb;
  id[q] = 0;
  iq[q] = (uint32_t)q;
  return ra != NONE || rb != NONE;
}

// ---- after the last round: an item is a difference or holds a stub
KH_HD bool df_missing(const DSide& A, uint32_t ra, const DSide& B, uint32_t rb) {
  return (ra != NONE && df_stub(A.R, ra)) || (rb != NONE && df_stub(B.R, rb));
}
KH_HD uint32_t df_kind(uint32_t ra, uint32_t rb) { return rb == NONE ? DF_ONLY_A : ra == NONE ? DF_ONLY_B : DF_CHANGED; }
// the bytes of side b's value the item returns
KH_HD uint64_t df_len(const DSide& A, uint32_t ra, const DSide& B, uint32_t rb) {
  return (rb == NONE || df_missing(A, ra, B, rb)) ? 0 : B.R.rvl[rb];
}
KH_HD const uint64_t* df_key(const DSide& A, uint32_t ra, const DSide& B, uint32_t rb) {
  return ra != NONE ? A.R.key(ra) : B.R.key(rb);
}
// difference i of the answer: its key, its kind, its offset, side b's value
KH_HD void df_write(const DSide& A, uint32_t ra, const DSide& B, uint32_t rb, uint64_t i, uint64_t at,
                    uint8_t* keys32, uint8_t* kinds, uint64_t* voff, uint8_t* vals) {
  const uint8_t* k = (const uint8_t*)df_key(A, ra, B, rb);
  for (int b = 0; b < 32; ++b) keys32[32 * i + b] = k[b];
  kinds[i] = (uint8_t)df_kind(ra, rb);
  voff[i] = at;
  if (rb == NONE) return;
  const uint8_t* src = B.heap + B.R.rvo[rb];
  for (uint32_t b = 0, L = B.R.rvl[rb]; b < L; ++b) vals[at + b] = src[b];
}

}  // namespace khst
