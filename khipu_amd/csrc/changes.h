// Changes since a savepoint: the keys whose entries differ between the version at an open savepoint
// (S) and the current version (C) of ONE handle (kh_trie_changes_since_host,
// kh_dev_trie_changes_since), read from the undo journal and the appended records alone -- no copy
// of the handle, and work that follows the journal, not the trie.
//
//   what the journal holds   With a savepoint open, a commit saves every record it rewrites in place
//             before the first change (k_rec_save, Commit::journal_begin): the TOUCHED records (the
//             leaves its ops end at: k_map_delete marks them dead; one that no op replaced or
//             deleted is written again, live, by k_f_elem_recs) and the element sources that move
//             (a subtree or leaf re-anchored because a sibling went or came: k_f_elem_recs rewrites
//             it at its index with the same key and value span).  Every other record is left as it
//             is, and everything new -- an upsert's leaf, the new branches, a forest load's records
//             -- is appended past the savepoint's rn.  A leaf record never changes its key, and a
//             dead record is never written again (it is in no map, so no descent reaches it).
//   so        a key whose entry differs between S and C had its S record saved (it was touched), or
//             has no S record; and its C record is that same index rewritten, or an appended one.
//   candidates   OLD: the saved copy at journal position p in [j0, j0 + jn) when jidx[p] is a
//             record below the savepoint's rn and the copy is a live entry (a leaf or a value-only
//             branch).  A record saved more than once has its savepoint version in its EARLIEST
//             copy; the later copies carry the same key, so they fall into the same run below and
//             the lowest position is taken.  NEW: the current record at the index of each OLD
//             candidate when it is a live entry, and every live entry among the appended records
//             [rn0, rn0 + an).  Nothing is inferred from dead / live alone: both sides are put up
//             and the join decides, which is what makes a re-anchored leaf, a leaf touched and
//             kept, and a key deleted and put back with its bytes vanish.
//   a slot    candidate number s of the 2 jn + an possible ones: s < jn the OLD of position
//             j0 + s; s < 2 jn the NEW of position j0 + s - jn; else appended record
//             rn0 + s - 2 jn.  Slot order is (side, journal position).
//   order     the kept slots sorted by (trie id, key, slot): stable LSD radix passes over 64-bit
//             words (chg_sort_word), first on the key's leading 8 bytes and the trie id alone; two
//             neighbours equal in those and different in the key (dense keys; never hashes) raise
//             a flag and the call sorts again on all four words.
//   join      the run of equal (trie, key) starting at a head: its lowest OLD slot and its lowest
//             NEW slot (the NEW slots of one record are copies of each other).  OLD only: the key
//             left (kind 1 on the way S -> C); NEW only: it came (kind 2); both: equal
//             value-only-branch status, length and bytes drop the run, anything else is kind 3.
//   page      the differences at or after the resume point (trie, key) are counted (n_total) and
//             the first max_entries + 1 of them become items (record of a, record of b) of diff.h
//             over two record arrays -- the journal's copies and the handle's records, one heap --
//             so lengths, fit, write and the kinds are the trie diff's own (df_len, rng_fit,
//             df_write).  KH_CHANGES_REVERSE swaps the two sides.
//
// KH_HD bodies only, shared by range_kernels.hip and the host replay of tests/changes_host.
#pragma once
#include "diff.h"

namespace khst {

struct ChgSrc {
  Recs J;                // the journal's saved copies as records: index = journal position
  const uint32_t* jidx;  // [journal position] the record a copy was taken from (NONE: none)
  Recs R;                // the handle's records now
  const uint8_t* heap;   // the one value heap both read (append-only while a savepoint is open)
  uint64_t j0, jn;       // journal positions [j0, j0 + jn): saved since the savepoint
  uint64_t rn0, an;      // records [rn0, rn0 + an): appended since the savepoint
};
constexpr uint32_t CHG_WORD_TRIE = 4;  // chg_sort_word: the trie id (0..3: the key's words)

KH_HD uint64_t chg_slots(const ChgSrc& S) { return 2 * S.jn + S.an; }
KH_HD bool chg_old(const ChgSrc& S, uint64_t s) { return s < S.jn; }
// the record a KEPT slot stands for: a journal position in S.J (OLD), an index in S.R (NEW)
KH_HD const Recs& chg_recs(const ChgSrc& S, uint64_t s) { return s < S.jn ? S.J : S.R; }
KH_HD uint32_t chg_rec(const ChgSrc& S, uint64_t s) {
  if (s < S.jn) return (uint32_t)(S.j0 + s);
  if (s < 2 * S.jn) return S.jidx[S.j0 + s - S.jn];
  return (uint32_t)(S.rn0 + (s - 2 * S.jn));
}

// ---- collect.  A live entry, from the 16-byte word at byte 32 of a record (rec_store's w[4], w[5]:
// t | d << 32 | db << 40 | mask << 48, then live | rl << 8 | brl << 16 | vl << 32) ...
KH_HD bool chg_entry_words(uint64_t w4, uint64_t w5) {
  const uint32_t db = (uint32_t)(w4 >> 40) & 0xFFu;
  return (uint8_t)w5 == REC_LIVE && (db == EL_LEAF || db == VB_DEPTH);
}
// ... and from the record itself
KH_HD bool chg_live_entry(const Recs& R, uint32_t r) { return R.rlive[r] == REC_LIVE && df_entry(R, r); }
// journal position p: is its copy an OLD candidate (idx = jidx[p], copy_entry: the copy is a live
// entry), and with it the current record at idx a NEW one (cur_entry)?
KH_HD bool chg_keep_old(uint32_t idx, uint64_t rn0, bool copy_entry) { return idx != NONE && idx < rn0 && copy_entry; }
KH_HD bool chg_keep_new(uint32_t idx, uint64_t rn0, bool copy_entry, bool cur_entry) {
  return chg_keep_old(idx, rn0, copy_entry) && cur_entry;
}

// ---- order: word w of a kept slot's sort key (big-endian key words, so integer order is key order)
KH_HD uint64_t chg_sort_word(const ChgSrc& S, uint64_t s, uint32_t w) {
  const Recs& R = chg_recs(S, s);
  const uint32_t r = chg_rec(S, s);
  return w == CHG_WORD_TRIE ? (uint64_t)R.rt[r] : bswap64(R.rk[4ull * r + w]);
}

// ---- join.  Is sorted place j the head of its run of equal (trie, key)?  *tie is set when j and
// its left neighbour agree in the trie and the key's first word and differ in the key: the order
// within such a stretch is not the key order unless all four words were sorted.
KH_HD bool chg_head(const ChgSrc& S, const uint32_t* sv, uint64_t j, bool* tie) {
  *tie = false;
  if (j == 0) return true;
  const Recs &Ra = chg_recs(S, sv[j - 1]), &Rb = chg_recs(S, sv[j]);
  const uint32_t a = chg_rec(S, sv[j - 1]), b = chg_rec(S, sv[j]);
  if (Ra.rt[a] != Rb.rt[b]) return true;
  const uint64_t *ka = Ra.key(a), *kb = Rb.key(b);
  if (ka[0] == kb[0] && ka[1] == kb[1] && ka[2] == kb[2] && ka[3] == kb[3]) return false;
  *tie = ka[0] == kb[0];
  return true;
}
KH_HD bool chg_same_key(const ChgSrc& S, uint64_t sa, uint64_t sb) {
  const Recs &Ra = chg_recs(S, sa), &Rb = chg_recs(S, sb);
  const uint32_t a = chg_rec(S, sa), b = chg_rec(S, sb);
  if (Ra.rt[a] != Rb.rt[b]) return false;
  const uint64_t *ka = Ra.key(a), *kb = Rb.key(b);
  return ka[0] == kb[0] && ka[1] == kb[1] && ka[2] == kb[2] && ka[3] == kb[3];
}
// The run that starts at head j of the n sorted slots sv: false when S and C agree on its key; else
// *po = the journal position of the savepoint's entry (NONE: the key is not in S) and *rn = the
// record of the current entry (NONE: the key is not in C).
KH_HD bool chg_join(const ChgSrc& S, const uint32_t* sv, uint64_t n, uint64_t j, uint32_t* po, uint32_t* rn) {
  uint64_t so = ~0ULL, sn = ~0ULL;
  for (uint64_t e = j; e < n && (e == j || chg_same_key(S, sv[j], sv[e])); ++e) {
    const uint64_t s = sv[e];
    if (chg_old(S, s))
      so = s < so ? s : so;
    else
      sn = s < sn ? s : sn;
  }
  *po = so == ~0ULL ? NONE : chg_rec(S, so);
  *rn = sn == ~0ULL ? NONE : chg_rec(S, sn);
  if (*po == NONE || *rn == NONE) return true;
  const uint32_t p = *po, r = *rn;
  if (S.J.rdb[p] != S.R.rdb[r] || S.J.rvl[p] != S.R.rvl[r]) return true;
  const uint8_t *x = S.heap + S.J.rvo[p], *y = S.heap + S.R.rvo[r];
  if (x == y) return false;  // (a record re-anchored or kept: the same span)
  for (uint32_t i = 0, L = S.J.rvl[p]; i < L; ++i)
    if (x[i] != y[i]) return true;
  return false;
}

// ---- page: is the key of kept slot s at or after the resume point (trie id, key)?
KH_HD bool chg_from(const ChgSrc& S, uint64_t s, uint32_t from_trie, const uint64_t* from) {
  const Recs& R = chg_recs(S, s);
  const uint32_t r = chg_rec(S, s), t = R.rt[r];
  if (t != from_trie) return t > from_trie;
  return key_cmp(R.key(r), from) >= 0;
}
// the two sides of the answer's items as diff.h reads them: a's records, b's records (no anchor
// map: nothing is probed), and the item of a difference (po, rn)
KH_HD DSide chg_side(const ChgSrc& S, bool journal) {
  return DSide{journal ? S.J : S.R, AMap{{nullptr}, {nullptr}, 0}, S.heap};
}
KH_HD void chg_item(uint32_t po, uint32_t rn, bool reverse, uint32_t* ia, uint32_t* ib) {
  *ia = reverse ? rn : po;
  *ib = reverse ? po : rn;
}
KH_HD uint32_t chg_item_trie(const DSide& A, uint32_t ra, const DSide& B, uint32_t rb) {
  return ra != NONE ? A.R.rt[ra] : B.R.rt[rb];
}

}  // namespace khst
