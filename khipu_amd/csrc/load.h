// Forest load: many tries decoded from one node store into a resident forest, beside what it
// holds (kh_forest_load_nodes), and the bodies of kh_forest_roots / kh_forest_evict.  The open of
// a single trie from a node store (kh_trie_open_nodes, kh_trie_open_partial) is this load with
// the one trie id 0: there is no other walk.
//
// The walk is level-synchronous, the listed roots being round 0.  One round over a frontier of
// ni items (an item is one node to decode: referenced by hash and looked up in the store, or
// embedded in its parent, its < 32-byte encoding carried in the item):
//   count  every item is decoded once and reports what it makes: children (items of the next
//          round), records (0 or 1), value bytes, and whether its hash is absent from the store;
//   scan   exclusive scans of the three counts: the host reads their totals (one sync a round)
//          and sizes the next frontier, the records and the value heap exactly;
//   fill   the same decode again, writing at the scanned places.
// Nothing is claimed with an atomic counter, so the records come in a fixed order -- round by
// round, inside a round in frontier order, a node's children in nibble order, the roots in list
// order -- and two loads of the same inputs give the same records (and the same export order).
//
// load_node is the decode, shared by both passes through a sink (LoadCount / LoadFill), by the
// kernels of load_kernels.hip and by the host replay of tests/load_host.  The per-node rules are
// those of Node.nodeDec and HexPrefix.decode for a 64-nibble key: an embedded node must be shorter
// than 32 bytes where it is pushed, a branch with children cannot start at nibble 64, and a
// HexPrefix flag nibble is 0..3 with a zero pad nibble.  The items of a node are walked in order:
// there is no array of 18 items and no array of 64 nibbles per thread, so nothing is indexed at
// run time in scratch memory.
#pragma once
#include "forest.h"

namespace khst {

// a frontier: one item per node to decode, with the list index of the trie it belongs to
struct LItems {
  uint64_t* pre;   // [cap*4] key prefix: nibbles [0, d) of every key below
  uint8_t* a;      // anchor depth of the record the node belongs to
  uint8_t* d;      // depth at which the node starts (> a: the child of an extension)
  uint64_t* ref;   // [cap*4] hash, or the embedded encoding
  uint8_t* rl;     // 32 = hash, else the embedded length
  uint64_t* pref;  // [cap*4] the capped reference the record's parent holds
  uint8_t* prl;
  uint32_t* j;     // index into the call's trie list
  uint64_t cap;
};
// what the count pass leaves per item (the scans run in place)
struct LCounts {
  uint32_t* child;  // items pushed to the next round
  uint32_t* rec;    // records made (0: an extension, whose branch carries the record)
  uint64_t* val;    // value bytes
  uint32_t* miss;   // 1: a hash reference absent from the store
  uint32_t* src;    // position of the node among the store's sorted hashes (NONE: embedded)
};
constexpr uint32_t LOAD_KEY = 1;  // LoadCount::flags: the record holds one of the trie's keys

struct LoadCount {
  uint32_t child = 0, rec = 0, flags = 0;
  uint64_t val = 0;
  KH_HD void push(const uint64_t*, uint32_t, uint32_t, const uint8_t*, uint32_t, bool, const uint64_t*, uint32_t) {
    ++child;
  }
  KH_HD void record(RecVal&, const uint8_t*, uint32_t vl, bool is_key) {
    rec = 1;
    val = vl;
    if (is_key) flags |= LOAD_KEY;
  }
};
struct LoadFill {
  LItems N;        // the next frontier
  uint64_t cbase;  // this node's first child there
  uint32_t j;
  uint8_t* recs;   // the handle's records
  uint64_t r, rcap;
  uint32_t trie;
  uint8_t* heap;
  uint64_t vo, heap_cap;
  uint32_t k = 0;
  KH_HD void push(const uint64_t* np, uint32_t na, uint32_t nd, const uint8_t* cref, uint32_t crl, bool is_hash,
                  const uint64_t* pr, uint32_t prl) {
    const uint64_t t = cbase + k++;
    if (t >= N.cap) return;  // (the count pass sized the frontier: never taken)
    uint64_t w[4];
    words_of(cref, crl, w);
    for (int q = 0; q < 4; ++q) {
      N.pre[4 * t + q] = np[q];
      N.ref[4 * t + q] = w[q];
      N.pref[4 * t + q] = pr ? pr[q] : w[q];
    }
    N.a[t] = (uint8_t)na;
    N.d[t] = (uint8_t)nd;
    N.rl[t] = (uint8_t)(is_hash ? 32 : crl);
    N.prl[t] = (uint8_t)(pr ? prl : (is_hash ? 32 : crl));
    N.j[t] = j;
  }
  KH_HD void record(RecVal& v, const uint8_t* val, uint32_t vl, bool) {
    if (r >= rcap || vo + vl > heap_cap) return;
    for (uint32_t q = 0; q < vl; ++q) heap[vo + q] = val[q];
    v.t = trie;
    v.vo = vl ? vo : 0;
    v.vl = vl;
    v.live = REC_LIVE;
    rec_store(recs, r, v);
  }
};

// nibble q of a HexPrefix path b (odd: the first nibble shares byte 0 with the flag)
KH_HD uint32_t hp_nibble(const uint8_t* b, bool odd, uint32_t q) {
  if (odd) {
    if (q == 0) return b[0] & 0xF;
    --q;
  }
  const uint8_t x = b[1 + (q >> 1)];
  return (q & 1) ? (x & 0xF) : (x >> 4);
}

// Decode the node e[0, L) of a frontier item (by_hash: it was referenced by the hash h, else it
// is the embedded encoding itself) hanging at depth d under anchor a with key prefix pre; pref /
// prl: the capped reference the record's parent holds.  Returns an OPEN_* code.
template <typename Sink>
KH_HD unsigned long long load_node(const uint8_t* e, uint32_t L, bool by_hash, const uint64_t* h, const uint64_t* pre,
                                   uint32_t a, uint32_t d, const uint64_t* pref, uint32_t prl, Sink& sink) {
  RItem top;
  if (!rlp_valid(e, L, 0, 0) || !rlp_at(e, L, 0, top) || !top.list) return OPEN_BAD;
  if (L >= 32 && !by_hash) return OPEN_BAD;  // an embedded node must be < 32 B
  const int k = rlp_items(e, L, top, nullptr, 0);
  RecVal v;
  for (int q = 0; q < 4; ++q) {
    v.k[q] = pre[q];
    v.ref[q] = pref[q];
    v.bref[q] = 0;
  }
  v.t = 0;
  v.d = (uint8_t)a;
  v.mask = 0;
  v.live = REC_LIVE;
  v.rl = (uint8_t)prl;
  v.brl = 0;
  v.vl = 0;
  v.vo = 0;
  uint64_t own[4];  // the node's capped reference (Node.capped, Node.scala:114)
  uint32_t ownl;
  if (L >= 32) {
    for (int q = 0; q < 4; ++q) own[q] = h[q];
    ownl = 32;
  } else {
    words_of(e, L, own);
    ownl = L;
  }
  if (k == 17) {  // branch [ref_0 .. ref_15, value]
    RItem it;
    uint32_t p = top.off;
    bool none = true;  // no child at all
    for (int c = 0; c < 16; ++c) {
      if (!rlp_at(e, L, p, it)) return OPEN_BAD;
      none = none && !it.list && it.len == 0;
      p = it.next;
    }
    if (!rlp_at(e, L, p, it)) return OPEN_BAD;  // the value item
    for (int q = 0; q < 4; ++q) v.bref[q] = own[q];
    v.brl = (uint8_t)ownl;
    if (it.list || it.len) {
      // a secure trie stores a branch value only in khipu's value-only branch (forest.h VB_DEPTH)
      if (it.list || d != VB_DEPTH || !none) return OPEN_VALUE;
      v.db = (uint8_t)VB_DEPTH;
      sink.record(v, e + it.off, it.len, true);
      return OPEN_OK;
    }
    if (d >= 64) return OPEN_BAD;  // its children would hang past the key's last nibble
    uint32_t mask = 0;
    p = top.off;
    for (int c = 0; c < 16; ++c) {
      const uint32_t st = p;
      if (!rlp_at(e, L, p, it)) return OPEN_BAD;
      p = it.next;
      if (!it.list && it.len == 0) continue;
      uint64_t np[4] = {pre[0], pre[1], pre[2], pre[3]};
      set_nibble(np, d, (uint32_t)c);
      if (!it.list) {
        if (it.len != 32) return OPEN_BAD;
        sink.push(np, d + 1, d + 1, e + it.off, 32, true, nullptr, 0);
      } else {
        if (it.next - st >= 32) return OPEN_BAD;
        sink.push(np, d + 1, d + 1, e + st, it.next - st, false, nullptr, 0);
      }
      mask |= 1u << c;
    }
    v.db = (uint8_t)d;
    v.mask = (uint16_t)mask;
    sink.record(v, nullptr, 0, false);
    return OPEN_OK;
  }
  if (k != 2 || d != a) return OPEN_BAD;  // a leaf / extension hangs where it starts
  RItem i0, i1;
  if (!rlp_at(e, L, top.off, i0) || i0.list || i0.len == 0) return OPEN_BAD;
  if (!rlp_at(e, L, i0.next, i1)) return OPEN_BAD;
  const uint8_t* hp = e + i0.off;
  const uint32_t f = hp[0] >> 4;
  if (f > 3 || (!(f & 1) && (hp[0] & 0xF))) return OPEN_BAD;  // HexPrefix.decode (HexPrefix.scala:30-40)
  const bool odd = (f & 1) != 0, leaf = (f & 2) != 0;
  const uint32_t np = 2 * (i0.len - 1) + (odd ? 1 : 0);
  if (d + np > 64) return OPEN_BAD;
  uint64_t key[4] = {pre[0], pre[1], pre[2], pre[3]};
  for (uint32_t q = 0; q < np; ++q) set_nibble(key, d + q, hp_nibble(hp, odd, q));
  if (leaf) {  // [HP(path, leaf), value]: the key is complete (32-byte keys)
    if (d + np != 64 || i1.list) return OPEN_BAD;
    for (int q = 0; q < 4; ++q) v.k[q] = key[q];
    v.db = EL_LEAF;
    sink.record(v, e + i1.off, i1.len, true);
    return OPEN_OK;
  }
  // extension [HP(shared, ext), ref]: its branch child gets the extension's record (anchor a)
  if (np == 0) return OPEN_BAD;
  if (!i1.list) {
    if (i1.len != 32) return OPEN_BAD;
    sink.push(key, a, d + np, e + i1.off, 32, true, pref, prl);
  } else {
    if (i1.next - i0.next >= 32) return OPEN_BAD;
    sink.push(key, a, d + np, e + i0.next, i1.next - i0.next, false, pref, prl);
  }
  return OPEN_OK;
}

// where frontier item i's encoding lies: the store (pos: its place among the sorted hashes, found
// by the count pass; NONE: look it up) or the item itself.  False: the hash is not in the store.
KH_HD bool load_locate(const LItems& I, uint64_t i, const NStore& S, uint32_t* pos, const uint8_t** e, uint32_t* L) {
  if (I.rl[i] != 32) {
    *pos = NONE;
    *e = (const uint8_t*)(I.ref + 4 * i);
    *L = I.rl[i];
    return true;
  }
  uint64_t p = *pos;
  if (p == NONE) {
    const uint64_t* h = I.ref + 4 * i;
    p = key_lower_bound(S.hash, S.m, h);
    if (p >= S.m || key_cmp(S.hash + 4 * p, h) != 0) return false;  // MPTNodeMissingException
    *pos = (uint32_t)p;
  }
  const uint32_t n = S.idx[p];
  *e = S.enc + S.off[n];
  *L = (uint32_t)(S.off[n + 1] - S.off[n]);
  return true;
}

// the stub (forest.h EL_STUB) a partial load leaves for frontier item i, whose hash is absent from
// the store: the item itself, kept as a record (load_stub_item is the way back)
KH_HD void load_stub_record(const LItems& I, uint64_t i, uint32_t trie, uint8_t* recs, uint64_t r, uint64_t rcap) {
  if (r >= rcap) return;
  RecVal v;
  for (int q = 0; q < 4; ++q) {
    v.k[q] = I.pre[4 * i + q];
    v.ref[q] = I.pref[4 * i + q];
    v.bref[q] = I.ref[4 * i + q];
  }
  v.t = trie;
  v.d = I.a[i];
  v.db = EL_STUB;
  v.mask = (uint16_t)(I.d[i] | (I.d[i] > I.a[i] ? STUB_BRANCH : 0));  // (an extension's child is a branch)
  v.live = REC_LIVE;
  v.rl = I.prl[i];
  v.brl = 32;
  v.vl = 0;
  v.vo = 0;
  rec_store(recs, r, v);
}
// fill: frontier item t of list index j from stub record r
KH_HD void load_stub_item(const Recs& R, uint64_t r, const LItems& N, uint64_t t, uint32_t j) {
  if (t >= N.cap) return;
  for (int q = 0; q < 4; ++q) {
    N.pre[4 * t + q] = R.rk[4 * r + q];
    N.ref[4 * t + q] = R.rbref[4 * r + q];
    N.pref[4 * t + q] = R.rref[4 * r + q];
  }
  N.a[t] = R.rd[r];
  N.d[t] = (uint8_t)R.rmask[r];
  N.rl[t] = 32;
  N.prl[t] = R.rrl[r];
  N.j[t] = j;
}

// count pass, item i; returns the OPEN_* code (OPEN_MISSING: C.miss[i] is set).  partial: a hash
// absent from the store makes a stub (one record) instead
KH_HD unsigned long long load_count_item(const LItems& I, uint64_t i, const NStore& S, const LCounts& C,
                                         uint32_t* is_key, bool partial = false) {
  C.child[i] = 0;
  C.rec[i] = 0;
  C.val[i] = 0;
  C.miss[i] = 0;
  C.src[i] = NONE;
  *is_key = 0;
  uint32_t pos = NONE, L;
  const uint8_t* e;
  if (!load_locate(I, i, S, &pos, &e, &L)) {
    if (partial) {  // the subtree stays a stub: one record, no children, no value
      C.rec[i] = 1;
      return OPEN_OK;
    }
    C.miss[i] = 1;
    return OPEN_MISSING;
  }
  C.src[i] = pos;
  LoadCount sink;
  const unsigned long long code = load_node(e, L, I.rl[i] == 32, I.ref + 4 * i, I.pre + 4 * i, I.a[i], I.d[i],
                                            I.pref + 4 * i, I.prl[i], sink);
  if (code != OPEN_OK) return code;
  C.child[i] = sink.child;
  C.rec[i] = sink.rec;
  C.val[i] = sink.val;
  *is_key = sink.flags & LOAD_KEY;
  return OPEN_OK;
}
// fill pass, item i: C holds the exclusive scans of the counts (src as the count pass left it)
KH_HD void load_fill_item(const LItems& I, uint64_t i, const NStore& S, const LCounts& C, const LItems& N,
                          const uint32_t* tries, uint8_t* recs, uint64_t rbase, uint64_t rcap, uint8_t* heap,
                          uint64_t hbase, uint64_t heap_cap, bool partial = false) {
  uint32_t pos = C.src[i], L;
  const uint8_t* e;
  if (I.rl[i] == 32 && pos == NONE) {  // absent from the store: nothing, or the stub the count pass counted
    if (partial) load_stub_record(I, i, tries[I.j[i]], recs, rbase + C.rec[i], rcap);
    return;
  }
  if (!load_locate(I, i, S, &pos, &e, &L)) return;
  LoadFill sink{N, C.child[i], I.j[i], recs, rbase + C.rec[i], rcap, tries[I.j[i]], heap, hbase + C.val[i], heap_cap};
  load_node(e, L, I.rl[i] == 32, I.ref + 4 * i, I.pre + 4 * i, I.a[i], I.d[i], I.pref + 4 * i, I.prl[i], sink);
}

// ---- kh_forest_roots / kh_forest_evict: one streaming pass over the records
// a trie's root record: live, anchored at depth 0 (its rref is the root hash)
KH_HD bool load_is_root(const Recs& R, uint64_t r) { return R.rlive[r] == REC_LIVE && R.rd[r] == 0; }
// a live record of one of the nt sorted trie ids
KH_HD bool load_in_list(const Recs& R, uint64_t r, const uint32_t* tries, uint32_t nt) {
  if (R.rlive[r] != REC_LIVE) return false;
  const uint32_t t = R.rt[r], s = seg_of(tries, nt, t);
  return s < nt && tries[s] == t;
}
KH_HD bool load_holds_key(const Recs& R, uint64_t r) { return R.rdb[r] == EL_LEAF || R.rdb[r] == VB_DEPTH; }
KH_HD bool load_is_stub(const Recs& R, uint64_t r) { return R.rlive[r] == REC_LIVE && R.rdb[r] == EL_STUB; }

// ---- kh_trie_evict_subtrees: the inverse of the fill.  A prefix (trie, p nibbles) names the
// subtree that hangs there: the live record anchored at exactly (trie, p, prefix).
//   probe  one map_find a prefix: status, the hash to fetch, the record;
//   flag   one streaming pass over the records (their first line): a record dies iff an evicted
//          prefix of its trie is a proper prefix of its anchor path;
//   stub   the anchors' records rewritten in place as plain stubs (the anchor tag and map_find's
//          check read only the first p nibbles, so the record keeps its map slot).
constexpr uint8_t EVICT_NONE = 0, EVICT_DONE = 1, EVICT_STUB = 2, EVICT_EMBEDDED = 3;  // (khst.h KH_EVICT_*)
// the evicted prefixes, sorted by (trie, zero-padded path), none equal to or extending another
struct EvictList {
  const uint32_t* trie;
  const uint64_t* path;  // [m*4] zero past the depth
  const uint8_t* depth;
  uint64_t m;
};

// prefix (t, p, P): its status; *rec the record found there (NONE: none), hash the one to fetch
// (zero for NONE and EMBEDDED), *is_key: the record holds one of the trie's keys
KH_HD uint8_t evict_probe(const AMap& M, const Recs& R, uint32_t t, uint32_t p, const uint64_t* P, uint32_t* rec,
                          uint64_t hash[4], uint8_t* is_key) {
  for (int q = 0; q < 4; ++q) hash[q] = 0;
  *is_key = 0;
  const uint32_t r = map_find(M, R, t, p, P);
  *rec = r;
  if (r == NONE || R.rlive[r] != REC_LIVE) {
    *rec = NONE;
    return EVICT_NONE;
  }
  if (R.rdb[r] == EL_STUB) {
    for (int q = 0; q < 4; ++q) hash[q] = R.rbref[4ull * r + q];
    return EVICT_STUB;
  }
  if (R.rrl[r] < 32) return EVICT_EMBEDDED;
  for (int q = 0; q < 4; ++q) hash[q] = R.rref[4ull * r + q];
  *is_key = load_holds_key(R, r) ? 1 : 0;
  return EVICT_DONE;
}

// the last entry of E not after (t, K) in (trie, path) order, plus one (0: none)
KH_HD uint64_t evict_upper_bound(const EvictList& E, uint32_t t, const uint64_t* K) {
  uint64_t lo = 0, hi = E.m;
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    const uint32_t mt = E.trie[mid];
    const int c = mt != t ? (mt < t ? -1 : 1) : key_cmp(E.path + 4 * mid, K);
    if (c <= 0)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}
// does live record r lie strictly below an evicted prefix?  Every key between a zero-padded prefix
// and a key that starts with it starts with it too, and no listed prefix extends another: so the
// only candidate is the predecessor of the record's key in the sorted list.
KH_HD bool evict_covers(const Recs& R, uint64_t r, const EvictList& E) {
  if (R.rlive[r] != REC_LIVE) return false;
  const uint64_t* K = R.key(r);
  const uint32_t t = R.rt[r];
  const uint64_t u = evict_upper_bound(E, t, K);
  if (u == 0) return false;
  const uint64_t i = u - 1;
  return E.trie[i] == t && E.depth[i] < R.rd[r] && prefix_eq(E.path + 4 * i, K, E.depth[i]);
}
// record r, anchored at depth p, becomes the plain stub that stands for it: what a partial load
// leaves for a hash the store lacks (load_stub_record with the item's d == a)
KH_HD void evict_stub_record(const Recs& R, uint64_t r, uint32_t p) {
  RecVal v;
  for (int q = 0; q < 4; ++q) {
    v.k[q] = prefix_word(R.key(r), p, q);
    v.ref[q] = v.bref[q] = R.rref[4 * r + q];
  }
  v.t = R.rt[r];
  v.d = (uint8_t)p;
  v.db = EL_STUB;
  v.mask = (uint16_t)p;
  v.live = REC_LIVE;
  v.rl = 32;
  v.brl = 32;
  v.vl = 0;
  v.vo = 0;
  rec_store(R.rk.b, r, v);
}

}  // namespace khst
