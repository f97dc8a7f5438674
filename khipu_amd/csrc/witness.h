// Commit witnesses (kh_trie_commit_witness_host): the nodes a partial handle must hold to commit a
// batch of upserts and deletes at the first attempt -- the proof paths of the op keys, and the one
// child the reference's fix loads when a delete leaves a branch a single child
// (MerklePatriciaTrie.scala:430-477).
//
// One walk per op (prove.h's descent: the same hits) also records, per VISITED record, what the
// batch does under it; the visited branch records are then judged deepest first:
//   a slot is non-empty after the batch when its child record is unvisited (no op key lies under
//   it), or visited and ALIVE; a record is alive when an effective upsert (one no delete of the
//   batch cancels) lies under its anchor, else a leaf when no delete names its key, a branch when
//   one of its slots is non-empty or newly filled;
//   a branch whose one non-empty slot is an old one COLLAPSES: the node in that slot is needed --
//   listed when it is unvisited (a visited one is on a path already) and referred to by hash.
// The visited set is an open-addressing table keyed by record index, sized by the walks' visits;
// the deletes of the batch are a second one keyed by (trie, key), which the upserts are looked up in.
//
// KH_HD bodies only (the kernels are prove_kernels.hip's, the host replay tests/witness_host's).
#pragma once
#include "prove.h"

namespace khst {

// ---- the words the walks share: or-ed and claimed atomically on the device, plainly on the host
KH_HD uint32_t wit_or(uint32_t* p, uint32_t v) {
#ifdef __HIP_DEVICE_COMPILE__
  return atomicOr(p, v);
#else
  const uint32_t o = *p;
  *p = o | v;
  return o;
#endif
}
KH_HD uint32_t wit_cas(uint32_t* p, uint32_t expect, uint32_t v) {
#ifdef __HIP_DEVICE_COMPILE__
  return atomicCAS(p, expect, v);
#else
  const uint32_t o = *p;
  if (o == expect) *p = v;
  return o;
#endif
}
// a read that may be stale (the words only gain bits, a slot is claimed once): it saves the atomic
// where the bits are already there -- every op of a batch passes its trie's top records, and one
// atomic per op on their words would serialise there
KH_HD uint32_t wit_peek(const uint32_t* p) {
#ifdef __HIP_DEVICE_COMPILE__
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  return *p;
#endif
}
KH_HD void wit_set(uint32_t* p, uint32_t v) {
  if ((wit_peek(p) & v) != v) wit_or(p, v);
}
KH_HD uint32_t wit_popc16(uint32_t m) {
  uint32_t c = 0;
  for (m &= 0xFFFFu; m; m &= m - 1) ++c;
  return c;
}

// ---- the deletes of the batch: slots hold the op index of a delete (NONE: empty); K / T are the
// trie keys and trie ids of all ops (T null: one trie)
struct WDels {
  uint32_t* idx;
  uint64_t mask;  // slots - 1 (a power of two, at least twice the deletes)
};
KH_HD uint64_t wit_key_hash(uint32_t t, const uint64_t* k) {
  uint64_t h = fmix64((uint64_t)t ^ 0x9E3779B97F4A7C15ULL);
  for (int q = 0; q < 4; ++q) h = fmix64(h ^ k[q] ^ (0x632BE59BD9B4E019ULL * (q + 1)));
  return h;
}
KH_HD bool wit_same_op(const uint64_t* K, const uint32_t* T, uint64_t i, uint32_t t, const uint64_t* key) {
  const uint64_t* L = K + 4 * i;
  return (T ? T[i] : 0u) == t && L[0] == key[0] && L[1] == key[1] && L[2] == key[2] && L[3] == key[3];
}
// delete i into the set (a repeated key keeps the first index claimed)
KH_HD void wdels_insert(const WDels& D, const uint64_t* K, const uint32_t* T, uint64_t i) {
  const uint32_t t = T ? T[i] : 0u;
  const uint64_t* key = K + 4 * i;
  for (uint64_t s = wit_key_hash(t, key) & D.mask, n = 0; n <= D.mask; s = (s + 1) & D.mask, ++n) {
    const uint32_t o = wit_cas(&D.idx[s], NONE, (uint32_t)i);
    if (o == NONE || wit_same_op(K, T, o, t, key)) return;
  }
}
KH_HD bool wdels_has(const WDels& D, const uint64_t* K, const uint32_t* T, uint32_t t, const uint64_t* key) {
  for (uint64_t s = wit_key_hash(t, key) & D.mask, n = 0; n <= D.mask; s = (s + 1) & D.mask, ++n) {
    const uint32_t o = D.idx[s];
    if (o == NONE) return false;
    if (wit_same_op(K, T, o, t, key)) return true;
  }
  return false;
}

// ---- the visited records: rec[s] the record of slot s (NONE: empty), st[s] its flags, mk[s] its
// slot masks -- low half: the child nibbles a walk went into; high half: the empty slots an
// effective upsert lands in
enum : uint32_t {
  WS_UP = 1,       // an effective upsert lies under the record's anchor
  WS_DEAD = 2,     // a leaf (or value-only branch) whose key the batch deletes
  WS_ALIVE = 4,    // a branch record judged non-empty after the batch (wit_eval)
  WS_REACHED = 8,  // a stub an op's walk ends in: listed once
};
struct WSet {
  uint32_t* rec;
  uint32_t* st;
  uint32_t* mk;
  uint64_t mask;  // slots - 1 (a power of two, at least twice the visits)
};
constexpr uint64_t WS_ABSENT = ~0ULL;
KH_HD uint64_t wset_insert(const WSet& V, uint32_t r) {
  for (uint64_t s = fmix64(r) & V.mask, n = 0; n <= V.mask; s = (s + 1) & V.mask, ++n) {
    uint32_t o = wit_peek(&V.rec[s]);
    if (o == NONE) o = wit_cas(&V.rec[s], NONE, r);
    if (o == NONE || o == r) return s;
  }
  return WS_ABSENT;  // (cannot happen: the table holds twice the visits)
}
KH_HD uint64_t wset_find(const WSet& V, uint32_t r) {
  for (uint64_t s = fmix64(r) & V.mask, n = 0; n <= V.mask; s = (s + 1) & V.mask, ++n) {
    const uint32_t o = V.rec[s];
    if (o == NONE) return WS_ABSENT;
    if (o == r) return s;
  }
  return WS_ABSENT;
}

// ---- the walk of one op key: prove_walk's descent and hits, visit(r, c) for every record it
// comes to (c: the nibble r hangs by under the record visited before it, 16 at the root), and
// where it ends
enum : uint32_t {
  WE_OTHER = 0,  // an empty trie, a leaf of another key, or the key leaves an extension
  WE_SLOT = 1,   // the empty slot `nib` of the branch of record `rec`
  WE_LEAF = 2,   // the leaf (or value-only branch) `rec` that holds the key
  WE_STUB = 3,   // the stub `rec`: the subtree is not held
};
struct WitEnd {
  uint32_t found;  // prove_walk's answer
  uint32_t kind, rec, nib;
};
template <typename Hit, typename Visit>
KH_HD WitEnd wit_walk(const AMap& M, const Recs& R, uint32_t t, const uint64_t* key, Hit hit, Visit visit) {
  const Key4 k4 = load_key(key, 0);
  uint32_t d = 0, prev = NONE;
  for (int step = 0; step < 70; ++step) {
    const uint32_t r = map_find(M, R, t, d, key);
    if (r == NONE) {
      if (prev == NONE) return WitEnd{0, WE_OTHER, NONE, 0};
      return WitEnd{0, WE_SLOT, prev, key_nibble(k4, (int)d - 1)};
    }
    visit(r, d ? key_nibble(k4, (int)d - 1) : 16u);
    const uint32_t db = R.rdb[r];
    if (db == EL_STUB) {
      const uint32_t md = R.rmask[r] & 0xFF;
      if (md > d && (R.rrl[r] == 32 || d == 0)) hit(2ull * r);
      if (md > d && lcp_nibbles(k4, load_key(R.key(r), 0)) < (int)md) return WitEnd{0, WE_OTHER, r, 0};
      return WitEnd{2, WE_STUB, r, 0};
    }
    if (R.rrl[r] == 32 || d == 0) hit(2ull * r);
    const uint64_t* L = R.key(r);
    const bool same = L[0] == key[0] && L[1] == key[1] && L[2] == key[2] && L[3] == key[3];
    if (db == EL_LEAF) return WitEnd{same, same ? WE_LEAF : WE_OTHER, r, 0};
    if (exp_has_lower(d, db)) {
      if (lcp_nibbles(k4, load_key(L, 0)) < (int)db) return WitEnd{0, WE_OTHER, r, 0};
      if (R.rbrl[r] == 32) hit(2ull * r + 1);
    }
    if (db == VB_DEPTH) return WitEnd{same, same ? WE_LEAF : WE_OTHER, r, 0};
    prev = r;
    d = db + 1;
  }
  return WitEnd{0, WE_OTHER, NONE, 0};
}

// One op of the batch into the visited set: its hits, its marks, and reach(stub) for the first
// walk that ends in a stub.  up: an effective upsert; del: a delete.
template <typename Hit, typename Reach>
KH_HD void wit_op(const AMap& M, const Recs& R, const WSet& V, uint32_t t, const uint64_t* key, bool up, bool del,
                  Hit hit, Reach reach) {
  uint64_t ps = WS_ABSENT;
  const WitEnd e = wit_walk(M, R, t, key, hit, [&](uint32_t r, uint32_t c) {
    const uint64_t s = wset_insert(V, r);
    if (s == WS_ABSENT) return;
    if (up) wit_set(&V.st[s], WS_UP);
    if (ps != WS_ABSENT && c < 16) wit_set(&V.mk[ps], 1u << c);
    ps = s;
  });
  if (ps == WS_ABSENT) return;  // an empty trie
  if (e.kind == WE_SLOT && up) wit_set(&V.mk[ps], 0x10000u << e.nib);
  if (e.kind == WE_LEAF && del) wit_set(&V.st[ps], WS_DEAD);
  if (e.kind == WE_STUB && !(wit_or(&V.st[ps], WS_REACHED) & WS_REACHED)) reach(e.rec);
}

// whether the visited record r (slot s) holds a key after the batch; a branch record's answer is
// the one wit_eval left (its depth is greater than the asking branch's: judged in an earlier round)
KH_HD bool wit_alive(const Recs& R, const WSet& V, uint64_t s, uint32_t r) {
  const uint32_t db = R.rdb[r], st = V.st[s];
  if (db == EL_STUB) return true;  // (a walk that only passes its extension leaves the subtree alone)
  if (st & WS_UP) return true;
  if (db == EL_LEAF || db == VB_DEPTH) return !(st & WS_DEAD);
  return (st & WS_ALIVE) != 0;
}
KH_HD bool wit_is_branch(const Recs& R, uint32_t r) { return R.rdb[r] < VB_DEPTH; }

// The visited branch record of slot s judged: its ALIVE flag, and when it collapses onto an
// unvisited child, hit(2 * child) for a child referred to by hash, or miss(child) for a stub of
// unknown kind (forest.h: its anchor would move, which the commit refuses).  A stub that stands
// for the branch under a present extension gives the extension; one whose extension is cut down
// to nothing (STUB_BRANCH, rmask = d) gives nothing.
template <typename Hit, typename Miss>
KH_HD void wit_eval(const AMap& M, const Recs& R, const WSet& V, uint64_t s, Hit hit, Miss miss) {
  const uint32_t r = V.rec[s];
  const uint32_t db = R.rdb[r], t = R.rt[r], mask = R.rmask[r];
  const uint32_t vis = V.mk[s] & mask & 0xFFFFu, fresh = V.mk[s] >> 16;
  const uint32_t rest = mask & ~vis & 0xFFFFu;  // the old slots no walk went into
  uint32_t cnt = wit_popc16(rest) + wit_popc16(fresh);
  uint64_t key[4];
  for (int q = 0; q < 4; ++q) key[q] = R.rk[4ull * r + q];
  for (uint32_t c = 0; c < 16; ++c) {
    if (!(vis >> c & 1)) continue;
    set_nibble(key, db, c);
    const uint32_t r2 = map_find(M, R, t, db + 1, key);
    if (r2 == NONE) continue;  // (cannot happen: a walk went into it)
    const uint64_t s2 = wset_find(V, r2);
    if (s2 == WS_ABSENT || wit_alive(R, V, s2, r2)) ++cnt;
  }
  if (cnt) wit_or(&V.st[s], WS_ALIVE);
  if (cnt != 1 || fresh || wit_popc16(rest) != 1) return;  // (a visited survivor is on a path)
  uint32_t c = 0;
  while (!(rest >> c & 1)) ++c;
  set_nibble(key, db, c);
  const uint32_t r2 = map_find(M, R, t, db + 1, key);
  if (r2 == NONE) return;
  if (R.rdb[r2] == EL_STUB) {
    const uint32_t md = R.rmask[r2] & 0xFF;
    if (md > db + 1) {
      if (R.rrl[r2] == 32) hit(2ull * r2);
    } else if (!(R.rmask[r2] & STUB_BRANCH)) {
      miss(r2);
    }
    return;
  }
  if (R.rrl[r2] == 32) hit(2ull * r2);
}

}  // namespace khst
