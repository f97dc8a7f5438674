// Range verification (kh_verify_ranges, kh_dev_verify_ranges): a page of entries checked against a
// root without a handle -- the receiving half of kh_trie_range_host + KH_PROVE_TRIE_KEYS, geth's
// VerifyRangeProof.  Per range s with origin o, entries k_1 < .. < k_m and hi = k_m (o when m = 0):
//
//   order   one thread an entry: k_i against its predecessor (k_1 against o), its value not empty
//   walk    two walks from the root over the node set, one along o (side 0) and one along hi
//           (side 1).  A branch's children below o's prefix are KEPT on the left, those above
//           hi's prefix KEPT on the right (the trie holds more keys: RV_MORE), the ones on a path
//           are entered, the ones strictly between are dropped: the entries must account for
//           them.  A leaf or an extension that leaves both paths is kept as the node itself, or
//           dropped when it lies within.  Where both paths still coincide side 0 alone emits, so
//           nothing is kept twice.  A kept subtree is an ELEMENT of the rebuild: its key prefix,
//           the depth at which the kept node starts, its reference (a hash or an embedded list).
//   build   the entries (leaves) and the kept subtrees (forest.h's opaque subtree elements, db =
//           oldd = the depth the node hangs at, bref = cref = its reference) of every range that
//           is still in the run go through ONE segmented element build (run_build).  A kept
//           element the topology hangs anywhere but at its own depth stands for a response that
//           omits or invents entries (rv_moved); a segment's root is compared with the given one.
//
// The walk is run twice with one body (rv_walk with a counting and a filling sink), the kept
// counts scanned in between: no slot is claimed with an atomic.  KH_HD bodies only, shared by
// rangeverify_kernels.hip and the host replay of tests/rangeverify_host.
#pragma once
#include "load.h"
#include "range.h"

namespace khst {

enum RangeStatus : uint8_t {
  RANGE_OK = 0,
  RANGE_BAD_ORDER = 1,
  RANGE_MISSING = 2,
  RANGE_BAD_NODE = 3,
  RANGE_BAD_ROOT = 4,
  RANGE_INCOMPLETE = 5,
};
// what a walk returns: a RangeStatus in the low byte (OK, MISSING or BAD_NODE) and
constexpr uint32_t RV_MORE = 0x100;   // a subtree or node was kept on the right
constexpr uint32_t RV_UNDER = 0x200;  // an entry runs under a kept node's prefix: the rebuild would move it
constexpr uint32_t RV_WHOLE = 0x400;  // the root node itself was kept (the trie is that one node)
constexpr uint32_t RV_MAX_STEPS = 160;  // nodes on one path (64 branches, their extensions, embedded ones)

// the call's inputs: keys, roots and origins as 4 little-endian words each
struct RvIn {
  const uint64_t* roots;    // [nr*4]
  const uint64_t* origins;  // [nr*4], nullable: all zero
  const uint8_t* proved;    // [nr]
  uint64_t nr;
  const uint64_t* keys;     // [ne*4]
  const uint64_t* voff;     // [ne+1]
  const uint64_t* ent_off;  // [nr+1]
  NStore S;                 // the node set, hashed and sorted
};
// the elements of the rebuild (host.h ElemArgs / forest.h Elems, input order)
struct RvElems {
  uint64_t* key;   // [cap*4]
  uint32_t* seg;   // [cap] compact segment id of the element's range
  uint8_t* db;     // [cap] EL_LEAF, or the depth at which a kept node starts
  uint64_t* ref;   // [cap*4] a kept node's reference (bref and cref alike)
  uint8_t* rl;     // [cap] 32 = hash, else the embedded length; 0 for an entry
  uint8_t* oldd;   // [cap] = db for a kept node, EL_NEW for an entry
  uint64_t* vo;    // [cap] an entry's value offset
  uint32_t* vl;    // [cap] its length
  uint8_t* side;   // [cap] 0 an entry, 1 kept on the left, 2 kept on the right
  uint64_t cap;
};

KH_HD void rv_origin(const RvIn& I, uint64_t s, uint64_t o[4]) {
  for (int q = 0; q < 4; ++q) o[q] = I.origins ? I.origins[4 * s + q] : 0;
}
// the range of entry i: the last s with ent_off[s] <= i (empty ranges share an offset)
KH_HD uint64_t rv_range_of(const uint64_t* ent_off, uint64_t nr, uint64_t i) {
  uint64_t lo = 0, hi = nr;  // first s with ent_off[s] > i, minus one
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if (ent_off[mid] <= i) lo = mid + 1; else hi = mid;
  }
  return lo - 1;
}
// order: entry i of range s breaks the contract (keys strictly ascending, k_1 >= origin, a value
// of at least one byte)
KH_HD bool rv_order_bad(const RvIn& I, uint64_t s, uint64_t i) {
  if (I.voff[i + 1] == I.voff[i]) return true;
  if (i == I.ent_off[s]) {
    uint64_t o[4];
    rv_origin(I, s, o);
    return key_cmp(I.keys + 4 * i, o) < 0;
  }
  return key_cmp(I.keys + 4 * (i - 1), I.keys + 4 * i) >= 0;
}

// the sinks of the walk: keep(path, d, c, ref, rl, right) -- the subtree under nibbles [0, d) of
// path followed by nibble c (c < 0: the node that starts at depth d itself), referenced by ref[0, rl)
struct RvCount {
  uint32_t n = 0;
  KH_HD void keep(const uint64_t*, uint32_t, int, const uint8_t*, uint32_t, bool) { ++n; }
};
struct RvFill {
  RvElems E;
  uint64_t at;   // the walk's first element
  uint32_t seg;
  uint32_t n = 0;
  KH_HD void keep(const uint64_t* path, uint32_t d, int c, const uint8_t* ref, uint32_t rl, bool right) {
    const uint64_t e = at + n++;
    if (e >= E.cap) return;  // (the count pass sized the arrays: never taken)
    uint64_t k[4], w[4];
    for (int q = 0; q < 4; ++q) k[q] = prefix_word(path, d, q);
    if (c >= 0) set_nibble(k, d, (uint32_t)c);
    words_of(ref, rl, w);
    for (int q = 0; q < 4; ++q) {
      E.key[4 * e + q] = k[q];
      E.ref[4 * e + q] = w[q];
    }
    E.seg[e] = seg;
    E.db[e] = E.oldd[e] = (uint8_t)(c >= 0 ? d + 1 : d);
    E.rl[e] = (uint8_t)rl;
    E.vo[e] = 0;
    E.vl[e] = 0;
    E.side[e] = right ? 2 : 1;
  }
};

// The boundary walk of range s along origin (side 0) or along hi (side 1).  Returns the status
// (RANGE_OK, RANGE_MISSING with the hash in miss, RANGE_BAD_NODE) and the RV_* flags; the walk
// stops at its first problem.
template <typename Sink>
KH_HD uint32_t rv_walk(const RvIn& I, uint64_t s, uint32_t side, uint64_t miss[4], Sink& sink) {
  uint64_t o[4];
  rv_origin(I, s, o);
  const uint64_t e0 = I.ent_off[s], m = I.ent_off[s + 1] - e0;
  const uint64_t* hi = m ? I.keys + 4 * (e0 + m - 1) : o;
  const uint64_t* path = side ? hi : o;
  const uint32_t lcp = (uint32_t)lcp_nibbles(load_key(o, 0), load_key(hi, 0));
  const uint8_t* root = (const uint8_t*)(I.roots + 4 * s);
  uint32_t flags = 0;
  if (bytes_eq32(root, empty_root_hash())) return RANGE_OK;
  const uint8_t* ref = root;  // the reference of the node to visit: a hash, or the embedded list
  uint32_t rl = 32, d = 0;
  for (uint32_t step = 0; step < RV_MAX_STEPS; ++step) {
    const uint8_t* e = ref;
    uint32_t L = rl;
    if (rl == 32) {
      uint64_t h[4];
      words_of(ref, 32, h);
      const uint64_t p = key_lower_bound(I.S.hash, I.S.m, h);
      if (p >= I.S.m || key_cmp(I.S.hash + 4 * p, h) != 0) {
        for (int q = 0; q < 4; ++q) miss[q] = h[q];
        return RANGE_MISSING | flags;
      }
      const uint32_t j = I.S.idx[p];
      const uint64_t len = I.S.off[j + 1] - I.S.off[j];
      if (len > 0xFFFFFFFFull) return RANGE_BAD_NODE | flags;
      e = I.S.enc + I.S.off[j];
      L = (uint32_t)len;
    }
    RItem top;
    if (!rlp_at(e, L, 0, top) || !top.list || top.next != L) return RANGE_BAD_NODE | flags;
    const int cnt = rlp_items(e, L, top, nullptr, 0);
    const bool co = lcp >= d;  // both paths run through this node
    if (cnt == 17) {
      RItem it;
      uint32_t p = top.off;
      if (d == 64) {  // khipu's value-only branch: a leaf whose key is the path itself, so within
        for (int c = 0; c < 17; ++c) {
          if (!rlp_at(e, L, p, it)) return RANGE_BAD_NODE | flags;
          p = it.next;
        }
        return (it.list ? RANGE_BAD_NODE : RANGE_OK) | flags;
      }
      const int nib = (int)rng_nibble(path, d), hn = (int)rng_nibble(hi, d);
      const uint8_t* nref = nullptr;
      uint32_t nrl = 0;
      for (int c = 0; c < 16; ++c) {
        const uint32_t st = p;
        if (!rlp_at(e, L, p, it)) return RANGE_BAD_NODE | flags;
        p = it.next;
        const uint8_t* cr;
        uint32_t cl;
        if (!it.list) {
          if (it.len == 0) continue;
          if (it.len != 32) return RANGE_BAD_NODE | flags;
          cr = e + it.off;
          cl = 32;
        } else {
          if (it.next - st >= 32) return RANGE_BAD_NODE | flags;  // an embedded node is shorter than a hash
          cr = e + st;
          cl = it.next - st;
        }
        if (c == nib) {
          nref = cr;
          nrl = cl;
        } else if (side == 0 && c < nib) {
          sink.keep(path, d, c, cr, cl, false);
        } else if (side == 0 ? (co && c > hn) : (!co && c > nib)) {
          sink.keep(path, d, c, cr, cl, true);
          flags |= RV_MORE;
        }
      }
      if (!nref) return RANGE_OK | flags;  // an empty slot: the path ends
      ref = nref;
      rl = nrl;
      ++d;
      continue;
    }
    if (cnt != 2) return RANGE_BAD_NODE | flags;  // (a list overrun included: cnt < 0)
    RItem i0, i1;
    if (!rlp_at(e, L, top.off, i0) || i0.list || i0.len == 0) return RANGE_BAD_NODE | flags;
    if (!rlp_at(e, L, i0.next, i1)) return RANGE_BAD_NODE | flags;
    const uint8_t* hp = e + i0.off;
    const uint32_t f = hp[0] >> 4;
    if (f > 3 || (!(f & 1) && (hp[0] & 0xF))) return RANGE_BAD_NODE | flags;
    const bool odd = (f & 1) != 0, leaf = (f & 2) != 0;
    const uint32_t pn = 2 * (i0.len - 1) + (odd ? 1 : 0);
    if (d + pn > 64) return RANGE_BAD_NODE | flags;
    const uint8_t* cr = nullptr;
    uint32_t cl = 0;
    if (leaf) {
      if (i1.list || d + pn != 64) return RANGE_BAD_NODE | flags;
    } else if (!i1.list) {
      if (i1.len != 32) return RANGE_BAD_NODE | flags;
      cr = e + i1.off;
      cl = 32;
    } else {
      if (i1.next - i0.next >= 32) return RANGE_BAD_NODE | flags;
      cr = e + i0.next;
      cl = i1.next - i0.next;
    }
    // the node's full prefix q (the path's first d nibbles, then its own) against o and hi
    int co_ = side ? 1 : 0, ch_ = side ? 0 : -1;  // past the split: side 0 is below hi, side 1 above o
    bool so = co || side == 0, sh = co || side == 1;  // still equal to o's / hi's prefix
    for (uint32_t q = 0; q < pn; ++q) {
      const int x = (int)hp_nibble(hp, odd, q);
      if (so) {
        const int y = (int)rng_nibble(o, d + q);
        if (x != y) {
          co_ = x < y ? -1 : 1;
          so = false;
        }
      }
      if (sh) {
        const int y = (int)rng_nibble(hi, d + q);
        if (x != y) {
          ch_ = x < y ? -1 : 1;
          sh = false;
        }
      }
    }
    if (so) co_ = 0;
    if (sh) ch_ = 0;
    if (!leaf && (side ? ch_ : co_) == 0) {  // an extension on this side's path: entered
      ref = cr;
      rl = cl;
      d += pn;
      continue;
    }
    // kept as the node itself (below o, or above hi), or dropped (within, or the other side's)
    const bool left = side == 0 && co_ < 0, right = side == 0 ? (co && ch_ > 0) : (!co && ch_ > 0);
    if (left || right) {
      sink.keep(path, d, -1, ref, rl, right);
      if (right) flags |= RV_MORE;
      if (d == 0) flags |= RV_WHOLE;
      // an entry under the node's place would push it down: with entries, hi itself runs there
      // on the right; on the left the first entry does iff it shares the path's first d nibbles
      if (m && (right || prefix_eq(I.keys + 4 * e0, o, d))) flags |= RV_UNDER;
    }
    return RANGE_OK | flags;
  }
  return RANGE_BAD_NODE | flags;
}

// what the count pass leaves per (range, side), and the plan made of both sides
struct RvWalkOut {
  uint32_t* st;    // [2*nr] rv_walk's return
  uint32_t* cnt;   // [2*nr] kept elements
  uint64_t* miss;  // [2*nr*4]
};
// Range s after the order check and the count pass: its status so far and `more`; returns the
// elements it brings to the build (0: the range is decided, *final set) .
KH_HD uint64_t rv_plan(const RvIn& I, uint64_t s, uint32_t order_bad, const RvWalkOut& W, uint8_t* status,
                       uint8_t* more, uint64_t miss[4], bool* final) {
  const uint64_t m = I.ent_off[s + 1] - I.ent_off[s];
  *more = 0;
  *final = true;
  for (int q = 0; q < 4; ++q) miss[q] = 0;
  if (order_bad) {
    *status = RANGE_BAD_ORDER;
    return 0;
  }
  if (!I.proved[s]) {
    *final = m == 0;
    *status = (m == 0 && !bytes_eq32((const uint8_t*)(I.roots + 4 * s), empty_root_hash())) ? RANGE_BAD_ROOT : RANGE_OK;
    return m;
  }
  const uint32_t a = W.st[2 * s], b = W.st[2 * s + 1];
  if ((a & 0xFF) == RANGE_BAD_NODE || (b & 0xFF) == RANGE_BAD_NODE) {
    *status = RANGE_BAD_NODE;
    return 0;
  }
  if ((a & 0xFF) == RANGE_MISSING || (b & 0xFF) == RANGE_MISSING) {
    const uint64_t* h = W.miss + 4 * (2 * s + ((a & 0xFF) == RANGE_MISSING ? 0 : 1));
    for (int q = 0; q < 4; ++q) miss[q] = h[q];
    *status = RANGE_MISSING;
    return 0;
  }
  const uint32_t fl = a | b;
  *more = (fl & RV_MORE) ? 1 : 0;
  if (m == 0 && (fl & RV_MORE)) {
    *status = RANGE_INCOMPLETE;
    return 0;
  }
  if (fl & RV_UNDER) {
    *status = RANGE_BAD_ROOT;
    return 0;
  }
  const uint64_t n = m + W.cnt[2 * s] + W.cnt[2 * s + 1];
  if (fl & RV_WHOLE) {  // (no entries: the kept root node is the whole trie, found by the root's hash)
    *status = RANGE_OK;
    return 0;
  }
  if (n == 0) {
    *status = bytes_eq32((const uint8_t*)(I.roots + 4 * s), empty_root_hash()) ? RANGE_OK : RANGE_BAD_ROOT;
    return 0;
  }
  *final = false;
  *status = RANGE_OK;
  return n;
}

// entry i of range s as element e of segment seg
KH_HD void rv_entry_elem(const RvIn& I, uint64_t i, const RvElems& E, uint64_t e, uint32_t seg) {
  if (e >= E.cap) return;
  for (int q = 0; q < 4; ++q) {
    E.key[4 * e + q] = I.keys[4 * i + q];
    E.ref[4 * e + q] = 0;
  }
  E.seg[e] = seg;
  E.db[e] = EL_LEAF;
  E.oldd[e] = EL_NEW;
  E.rl[e] = 0;
  E.vo[e] = I.voff[i];
  E.vl[e] = (uint32_t)(I.voff[i + 1] - I.voff[i]);
  E.side[e] = 0;
}

// after the build: sorted element i (input index sidx[i]) is a kept node that the topology hangs
// at pd + 1 instead of its own depth -- its parent branch would have it as the only child, or
// keys ran under its prefix
KH_HD bool rv_moved(const RvElems& E, uint32_t in, int pd) {
  return E.side[in] != 0 && (uint32_t)(pd + 1) != (uint32_t)E.oldd[in];
}

}  // namespace khst
