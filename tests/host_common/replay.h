// What the stand-alone host replay programs (tests/*_host/*_check.cc) share: hex input and output,
// a record store with its anchor map and export.h's 16-lane encode, the bottom-up builder of a
// trie's canonical records, and the replay of load.h's rounds.  Every body that computes something
// is a KH_HD one of khipu_amd/csrc; the programs are built with g++ -fsanitize=address,undefined
// (tests/hostprog.py) and every array here has exactly the size the replayed code may touch.
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../khipu_amd/csrc/export.h"
#include "../../khipu_amd/csrc/load.h"

using namespace khst;
typedef std::array<uint8_t, 32> Key;
typedef std::vector<uint8_t> Bytes;

static Bytes unhex(const std::string& s) {
  Bytes o;
  if (s == "-") return o;
  for (size_t i = 0; i + 1 < s.size(); i += 2) o.push_back((uint8_t)strtoul(s.substr(i, 2).c_str(), nullptr, 16));
  return o;
}
// empty: what stands for no bytes at all
static void put_hex(const uint8_t* p, size_t n, const char* empty = "-") {
  if (!n) printf("%s", empty);
  for (size_t i = 0; i < n; ++i) printf("%02x", p[i]);
}
static uint32_t nib(const Key& k, uint32_t i) { return (i & 1) ? (k[i >> 1] & 0xF) : (k[i >> 1] >> 4); }
static void kec(const Bytes& e, uint64_t out[4]) {
  std::vector<uint64_t> w((e.size() + 15) / 8, 0);
  memcpy(w.data(), e.data(), e.size());
  kec256_msg<false>((const uint8_t*)w.data(), (uint32_t)e.size(), out);
}

// records with an anchor map over them, and export.h's 16-lane bodies
struct Host {
  uint8_t* recs = nullptr;
  uint8_t* slots = nullptr;
  Bytes heap;
  uint64_t rn = 0, cap = 0;
  Recs R;
  AMap M;

  Host() {}
  // the records rb (a whole number of them) and their value heap: an anchor for every live one
  Host(const Bytes& rb, const Bytes& hp) {
    rn = rb.size() / REC_BYTES;
    init(std::max<uint64_t>(rn, 1));
    memcpy(recs, rb.data(), rn * REC_BYTES);
    heap = hp;
    heap.resize(heap.size() + 8);
    for (uint32_t r = 0; r < rn; ++r) {
      if (R.rlive[r] != REC_LIVE) continue;
      if (map_find(M, R, R.rt[r], R.rd[r], R.key(r)) != NONE) exit(6);  // one live record an anchor
      anchor(r);
    }
  }
  Host(const Host&) = delete;
  ~Host() {
    free(recs);
    free(slots);
  }
  // room for n records (zeroed) and an empty map of at least four slots a record
  void init(uint64_t n) {
    cap = n;
    recs = (uint8_t*)aligned_alloc(128, cap * REC_BYTES);
    memset(recs, 0, cap * REC_BYTES);
    uint64_t mc = 16;
    while (mc < 4 * cap) mc <<= 1;
    slots = (uint8_t*)aligned_alloc(128, mc * 16);
    memset(slots, 0, mc * 16);
    R = recs_at(recs);
    M = AMap{{slots}, {slots}, mc - 1};
  }
  void anchor(uint32_t r) {
    const uint64_t tag = anchor_tag(R.rt[r], R.rd[r], R.key(r));
    uint64_t s = tag & M.mask;
    while (M.tag[s]) s = (s + 1) & M.mask;
    M.tag[s] = tag;
    M.rec[s] = r;
  }
  // the selected nodes of record r through the 16-lane bodies; returns the bytes, len[2] the split
  Bytes encode(uint64_t r, uint32_t sel, uint32_t len[2], uint32_t* size_bytes = nullptr,
               uint32_t* size_cnt = nullptr) {
    uint32_t child[EXP_LANES], il[EXP_LANES], pre[EXP_LANES], S = 0;
    const bool need = exp_needs_children(R, r, sel);
    for (uint32_t c = 0; c < EXP_LANES; ++c) {
      child[c] = need ? exp_child(R, M, r, c) : NONE;
      il[c] = need ? exp_item_len(R, child[c]) : 0;
      pre[c] = S;
      S += il[c];
    }
    uint32_t cnt = 0, bytes = 0;
    exp_sizes(R, heap.data(), r, sel, S, &cnt, &bytes);
    if (size_bytes) *size_bytes = bytes;
    if (size_cnt) *size_cnt = cnt;
    Bytes out(bytes);  // (exactly the sizes form's bytes: an overrun is ASan's)
    for (uint32_t lane = 0; lane < EXP_LANES; ++lane)
      exp_write(R, heap.data(), r, sel, lane, child[lane], pre[lane], S, out.data(), len);
    if (len[0] + len[1] != bytes) {
      fprintf(stderr, "sizes form %u != write form %u + %u (record %llu)\n", bytes, len[0], len[1],
              (unsigned long long)r);
      exit(3);
    }
    return out;
  }
  // one node (sel = EXP_UPPER or EXP_LOWER) of record r
  Bytes encode(uint64_t r, uint32_t sel) {
    uint32_t len[2];
    return encode(r, sel, len);
  }
  // capped reference of an encoding
  void capped(const Bytes& e, uint64_t ref[4], uint8_t* rl) {
    if (e.size() >= 32) {
      kec(e, ref);
      *rl = 32;
    } else {
      words_of(e.data(), (uint32_t)e.size(), ref);
      *rl = (uint8_t)e.size();
    }
  }
};

// a put of a program's input; vb: it leaves khipu's value-only branch (forest.h VB_DEPTH)
struct Put {
  Key k;
  Bytes v;
  bool vb = false;
};

// The canonical records of the trie of the puts (later puts win), built bottom-up -- each node's
// encoding made by export.h's own write bodies and hashed by keccak.h's host path to fill ref /
// bref -- with their anchors (anchor_tag, linear probing).  Records come children in nibble order,
// the parent last: the root is record rn - 1.
struct Builder : Host {
  std::vector<Key> keys;
  std::vector<Bytes> vals;
  std::vector<uint8_t> vb;

  explicit Builder(std::vector<Put> in) {
    std::stable_sort(in.begin(), in.end(), [](const Put& x, const Put& y) { return x.k < y.k; });
    for (size_t i = 0; i < in.size(); ++i) {
      if (i + 1 < in.size() && in[i + 1].k == in[i].k) continue;
      keys.push_back(in[i].k);
      vals.push_back(in[i].v);
      vb.push_back(in[i].vb);
    }
    init(2 * keys.size() + 4);
    if (!keys.empty()) build(0, keys.size(), 0);
  }
  // the trie's root hash (the root's hash even when its encoding is short)
  void root_hash(uint8_t root[32]) {
    memcpy(root, empty_root_hash(), 32);
    if (!rn) return;
    uint64_t h[4];
    kec(encode(rn - 1, EXP_UPPER), h);
    memcpy(root, h, 32);
  }
  // records of the subtrie of sorted keys [lo, hi) hanging at depth d; returns its record
  uint32_t build(size_t lo, size_t hi, uint32_t d) {
    uint32_t db = EL_LEAF, mask = 0;
    if (hi - lo > 1) {
      db = d;
      while (nib(keys[lo], db) == nib(keys[hi - 1], db)) ++db;
      for (size_t i = lo; i < hi;) {
        const uint32_t c = nib(keys[i], db);
        size_t j = i;
        while (j < hi && nib(keys[j], db) == c) ++j;
        build(i, j, db + 1);
        mask |= 1u << c;
        i = j;
      }
    } else if (vb[lo]) {
      if (d != 64) exit(5);  // (a value-only branch hangs under a depth-63 branch)
      db = VB_DEPTH;
    }
    const uint32_t r = (uint32_t)rn++;
    if (rn > cap) exit(4);
    memcpy(R.key(r), keys[lo].data(), 32);
    R.rt[r] = 0;
    R.rd[r] = (uint8_t)d;
    R.rdb[r] = (uint8_t)db;
    R.rmask[r] = (uint16_t)mask;
    R.rlive[r] = REC_LIVE;
    if (db == EL_LEAF || db == VB_DEPTH) {
      R.rvo[r] = heap.size();
      R.rvl[r] = (uint32_t)vals[lo].size();
      heap.insert(heap.end(), vals[lo].begin(), vals[lo].end());
    }
    uint64_t ref[4];
    uint8_t rl;
    if (exp_has_lower(d, db)) {  // the branch first, then the extension that refers to it
      capped(encode(r, EXP_LOWER), ref, &rl);
      for (int q = 0; q < 4; ++q) R.rbref[4ull * r + q] = ref[q];
      R.rbrl[r] = rl;
    }
    capped(encode(r, EXP_UPPER), ref, &rl);
    for (int q = 0; q < 4; ++q) R.rref[4ull * r + q] = ref[q];
    R.rrl[r] = rl;
    if (!exp_has_lower(d, db)) {
      for (int q = 0; q < 4; ++q) R.rbref[4ull * r + q] = ref[q];
      R.rbrl[r] = rl;
    }
    anchor(r);
    return r;
  }
};

// ---- the rounds of load.h
// a frontier of exactly cap items (each array its own allocation)
struct Frontier {
  LItems I{};
  explicit Frontier(uint64_t cap) {
    I.pre = new uint64_t[4 * cap];
    I.a = new uint8_t[cap];
    I.d = new uint8_t[cap];
    I.ref = new uint64_t[4 * cap];
    I.rl = new uint8_t[cap];
    I.pref = new uint64_t[4 * cap];
    I.prl = new uint8_t[cap];
    I.j = new uint32_t[cap];
    I.cap = cap;
  }
  Frontier(const Frontier&) = delete;
  ~Frontier() {
    delete[] I.pre;
    delete[] I.a;
    delete[] I.d;
    delete[] I.ref;
    delete[] I.rl;
    delete[] I.pref;
    delete[] I.prl;
    delete[] I.j;
  }
};

// a node store: packed encodings, their hashes sorted (equal hashes: one entry, as the library's
// sort keeps one of equal keys)
struct Store {
  Bytes enc;  // packed (+ 8 bytes of slack for word reads)
  std::vector<uint64_t> off, hash;
  std::vector<uint32_t> idx;
  NStore view() const { return NStore{hash.data(), idx.data(), idx.size(), enc.data(), off.data()}; }
  explicit Store(const std::vector<Bytes>& nodes) {
    off.push_back(0);
    std::vector<std::array<uint64_t, 4>> hs(nodes.size());
    for (size_t i = 0; i < nodes.size(); ++i) {
      enc.insert(enc.end(), nodes[i].begin(), nodes[i].end());
      off.push_back(enc.size());
      kec(nodes[i], hs[i].data());
    }
    enc.resize(enc.size() + 8);
    std::vector<uint32_t> order(nodes.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = (uint32_t)i;
    std::stable_sort(order.begin(), order.end(),
                     [&](uint32_t x, uint32_t y) { return key_cmp(hs[x].data(), hs[y].data()) < 0; });
    for (size_t i = 0; i < order.size(); ++i) {
      if (i && key_cmp(hs[order[i]].data(), hs[order[i - 1]].data()) == 0) continue;
      idx.push_back(order[i]);
      hash.insert(hash.end(), hs[order[i]].begin(), hs[order[i]].end());
    }
  }
};

// what a load or a fill appends: records and value bytes, in allocations of exactly their sizes
struct Result {
  unsigned long long code = OPEN_OK;
  uint32_t rounds = 0;
  uint64_t rn = 0, keys = 0, stubs = 0, decoded = 0;
  Bytes recs, heap;
  std::vector<std::pair<uint32_t, std::array<uint8_t, 32>>> miss;
};

// the library's modes (load_kernels.hip forest_load).  LOAD_FULL: a hash absent from the store is a
// missing node; LOAD_PARTIAL: below the listed roots it is counted and written as a stub;
// LOAD_FILL: round 0 is stubs, not roots, and an absent hash is a stub in every round.
enum LoadMode { LOAD_FULL = 0, LOAD_PARTIAL = 1, LOAD_FILL = 2 };

// The rounds from frontier cur (ni items; deleted here) as the library runs them: count every
// frontier item, scan, stop on an error or a missing node, fill into arrays of exactly the scanned
// sizes.  tries[j]: the trie id of list index j.  heap0: the value offsets of the new records
// start there.  After a failure res holds no records and no heap (all or nothing).
static void rounds(const Store& st, Frontier* cur, uint64_t ni, const std::vector<uint32_t>& tries, LoadMode mode,
                   uint64_t heap0, Result& res) {
  const NStore S = st.view();
  for (; ni && res.rounds < 80; ++res.rounds) {
    const bool partial = mode == LOAD_FILL || (mode == LOAD_PARTIAL && res.rounds > 0);
    std::vector<uint32_t> child(ni), rec(ni), miss(ni), src(ni);
    std::vector<uint64_t> val(ni);
    LCounts C{child.data(), rec.data(), val.data(), miss.data(), src.data()};
    unsigned long long code = OPEN_OK;
    uint64_t nmiss = 0, nstub = 0, ndec = 0;
    for (uint64_t i = 0; i < ni; ++i) {
      uint32_t is_key = 0;
      const unsigned long long c = load_count_item(cur->I, i, S, C, &is_key, partial);
      if (c == OPEN_MISSING)
        ++nmiss;
      else if (c != OPEN_OK)
        code = std::max(code, c);
      res.keys += is_key;
      if (partial && c == OPEN_OK && cur->I.rl[i] == 32) ++(src[i] == NONE ? nstub : ndec);
    }
    uint64_t nchild = 0, nrec = 0, nval = 0;  // the exclusive scans, in place
    for (uint64_t i = 0; i < ni; ++i) {
      const uint32_t c = child[i], r = rec[i];
      const uint64_t v = val[i];
      child[i] = (uint32_t)nchild;
      rec[i] = (uint32_t)nrec;
      val[i] = nval;
      nchild += c;
      nrec += r;
      nval += v;
    }
    if (code != OPEN_OK || nmiss) {
      res.code = code != OPEN_OK ? code : OPEN_MISSING;
      if (code == OPEN_OK)
        for (uint64_t i = 0; i < ni; ++i)
          if (miss[i]) {
            std::array<uint8_t, 32> h;
            memcpy(h.data(), cur->I.ref + 4 * i, 32);
            res.miss.push_back({cur->I.j[i], h});
          }
      res.rn = res.keys = res.stubs = res.decoded = 0;  // what the earlier rounds wrote is cleared
      res.recs.clear();
      res.heap.clear();
      delete cur;
      return;
    }
    // the round's records and values in allocations of their own, appended to the result afterwards
    uint8_t* rr = (uint8_t*)aligned_alloc(128, std::max<uint64_t>(nrec, 1) * REC_BYTES);
    memset(rr, 0, std::max<uint64_t>(nrec, 1) * REC_BYTES);
    uint8_t* hh = new uint8_t[nval];
    Frontier* nxt = new Frontier(nchild);
    for (uint64_t i = 0; i < ni; ++i)
      load_fill_item(cur->I, i, S, C, nxt->I, tries.data(), rr, 0, nrec, hh, 0, nval, partial);
    // (the value offsets of this round's records are relative to the round: rebase them)
    Recs R = recs_at(rr);
    uint64_t seen = 0;
    for (uint64_t r = 0; r < nrec; ++r) {
      if (R.rlive[r] != REC_LIVE) exit(4);  // every scanned place was written
      if (R.rvl[r]) R.rvo[r] += heap0 + res.heap.size();
      seen += load_is_stub(R, r);
    }
    if (seen != nstub) exit(5);
    res.recs.insert(res.recs.end(), rr, rr + nrec * REC_BYTES);
    res.heap.insert(res.heap.end(), hh, hh + nval);
    res.rn += nrec;
    res.stubs += nstub;
    res.decoded += ndec;
    free(rr);
    delete[] hh;
    delete cur;
    cur = nxt;
    ni = nchild;
  }
  delete cur;
  if (ni) res.code = OPEN_BAD;
}

// a load of the listed tries (mode LOAD_FULL or LOAD_PARTIAL); round 0: the roots that are not the
// empty trie's, in list order
static Result load(const Store& st, const std::vector<uint32_t>& tries, const std::vector<Bytes>& roots,
                   LoadMode mode) {
  Result res;
  uint64_t ni = 0;
  for (const Bytes& r : roots) ni += memcmp(r.data(), empty_root_hash(), 32) != 0;
  Frontier* cur = new Frontier(ni);
  uint64_t t = 0;
  for (size_t j = 0; j < roots.size(); ++j) {
    if (memcmp(roots[j].data(), empty_root_hash(), 32) == 0) continue;
    for (int q = 0; q < 4; ++q) cur->I.pre[4 * t + q] = 0;
    memcpy(cur->I.ref + 4 * t, roots[j].data(), 32);
    memcpy(cur->I.pref + 4 * t, roots[j].data(), 32);
    cur->I.a[t] = cur->I.d[t] = 0;
    cur->I.rl[t] = cur->I.prl[t] = 32;
    cur->I.j[t++] = (uint32_t)j;
  }
  rounds(st, cur, ni, tries, mode, 0, res);
  return res;
}
