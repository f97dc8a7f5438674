// Host replay of the partial load and the fill (khipu_amd/csrc/load.h, forest.h EL_STUB), stand-alone:
// built with g++ -fsanitize=address,undefined by tests/test_partial_host.py and run as a child
// process.
//
//   partial_check FILE
// FILE, one record a line:
//   N enchex          a node of the store the tries are loaded from (the program hashes it)
//   F enchex          a node of the store a fill is then given (no F line: no fill)
//   T id roothex      a listed trie
//   Q id keyhex       a 32-byte key whose get / need / prove walks run on the loaded records
// The program replays the rounds of load.h as the library runs a PARTIAL load -- count every
// frontier item, scan, fill, a hash absent from the store below a root counted and written as a
// stub -- into arrays of exactly the scanned sizes (a write past one is AddressSanitizer's), builds
// an anchor map over the live records, re-encodes every record's nodes through export.h, and runs
// forest_get and prove_walk for the queries.  It prints
//   S code rounds records keys heap_bytes n_missing stubs   (code: an OPEN_* value; 0 = loaded)
//   M idx hashhex                              every missing ROOT
//   B trie a d rrefhex rbrefhex                every stub: anchor depth, depth of the missing node
//   E trie hashhex enchex                      every node a node store needs, per record
//   G i found needhex k hashhex*k              query i: 0 / 1 / 2, the stub's rbref (- if none),
//                                              the hashes of the k nodes its proof lists
//   D 0|1                                      a second replay gave identical arrays
// and, when a fill store is given, the same S / B / E lines prefixed with F for the handle after
// the fill (FS: code rounds live_records keys heap_bytes decoded stubs).  A failed fill leaves the
// records as they were: the F lines then repeat the state before it.
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

#include "../../khipu_amd/csrc/load.h"
#include "../../khipu_amd/csrc/prove.h"

using namespace khst;
typedef std::vector<uint8_t> Bytes;

static Bytes unhex(const std::string& s) {
  Bytes o;
  if (s == "-") return o;
  for (size_t i = 0; i + 1 < s.size(); i += 2) o.push_back((uint8_t)strtoul(s.substr(i, 2).c_str(), nullptr, 16));
  return o;
}
static void put_hex(const uint8_t* p, size_t n) {
  if (!n) printf("-");
  for (size_t i = 0; i < n; ++i) printf("%02x", p[i]);
}
static void kec(const Bytes& e, uint64_t out[4]) {
  std::vector<uint64_t> w((e.size() + 15) / 8, 0);
  memcpy(w.data(), e.data(), e.size());
  kec256_msg<false>((const uint8_t*)w.data(), (uint32_t)e.size(), out);
}

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

// The rounds from frontier cur (ni items; deleted here).  tries[j]: the trie id of list index j.
// root_round: round 0 is the listed roots, where an absent hash is a missing node, not a stub.
// heap0: the value offsets of the new records start there.
static void rounds(const Store& st, Frontier* cur, uint64_t ni, const std::vector<uint32_t>& tries, bool root_round,
                   uint64_t heap0, Result& res) {
  const NStore S = st.view();
  for (; ni && res.rounds < 80; ++res.rounds) {
    const bool partial = !(root_round && res.rounds == 0);
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
      res.rn = res.keys = res.stubs = res.decoded = 0;  // all or nothing
      res.recs.clear();
      res.heap.clear();
      delete cur;
      return;
    }
    uint8_t* rr = (uint8_t*)aligned_alloc(128, std::max<uint64_t>(nrec, 1) * REC_BYTES);
    memset(rr, 0, std::max<uint64_t>(nrec, 1) * REC_BYTES);
    uint8_t* hh = new uint8_t[nval];
    Frontier* nxt = new Frontier(nchild);
    for (uint64_t i = 0; i < ni; ++i)
      load_fill_item(cur->I, i, S, C, nxt->I, tries.data(), rr, 0, nrec, hh, 0, nval, partial);
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

static Result load(const Store& st, const std::vector<uint32_t>& tries, const std::vector<Bytes>& roots) {
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
  rounds(st, cur, ni, tries, true, 0, res);
  return res;
}

// the records with an anchor map over the live ones, and export.h's 16-lane bodies
struct Host {
  uint8_t* recs = nullptr;
  uint8_t* slots = nullptr;
  uint64_t rn = 0;
  Bytes heap;
  Recs R;
  AMap M;
  Host(const Bytes& rb, const Bytes& hp) {
    rn = rb.size() / REC_BYTES;
    const uint64_t n = std::max<uint64_t>(rn, 1);
    recs = (uint8_t*)aligned_alloc(128, n * REC_BYTES);
    memcpy(recs, rb.data(), rn * REC_BYTES);
    uint64_t mc = 16;
    while (mc < 4 * n) mc <<= 1;
    slots = (uint8_t*)aligned_alloc(128, mc * 16);
    memset(slots, 0, mc * 16);
    heap = hp;
    heap.resize(heap.size() + 8);
    R = recs_at(recs);
    M = AMap{{slots}, {slots}, mc - 1};
    for (uint32_t r = 0; r < rn; ++r) {
      if (R.rlive[r] != REC_LIVE) continue;
      if (map_find(M, R, R.rt[r], R.rd[r], R.key(r)) != NONE) exit(6);  // one live record an anchor
      const uint64_t tag = anchor_tag(R.rt[r], R.rd[r], R.key(r));
      uint64_t s = tag & M.mask;
      while (M.tag[s]) s = (s + 1) & M.mask;
      M.tag[s] = tag;
      M.rec[s] = r;
    }
  }
  Host(const Host&) = delete;
  ~Host() {
    free(recs);
    free(slots);
  }
  Bytes encode(uint64_t r, uint32_t sel) {
    uint32_t child[EXP_LANES], il[EXP_LANES], pre[EXP_LANES], S = 0, len[2];
    const bool need = exp_needs_children(R, r, sel);
    for (uint32_t c = 0; c < EXP_LANES; ++c) {
      child[c] = need ? exp_child(R, M, r, c) : NONE;
      il[c] = need ? exp_item_len(R, child[c]) : 0;
      pre[c] = S;
      S += il[c];
    }
    uint32_t cnt = 0, bytes = 0;
    exp_sizes(R, heap.data(), r, sel, S, &cnt, &bytes);
    Bytes out(bytes);
    for (uint32_t lane = 0; lane < EXP_LANES; ++lane)
      exp_write(R, heap.data(), r, sel, lane, child[lane], pre[lane], S, out.data(), len);
    if (len[0] + len[1] != bytes) exit(3);
    return out;
  }
  void print(const char* pfx) {
    for (uint64_t r = 0; r < rn; ++r) {
      if (load_is_stub(R, r)) {
        printf("%sB %u %u %u ", pfx, R.rt[r], (unsigned)R.rd[r], (unsigned)(R.rmask[r] & 0xFF));
        put_hex((const uint8_t*)&R.rref[4 * r], R.rrl[r]);
        printf(" ");
        put_hex((const uint8_t*)&R.rbref[4 * r], R.rbrl[r]);
        printf("\n");
      }
      const uint32_t sel = exp_select(R, r, EXP_ALL_TRIES);
      for (uint32_t which : {EXP_UPPER, EXP_LOWER}) {
        if (!(sel & which)) continue;
        const Bytes e = encode(r, which);
        printf("%sE %u ", pfx, R.rt[r]);
        put_hex(exp_hash_of(R, r, which), 32);
        printf(" ");
        put_hex(e.data(), e.size());
        printf("\n");
      }
    }
  }
};

// kh_trie_fill_nodes on the host: the live stubs the store resolves are round 0 (record order);
// the rounds append; only a success swaps the listed stubs out.  Returns the appended result;
// recs / heap are updated on success.
static Result fill(const Store& st, Bytes& recs, Bytes& heap) {
  Result res;
  Host H(recs, heap);
  const NStore S = st.view();
  std::vector<uint32_t> list;
  for (uint64_t r = 0; r < H.rn; ++r) {
    if (!load_is_stub(H.R, r) || !S.m) continue;
    uint64_t h[4];
    for (int q = 0; q < 4; ++q) h[q] = H.R.rbref[4 * r + q];
    const uint64_t p = key_lower_bound(S.hash, S.m, h);
    if (p < S.m && key_cmp(S.hash + 4 * p, h) == 0) list.push_back((uint32_t)r);
  }
  if (list.empty()) return res;
  Frontier* cur = new Frontier(list.size());
  std::vector<uint32_t> tries(list.size());
  for (size_t t = 0; t < list.size(); ++t) {
    load_stub_item(H.R, list[t], cur->I, t, (uint32_t)t);
    tries[t] = H.R.rt[list[t]];
  }
  rounds(st, cur, list.size(), tries, false, heap.size(), res);
  if (res.code != OPEN_OK) return res;
  Recs R = recs_at(recs.data());
  for (uint32_t r : list) R.rlive[r] = REC_DEAD;
  recs.insert(recs.end(), res.recs.begin(), res.recs.end());
  heap.insert(heap.end(), res.heap.begin(), res.heap.end());
  res.miss.clear();
  res.rn = list.size();  // (reported: the stubs resolved)
  return res;
}

static uint64_t count_live(const Bytes& recs, bool stubs_only) {
  uint64_t n = 0;
  Recs R = recs_at(const_cast<uint8_t*>(recs.data()));
  for (uint64_t r = 0; r < recs.size() / REC_BYTES; ++r)
    n += stubs_only ? load_is_stub(R, r) : R.rlive[r] == REC_LIVE;
  return n;
}
static uint64_t count_keys(const Bytes& recs) {
  uint64_t n = 0;
  Recs R = recs_at(const_cast<uint8_t*>(recs.data()));
  for (uint64_t r = 0; r < recs.size() / REC_BYTES; ++r) n += R.rlive[r] == REC_LIVE && load_holds_key(R, r);
  return n;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream f(argv[1]);
  if (!f) return 2;
  std::vector<Bytes> nodes, fnodes, roots, qkeys;
  std::vector<uint32_t> tries, qtries;
  bool have_fill = false;
  std::string line;
  while (std::getline(f, line)) {
    std::istringstream ss(line);
    std::string tag, a, b;
    ss >> tag >> a >> b;
    if (tag == "N") {
      nodes.push_back(unhex(a));
    } else if (tag == "F") {
      have_fill = true;
      if (a != "-") fnodes.push_back(unhex(a));
    } else if (tag == "T") {
      tries.push_back((uint32_t)strtoul(a.c_str(), nullptr, 10));
      roots.push_back(unhex(b));
      if (roots.back().size() != 32) return 2;
    } else if (tag == "Q") {
      qtries.push_back((uint32_t)strtoul(a.c_str(), nullptr, 10));
      qkeys.push_back(unhex(b));
      if (qkeys.back().size() != 32) return 2;
    }
  }
  const Store st(nodes);
  const Result res = load(st, tries, roots);
  printf("S %llu %u %llu %llu %zu %zu %llu\n", res.code, res.rounds, (unsigned long long)res.rn,
         (unsigned long long)res.keys, res.heap.size(), res.miss.size(), (unsigned long long)res.stubs);
  for (const auto& m : res.miss) {
    printf("M %u ", m.first);
    put_hex(m.second.data(), 32);
    printf("\n");
  }
  Bytes recs = res.recs, heap = res.heap;
  if (res.code == OPEN_OK) {
    Host H(recs, heap);
    if (count_keys(recs) != res.keys || count_live(recs, true) != res.stubs) return 7;
    H.print("");
    for (size_t i = 0; i < qkeys.size(); ++i) {
      uint64_t key[4];
      memcpy(key, qkeys[i].data(), 32);
      const uint32_t r = forest_get(H.M, H.R, qtries[i], key);
      const bool stub = r != NONE && H.R.rdb[r] == EL_STUB;
      std::vector<uint64_t> hits;
      const uint32_t fnd = prove_walk(H.M, H.R, qtries[i], key, [&](uint64_t h) { hits.push_back(h); });
      if (fnd != (r == NONE ? 0u : stub ? 2u : 1u)) return 8;  // the two walks agree
      printf("G %zu %u ", i, fnd);
      if (stub)
        put_hex((const uint8_t*)&H.R.rbref[4ull * r], 32);
      else
        printf("-");
      printf(" %zu", hits.size());
      for (uint64_t h : hits) {
        printf(" ");
        put_hex(exp_hash_of(H.R, h >> 1, (h & 1) ? EXP_LOWER : EXP_UPPER), 32);
      }
      printf("\n");
    }
  }
  const Result again = load(st, tries, roots);
  printf("D %d\n", again.code == res.code && again.rn == res.rn && again.recs == res.recs && again.heap == res.heap);
  if (have_fill && res.code == OPEN_OK) {
    const Store fs(fnodes);
    const Bytes recs0 = recs, heap0 = heap;
    const Result fr = fill(fs, recs, heap);
    if (fr.code != OPEN_OK && (recs != recs0 || heap != heap0)) return 9;  // a failed fill changes nothing
    printf("FS %llu %u %llu %llu %zu %llu %llu\n", fr.code, fr.rounds, (unsigned long long)count_live(recs, false),
           (unsigned long long)count_keys(recs), heap.size(), (unsigned long long)fr.decoded,
           (unsigned long long)count_live(recs, true));
    Host H(recs, heap);
    H.print("F");
  }
  return 0;
}
