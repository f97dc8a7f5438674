// Host replay of the forest load (khipu_amd/csrc/load.h), stand-alone: built with
// g++ -fsanitize=address,undefined by tests/test_load_host.py and run as a child process.
//
//   load_check FILE
// FILE, one record a line:
//   N enchex          a node of the store (content addressed: the program hashes it)
//   T id roothex      a listed trie
// The program sorts the store's hashes, then replays the rounds of load.h as the library runs
// them -- count every frontier item, scan, stop on an error or a missing node, fill -- into
// arrays of exactly the scanned sizes (a write past one is AddressSanitizer's), builds an anchor
// map over the records, re-encodes every record's nodes through export.h and prints
//   S code rounds records keys heap_bytes n_missing     (code: an OPEN_* value; 0 = loaded)
//   M idx hashhex                                        every missing reference of the last round
//   E trie hashhex enchex                                every node a node store needs, per record
//   D 0|1                                                a second replay gave identical arrays
// After a failed load the records and the heap hold nothing (the library clears what the earlier
// rounds wrote): the counts printed are 0 then.
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

struct Result {
  unsigned long long code = OPEN_OK;
  uint32_t rounds = 0;
  uint64_t rn = 0, keys = 0;
  Bytes recs, heap;  // exactly rn records / the value bytes
  std::vector<std::pair<uint32_t, std::array<uint8_t, 32>>> miss;
};

struct Store {
  Bytes enc;  // packed (+ 8 bytes of slack for word reads)
  std::vector<uint64_t> off, hash;
  std::vector<uint32_t> idx;
  NStore view() const { return NStore{hash.data(), idx.data(), idx.size(), enc.data(), off.data()}; }
};

static Result replay(const Store& st, const std::vector<uint32_t>& tries, const std::vector<Bytes>& roots) {
  Result res;
  const NStore S = st.view();
  // round 0: the roots that are not the empty trie's, in list order
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
  for (; ni && res.rounds < 80; ++res.rounds) {
    std::vector<uint32_t> child(ni), rec(ni), miss(ni), src(ni);
    std::vector<uint64_t> val(ni);
    LCounts C{child.data(), rec.data(), val.data(), miss.data(), src.data()};
    unsigned long long code = OPEN_OK;
    uint64_t nmiss = 0;
    for (uint64_t i = 0; i < ni; ++i) {
      uint32_t is_key = 0;
      const unsigned long long c = load_count_item(cur->I, i, S, C, &is_key);
      if (c == OPEN_MISSING)
        ++nmiss;
      else if (c != OPEN_OK)
        code = std::max(code, c);
      res.keys += is_key;
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
      res.rn = res.keys = 0;  // all or nothing: what the earlier rounds wrote is cleared
      res.recs.clear();
      res.heap.clear();
      delete cur;
      return res;
    }
    // fill into exactly the scanned sizes: the round's records and values in allocations of
    // their own, appended to the result afterwards
    uint8_t* rr = (uint8_t*)aligned_alloc(128, std::max<uint64_t>(nrec, 1) * REC_BYTES);
    memset(rr, 0, std::max<uint64_t>(nrec, 1) * REC_BYTES);
    uint8_t* hh = new uint8_t[nval];
    Frontier* nxt = new Frontier(nchild);
    for (uint64_t i = 0; i < ni; ++i)
      load_fill_item(cur->I, i, S, C, nxt->I, tries.data(), rr, 0, nrec, hh, 0, nval);
    // (the value offsets of this round's records are relative to the round: rebase them)
    Recs R = recs_at(rr);
    for (uint64_t r = 0; r < nrec; ++r)
      if (R.rvl[r]) R.rvo[r] += res.heap.size();
    res.recs.insert(res.recs.end(), rr, rr + nrec * REC_BYTES);
    res.heap.insert(res.heap.end(), hh, hh + nval);
    res.rn += nrec;
    free(rr);
    delete[] hh;
    delete cur;
    cur = nxt;
    ni = nchild;
  }
  delete cur;
  if (ni) res.code = OPEN_BAD;
  return res;
}

// the records with an anchor map over them, and export.h's 16-lane bodies
struct Host {
  uint8_t* recs = nullptr;
  uint8_t* slots = nullptr;
  Bytes heap;
  Recs R;
  AMap M;
  Host(const Result& res) {
    const uint64_t n = std::max<uint64_t>(res.rn, 1);
    recs = (uint8_t*)aligned_alloc(128, n * REC_BYTES);
    memcpy(recs, res.recs.data(), res.rn * REC_BYTES);
    uint64_t mc = 16;
    while (mc < 4 * n) mc <<= 1;
    slots = (uint8_t*)aligned_alloc(128, mc * 16);
    memset(slots, 0, mc * 16);
    heap = res.heap;
    heap.resize(heap.size() + 8);
    R = recs_at(recs);
    M = AMap{{slots}, {slots}, mc - 1};
    for (uint32_t r = 0; r < res.rn; ++r) {
      const uint64_t tag = anchor_tag(R.rt[r], R.rd[r], R.key(r));
      uint64_t s = tag & M.mask;
      while (M.tag[s]) s = (s + 1) & M.mask;
      M.tag[s] = tag;
      M.rec[s] = r;
    }
  }
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
};

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream f(argv[1]);
  if (!f) return 2;
  std::vector<Bytes> nodes, roots;
  std::vector<uint32_t> tries;
  std::string line;
  while (std::getline(f, line)) {
    std::istringstream ss(line);
    std::string tag, a, b;
    ss >> tag >> a >> b;
    if (tag == "N") {
      nodes.push_back(unhex(a));
    } else if (tag == "T") {
      tries.push_back((uint32_t)strtoul(a.c_str(), nullptr, 10));
      roots.push_back(unhex(b));
      if (roots.back().size() != 32) return 2;
    }
  }
  // the store: packed encodings, their hashes sorted (equal hashes: one entry, as the library's
  // sort keeps one of equal keys)
  Store st;
  st.off.push_back(0);
  std::vector<std::array<uint64_t, 4>> hs(nodes.size());
  for (size_t i = 0; i < nodes.size(); ++i) {
    st.enc.insert(st.enc.end(), nodes[i].begin(), nodes[i].end());
    st.off.push_back(st.enc.size());
    kec(nodes[i], hs[i].data());
  }
  st.enc.resize(st.enc.size() + 8);
  std::vector<uint32_t> order(nodes.size());
  for (size_t i = 0; i < order.size(); ++i) order[i] = (uint32_t)i;
  std::stable_sort(order.begin(), order.end(),
                   [&](uint32_t x, uint32_t y) { return key_cmp(hs[x].data(), hs[y].data()) < 0; });
  for (size_t i = 0; i < order.size(); ++i) {
    if (i && key_cmp(hs[order[i]].data(), hs[order[i - 1]].data()) == 0) continue;
    st.idx.push_back(order[i]);
    st.hash.insert(st.hash.end(), hs[order[i]].begin(), hs[order[i]].end());
  }
  const Result res = replay(st, tries, roots);
  printf("S %llu %u %llu %llu %zu %zu\n", res.code, res.rounds, (unsigned long long)res.rn,
         (unsigned long long)res.keys, res.heap.size(), res.miss.size());
  for (const auto& m : res.miss) {
    printf("M %u ", m.first);
    put_hex(m.second.data(), 32);
    printf("\n");
  }
  if (res.code == OPEN_OK) {
    Host H(res);
    for (uint64_t r = 0; r < res.rn; ++r) {
      const uint32_t sel = exp_select(H.R, r, EXP_ALL_TRIES);
      for (uint32_t which : {EXP_UPPER, EXP_LOWER}) {
        if (!(sel & which)) continue;
        const Bytes e = H.encode(r, which);
        printf("E %u ", H.R.rt[r]);
        put_hex(exp_hash_of(H.R, r, which), 32);
        printf(" ");
        put_hex(e.data(), e.size());
        printf("\n");
      }
    }
  }
  const Result again = replay(st, tries, roots);
  printf("D %d\n", again.code == res.code && again.rn == res.rn && again.recs == res.recs && again.heap == res.heap);
  return 0;
}
