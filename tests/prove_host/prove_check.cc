// Host replay of the proof walks (khipu_amd/csrc/prove.h), stand-alone: built with
// g++ -fsanitize=address,undefined by tests/test_prove_host.py and run as a child process.
//
//   prove_check FILE
// FILE, one record a line:
//   P keyhex valuehex     a put (32-byte keys; "-" = the empty value)
//   Q keyhex              a key to prove and then verify under the trie's root
//   V roothex keyhex n enc_1 .. enc_n [idx]
//                         a proof to verify as given (n node encodings; with idx, one path entry
//                         holding that index instead of the n in order)
// The program builds the canonical records of the trie bottom-up (the builder of
// tests/export_host, with export.h's own bodies), then for the Q keys runs the count walk and
// the fill walk of prove.h into arrays of exactly the counted size, encodes every hit through
// export.h's bodies and prints
//   R roothex
//   Q found status valuehex n enc_1 .. enc_n     (status / value: proof_walk over that proof)
// and for every V line
//   V status valuehex
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

#include "../../khipu_amd/csrc/prove.h"

using namespace khst;
typedef std::array<uint8_t, 32> Key;
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
static uint32_t nib(const Key& k, uint32_t i) { return (i & 1) ? (k[i >> 1] & 0xF) : (k[i >> 1] >> 4); }
static void kec(const Bytes& e, uint64_t out[4]) {
  std::vector<uint64_t> w((e.size() + 15) / 8, 0);
  memcpy(w.data(), e.data(), e.size());
  kec256_msg<false>((const uint8_t*)w.data(), (uint32_t)e.size(), out);
}

struct Host {
  uint8_t* recs = nullptr;
  uint8_t* slots = nullptr;
  Bytes heap;
  uint64_t rn = 0, cap = 0;
  Recs R;
  AMap M;
  std::vector<Key> keys;
  std::vector<Bytes> vals;

  void init(uint64_t nkeys) {
    cap = 2 * nkeys + 4;
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
  // one node (sel = EXP_UPPER or EXP_LOWER) of record r through the 16-lane bodies
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
    Bytes out(bytes);  // (exactly the sizes form's bytes: an overrun is ASan's)
    for (uint32_t lane = 0; lane < EXP_LANES; ++lane)
      exp_write(R, heap.data(), r, sel, lane, child[lane], pre[lane], S, out.data(), len);
    if (len[0] + len[1] != bytes) exit(3);
    return out;
  }
  void capped(const Bytes& e, uint64_t ref[4], uint8_t* rl) {
    if (e.size() >= 32) {
      kec(e, ref);
      *rl = 32;
    } else {
      words_of(e.data(), (uint32_t)e.size(), ref);
      *rl = (uint8_t)e.size();
    }
  }
  // records of the subtrie of sorted keys [lo, hi) hanging at depth d
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
    }
    const uint32_t r = (uint32_t)rn++;
    if (rn > cap) exit(4);
    memcpy(R.key(r), keys[lo].data(), 32);
    R.rt[r] = 0;
    R.rd[r] = (uint8_t)d;
    R.rdb[r] = (uint8_t)db;
    R.rmask[r] = (uint16_t)mask;
    R.rlive[r] = REC_LIVE;
    if (db == EL_LEAF) {
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

// proof_walk over a table built from the encodings (buffers of exactly the needed size; the
// encodings padded to a whole word for the hashing)
static uint8_t verify(const uint8_t* root, const uint8_t* key, const std::vector<Bytes>& nodes,
                      const std::vector<uint32_t>& path, Bytes* value) {
  std::vector<uint64_t> off(nodes.size() + 1, 0), hash(4 * nodes.size() + 1);
  Bytes rlp;
  for (size_t j = 0; j < nodes.size(); ++j) {
    rlp.insert(rlp.end(), nodes[j].begin(), nodes[j].end());
    off[j + 1] = rlp.size();
    kec(nodes[j], &hash[4 * j]);
  }
  if (rlp.empty()) rlp.push_back(0);
  const ProofTable T{rlp.data(), off.data(), hash.data(), nodes.size()};
  const uint8_t* val;
  uint32_t vl;
  const uint8_t st = proof_walk(T, root, key, path.data(), path.size(), &val, &vl);
  value->assign(val, val + vl);
  return st;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream f(argv[1]);
  if (!f) return 2;
  std::vector<std::pair<Key, Bytes>> in;
  std::vector<Key> queries;
  std::vector<std::string> vlines;
  std::string line;
  while (std::getline(f, line)) {
    std::istringstream ss(line);
    std::string tag, a, b;
    ss >> tag;
    if (tag == "P" || tag == "Q") {
      ss >> a >> b;
      const Bytes k = unhex(a);
      if (k.size() != 32) return 2;
      Key key;
      memcpy(key.data(), k.data(), 32);
      if (tag == "P")
        in.push_back({key, unhex(b)});
      else
        queries.push_back(key);
    } else if (tag == "V") {
      vlines.push_back(line);
    }
  }
  // later puts win, then sorted
  std::stable_sort(in.begin(), in.end(), [](const auto& x, const auto& y) { return x.first < y.first; });
  Host H;
  for (size_t i = 0; i < in.size(); ++i) {
    if (i + 1 < in.size() && in[i + 1].first == in[i].first) continue;
    H.keys.push_back(in[i].first);
    H.vals.push_back(in[i].second);
  }
  H.init(H.keys.size());
  uint8_t root[32];
  memcpy(root, empty_root_hash(), 32);
  if (!H.keys.empty()) {
    const uint32_t r = H.build(0, H.keys.size(), 0);
    uint64_t h[4];
    kec(H.encode(r, EXP_UPPER), h);  // (the root's hash even when its encoding is short)
    memcpy(root, h, 32);
  }
  printf("R ");
  put_hex(root, 32);
  printf("\n");
  // count walk, scan, fill walk into exactly the counted size
  const size_t nq = queries.size();
  std::vector<uint64_t> pos(nq + 1, 0);
  std::vector<uint8_t> found(nq + 1, 0);
  for (size_t i = 0; i < nq; ++i) {
    uint64_t c = 0;
    found[i] = prove_walk(H.M, H.R, 0, (const uint64_t*)queries[i].data(), [&](uint64_t) { ++c; });
    pos[i + 1] = pos[i] + c;
  }
  uint64_t* hits = new uint64_t[pos[nq]];  // (no slack: a write past the count is ASan's)
  for (size_t i = 0; i < nq; ++i) {
    uint64_t at = pos[i];
    const bool fnd = prove_walk(H.M, H.R, 0, (const uint64_t*)queries[i].data(), [&](uint64_t h) { hits[at++] = h; });
    if (at != pos[i + 1] || fnd != (bool)found[i]) return 6;
  }
  for (size_t i = 0; i < nq; ++i) {
    std::vector<Bytes> nodes;
    std::vector<uint32_t> path;
    for (uint64_t k = pos[i]; k < pos[i + 1]; ++k) {
      path.push_back((uint32_t)nodes.size());
      nodes.push_back(H.encode(hits[k] >> 1, (hits[k] & 1) ? EXP_LOWER : EXP_UPPER));
    }
    Bytes val;
    const uint8_t st = verify(root, queries[i].data(), nodes, path, &val);
    printf("Q %u %u ", (unsigned)found[i], (unsigned)st);
    put_hex(val.data(), val.size());
    printf(" %zu", nodes.size());
    for (const Bytes& e : nodes) {
      printf(" ");
      put_hex(e.data(), e.size());
    }
    printf("\n");
  }
  delete[] hits;
  for (const std::string& vl : vlines) {
    std::istringstream ss(vl);
    std::string tag, rh, kh;
    size_t n;
    ss >> tag >> rh >> kh >> n;
    const Bytes rb = unhex(rh), kb = unhex(kh);
    if (rb.size() != 32 || kb.size() != 32) return 2;
    std::vector<Bytes> nodes;
    std::vector<uint32_t> path;
    for (size_t j = 0; j < n; ++j) {
      std::string e;
      ss >> e;
      nodes.push_back(unhex(e));
      path.push_back((uint32_t)j);
    }
    long idx;
    if (ss >> idx) path.assign(1, (uint32_t)idx);
    Bytes val;
    const uint8_t st = verify(rb.data(), kb.data(), nodes, path, &val);
    printf("V %u ", (unsigned)st);
    put_hex(val.data(), val.size());
    printf("\n");
  }
  free(H.recs);
  free(H.slots);
  return 0;
}
