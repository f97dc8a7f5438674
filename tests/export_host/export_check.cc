// Host replay of the record -> node encoder (khipu_amd/csrc/export.h), stand-alone: built with
// g++ -fsanitize=address,undefined by tests/test_export_host.py and run as a child process.
//
//   export_check FILE [flip]
// FILE: one "keyhex valuehex" line per put (32-byte keys; "-" = the empty value).  The program
// builds the canonical records of that trie bottom-up -- each node's encoding made by export.h's
// own write bodies and hashed by keccak.h's host path to fill ref / bref -- inserts the anchors
// (anchor_tag, linear probing), then runs the sizes and write bodies over all records the way
// the kernels do (16 lanes a record, replayed by loops; a prefix sum between the passes) into
// buffers of exactly the scanned size, verifies every node, and prints "hash enc" lines and a
// last line "verify_bad N".  With `flip`, one byte of one record's ref is flipped before the run.
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../khipu_amd/csrc/export.h"

using namespace khst;
typedef std::array<uint8_t, 32> Key;

static std::vector<uint8_t> unhex(const std::string& s) {
  std::vector<uint8_t> o;
  if (s == "-") return o;
  for (size_t i = 0; i + 1 < s.size(); i += 2) o.push_back((uint8_t)strtoul(s.substr(i, 2).c_str(), nullptr, 16));
  return o;
}
static void put_hex(const uint8_t* p, size_t n) {
  for (size_t i = 0; i < n; ++i) printf("%02x", p[i]);
}
static uint32_t nib(const Key& k, uint32_t i) { return (i & 1) ? (k[i >> 1] & 0xF) : (k[i >> 1] >> 4); }

struct Host {
  uint8_t* recs = nullptr;
  uint8_t* slots = nullptr;
  std::vector<uint8_t> heap;
  uint64_t rn = 0, cap = 0;
  Recs R;
  AMap M;
  std::vector<Key> keys;
  std::vector<std::vector<uint8_t>> vals;

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
  // the selected nodes of record r through the 16-lane bodies; returns the bytes, len[2] the split
  std::vector<uint8_t> encode(uint64_t r, uint32_t sel, uint32_t len[2], uint32_t* size_bytes = nullptr,
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
    std::vector<uint8_t> out(bytes);  // (exactly the sizes form's bytes: an overrun is ASan's)
    for (uint32_t lane = 0; lane < EXP_LANES; ++lane)
      exp_write(R, heap.data(), r, sel, lane, child[lane], pre[lane], S, out.data(), len);
    if (len[0] + len[1] != bytes) {
      fprintf(stderr, "sizes form %u != write form %u + %u (record %llu)\n", bytes, len[0], len[1],
              (unsigned long long)r);
      exit(3);
    }
    return out;
  }
  // capped reference of an encoding
  void capped(const std::vector<uint8_t>& e, uint64_t ref[4], uint8_t* rl) {
    if (e.size() >= 32) {
      std::vector<uint64_t> w((e.size() + 15) / 8, 0);
      memcpy(w.data(), e.data(), e.size());
      kec256_msg<false>((const uint8_t*)w.data(), (uint32_t)e.size(), ref);
      *rl = 32;
    } else {
      words_of(e.data(), (uint32_t)e.size(), ref);
      *rl = (uint8_t)e.size();
    }
  }
  // records of the subtrie of sorted keys [lo, hi) hanging at depth d; returns its record
  uint32_t build(size_t lo, size_t hi, uint32_t d) {
    uint32_t db = EL_LEAF;
    std::vector<std::pair<size_t, size_t>> kids(16, {0, 0});
    uint32_t mask = 0;
    if (hi - lo > 1) {
      db = d;
      while (nib(keys[lo], db) == nib(keys[hi - 1], db)) ++db;
      for (size_t i = lo; i < hi;) {
        const uint32_t c = nib(keys[i], db);
        size_t j = i;
        while (j < hi && nib(keys[j], db) == c) ++j;
        kids[c] = {i, j};
        mask |= 1u << c;
        i = j;
      }
      for (uint32_t c = 0; c < 16; ++c)
        if (mask >> c & 1) build(kids[c].first, kids[c].second, db + 1);
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
    uint32_t len[2];
    uint64_t ref[4];
    uint8_t rl;
    if (exp_has_lower(d, db)) {  // the branch first, then the extension that refers to it
      capped(encode(r, EXP_LOWER, len), ref, &rl);
      for (int q = 0; q < 4; ++q) R.rbref[4ull * r + q] = ref[q];
      R.rbrl[r] = rl;
    }
    capped(encode(r, EXP_UPPER, len), ref, &rl);
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

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const bool flip = argc > 2 && !strcmp(argv[2], "flip");
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  std::vector<std::pair<Key, std::vector<uint8_t>>> in;
  char kb[128], vb[8192];
  while (fscanf(f, "%127s %8191s", kb, vb) == 2) {
    const std::vector<uint8_t> k = unhex(kb);
    if (k.size() != 32) return 2;
    Key key;
    memcpy(key.data(), k.data(), 32);
    in.push_back({key, unhex(vb)});
  }
  fclose(f);
  // later puts win, then sorted
  std::stable_sort(in.begin(), in.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
  Host H;
  for (size_t i = 0; i < in.size(); ++i) {
    if (i + 1 < in.size() && in[i + 1].first == in[i].first) continue;
    H.keys.push_back(in[i].first);
    H.vals.push_back(in[i].second);
  }
  H.init(H.keys.size());
  if (!H.keys.empty()) H.build(0, H.keys.size(), 0);
  if (flip) {
    for (uint64_t r = 0; r < H.rn; ++r)
      if (H.R.rrl[r] == 32) {
        ((uint8_t*)&H.R.rref[4 * r])[7] ^= 0x10;
        break;
      }
  }
  // pass 1: sizes of every record (the kernels' selection), then the scans
  const uint64_t n = H.rn;
  std::vector<uint32_t> cnt(n + 1, 0), byt(n + 1, 0);
  uint32_t len[2];
  for (uint64_t r = 0; r < n; ++r) {
    const uint32_t sel = exp_select(H.R, r, EXP_ALL_TRIES);
    if (sel) H.encode(r, sel, len, &byt[r], &cnt[r]);
  }
  uint64_t tn = 0, tb = 0;
  std::vector<uint64_t> cpos(n), bpos(n);
  for (uint64_t r = 0; r < n; ++r) {
    cpos[r] = tn;
    bpos[r] = tb;
    tn += cnt[r];
    tb += byt[r];
  }
  // pass 2: write into buffers of exactly that size (the encodings padded to a whole word)
  std::vector<uint8_t> hashes(tn * 32);
  std::vector<uint64_t> off(tn + 1), rlpw((tb + 7) / 8 + 1, 0);
  uint8_t* rlp = (uint8_t*)rlpw.data();
  for (uint64_t r = 0; r < n; ++r) {
    const uint32_t sel = exp_select(H.R, r, EXP_ALL_TRIES);
    if (!sel) continue;
    const std::vector<uint8_t> e = H.encode(r, sel, len);
    if (bpos[r] + e.size() > tb) return 5;
    memcpy(rlp + bpos[r], e.data(), e.size());
    uint64_t slot = cpos[r], at = bpos[r];
    for (uint32_t w = 0; w < 2; ++w) {
      if (!len[w]) continue;
      memcpy(&hashes[32 * slot], exp_hash_of(H.R, r, w ? EXP_LOWER : EXP_UPPER), 32);
      off[slot++] = at;
      at += len[w];
    }
  }
  off[tn] = tb;
  uint64_t bad = 0;
  for (uint64_t j = 0; j < tn; ++j) {
    bad += exp_verify(hashes.data(), rlp, off.data(), j) ? 1 : 0;
    put_hex(&hashes[32 * j], 32);
    printf(" ");
    put_hex(rlp + off[j], off[j + 1] - off[j]);
    printf("\n");
  }
  printf("verify_bad %llu\n", (unsigned long long)bad);
  free(H.recs);
  free(H.slots);
  return 0;
}
