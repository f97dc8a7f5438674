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
#include "../host_common/replay.h"

#include "../../khipu_amd/csrc/prove.h"

// every stub of H (B lines) and every node a node store needs, per record (E lines)
static void print(Host& H, const char* pfx) {
  const Recs& R = H.R;
  for (uint64_t r = 0; r < H.rn; ++r) {
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
      const Bytes e = H.encode(r, which);
      printf("%sE %u ", pfx, R.rt[r]);
      put_hex(exp_hash_of(R, r, which), 32);
      printf(" ");
      put_hex(e.data(), e.size());
      printf("\n");
    }
  }
}

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
  rounds(st, cur, list.size(), tries, LOAD_FILL, heap.size(), res);
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
  const Result res = load(st, tries, roots, LOAD_PARTIAL);
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
    print(H, "");
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
  const Result again = load(st, tries, roots, LOAD_PARTIAL);
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
    print(H, "F");
  }
  return 0;
}
