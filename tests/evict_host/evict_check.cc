// Host replay of the subtree eviction (khipu_amd/csrc/load.h: evict_probe, evict_covers with its
// predecessor search, evict_stub_record), stand-alone: built with g++ -fsanitize=address,undefined by
// tests/test_evict_host.py and run as a child process.
//
//   evict_check FILE
// FILE, one record a line:
//   N enchex               a node of the store the tries are loaded from (the program hashes it)
//   T id roothex           a listed trie (a PARTIAL load: hashes the store lacks become stubs)
//   P id depth pathhex     a prefix to evict: the first `depth` nibbles of the 32-byte path
// The program loads the tries with the load replay (tests/host_common/replay.h), builds the anchor
// map, and then runs the steps of the library's driver (load_kernels.hip evict_subtrees) through the
// same KH_HD bodies the kernels call, every array of exactly the size the step may touch: the list
// sorted by (trie, zero-padded path), the probe, the DONE prefixes compacted in that order, the flag
// pass over the records, the dead list in record order, their anchors tombstoned, the anchors'
// records rewritten as stubs.  It prints
//   V i status hashhex                  prefix i (input order); hash: 64 hex digits (zero: none)
//   C evicted keys records stubs size   the call's three counters, the live stubs and keys after it
//   B trie a d rrefhex rbrefhex keyhex  every stub afterwards
//   E trie hashhex enchex               every node a node store needs afterwards, per record
//   X 0|1                               1: the listed prefixes are refused (one equals or extends
//                                       another); nothing else is printed
#include "../host_common/replay.h"

struct Prefix {
  uint32_t trie;
  uint8_t depth;
  uint64_t w[4];  // zero past the depth
};

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream f(argv[1]);
  if (!f) return 2;
  std::vector<Bytes> nodes, roots;
  std::vector<uint32_t> tries;
  std::vector<Prefix> pre;
  std::string line;
  while (std::getline(f, line)) {
    std::istringstream ss(line);
    std::string tag, a, b, c;
    ss >> tag >> a >> b >> c;
    if (tag == "N") {
      nodes.push_back(unhex(a));
    } else if (tag == "T") {
      tries.push_back((uint32_t)strtoul(a.c_str(), nullptr, 10));
      roots.push_back(unhex(b));
      if (roots.back().size() != 32) return 2;
    } else if (tag == "P") {
      Prefix p;
      p.trie = (uint32_t)strtoul(a.c_str(), nullptr, 10);
      p.depth = (uint8_t)strtoul(b.c_str(), nullptr, 10);
      const Bytes path = unhex(c);
      if (path.size() != 32 || p.depth == 0 || p.depth > 64) return 2;
      uint64_t w[4];
      words_of(path.data(), 32, w);
      for (int q = 0; q < 4; ++q) p.w[q] = prefix_word(w, p.depth, q);
      pre.push_back(p);
    }
  }
  const Store st(nodes);
  const Result res = load(st, tries, roots, LOAD_PARTIAL);
  if (res.code != OPEN_OK) return 3;
  Host H(res.recs, res.heap);
  const Recs& R = H.R;
  const uint64_t n = pre.size(), rn = H.rn;
  // the list sorted by (trie, zero-padded path, depth); nested prefixes show between neighbours
  std::vector<uint32_t> order(n);
  for (uint64_t i = 0; i < n; ++i) order[i] = (uint32_t)i;
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
    if (pre[a].trie != pre[b].trie) return pre[a].trie < pre[b].trie;
    const int c = key_cmp(pre[a].w, pre[b].w);
    if (c) return c < 0;
    return pre[a].depth != pre[b].depth ? pre[a].depth < pre[b].depth : a < b;
  });
  for (uint64_t s = 0; s + 1 < n; ++s) {
    const Prefix &a = pre[order[s]], &b = pre[order[s + 1]];
    if (a.trie == b.trie && prefix_eq(a.w, b.w, std::min(a.depth, b.depth))) {
      printf("X 1\n");
      return 0;
    }
  }
  printf("X 0\n");
  // the probe, in sorted order
  std::vector<uint8_t> status(n), is_key(n);
  std::vector<uint32_t> rec(n);
  std::vector<uint64_t> hash(4 * n);
  for (uint64_t s = 0; s < n; ++s) {
    const Prefix& p = pre[order[s]];
    status[s] = evict_probe(H.M, R, p.trie, p.depth, p.w, &rec[s], &hash[4 * s], &is_key[s]);
  }
  std::vector<uint64_t> by_input(n);
  for (uint64_t s = 0; s < n; ++s) by_input[order[s]] = s;
  for (uint64_t i = 0; i < n; ++i) {
    printf("V %llu %u ", (unsigned long long)i, (unsigned)status[by_input[i]]);
    put_hex((const uint8_t*)&hash[4 * by_input[i]], 32);
    printf("\n");
  }
  // the DONE prefixes, compacted in sorted order, in arrays of exactly their number
  uint64_t m = 0, keys = 0, stubs_died = 0;
  for (uint64_t s = 0; s < n; ++s) m += status[s] == EVICT_DONE;
  std::vector<uint32_t> et(m), erec(m);
  std::vector<uint64_t> ep(4 * m);
  std::vector<uint8_t> ed(m);
  for (uint64_t s = 0, t = 0; s < n; ++s) {
    if (status[s] != EVICT_DONE) continue;
    et[t] = pre[order[s]].trie;
    ed[t] = pre[order[s]].depth;
    erec[t] = rec[s];
    memcpy(&ep[4 * t], pre[order[s]].w, 32);
    keys += is_key[s];
    ++t;
  }
  const EvictList E{et.data(), ep.data(), ed.data(), m};
  // the flag pass, the dead list in record order, the delete, the stubs
  std::vector<uint32_t> flag(rn), list;
  if (m) {
    for (uint64_t r = 0; r < rn; ++r) {
      flag[r] = evict_covers(R, r, E) ? 1u : 0u;
      if (!flag[r]) continue;
      keys += load_holds_key(R, r);
      stubs_died += R.rdb[r] == EL_STUB;
      list.push_back((uint32_t)r);
    }
    for (uint32_t r : list) {
      const uint64_t sl = map_slot_of(H.M, R, r);
      if (sl == ~0ULL) return 7;  // a live record has its anchor
      H.M.tag[sl] = 1;
      R.rlive[r] = REC_DEAD;
    }
    for (uint64_t t = 0; t < m; ++t) evict_stub_record(R, erec[t], ed[t]);
  }
  // the map afterwards: every live record is found at its anchor, no dead one is
  uint64_t live_stubs = 0, size = 0;
  for (uint64_t r = 0; r < rn; ++r) {
    const uint32_t at = map_find(H.M, R, R.rt[r], R.rd[r], R.key(r));
    if (R.rlive[r] == REC_LIVE ? at != r : at == r) return 8;
    live_stubs += load_is_stub(R, r);
    size += R.rlive[r] == REC_LIVE && load_holds_key(R, r);
  }
  if (live_stubs != res.stubs + m - stubs_died || size != res.keys - keys) return 9;
  printf("C %llu %llu %zu %llu %llu\n", (unsigned long long)m, (unsigned long long)keys, list.size(),
         (unsigned long long)live_stubs, (unsigned long long)size);
  for (uint64_t r = 0; r < rn; ++r) {
    if (load_is_stub(R, r)) {
      printf("B %u %u %u ", R.rt[r], (unsigned)R.rd[r], (unsigned)(R.rmask[r] & 0xFF));
      put_hex((const uint8_t*)&R.rref[4 * r], R.rrl[r]);
      printf(" ");
      put_hex((const uint8_t*)&R.rbref[4 * r], R.rbrl[r]);
      printf(" ");
      put_hex((const uint8_t*)R.key(r), 32);
      printf("\n");
    }
    const uint32_t sel = exp_select(R, r, EXP_ALL_TRIES);
    for (uint32_t which : {EXP_UPPER, EXP_LOWER}) {
      if (!(sel & which)) continue;
      const Bytes e = H.encode(r, which);
      printf("E %u ", R.rt[r]);
      put_hex(exp_hash_of(R, r, which), 32);
      printf(" ");
      put_hex(e.data(), e.size());
      printf("\n");
    }
  }
  return 0;
}
