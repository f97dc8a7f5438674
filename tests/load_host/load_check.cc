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
#include "../host_common/replay.h"

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
  const Store st(nodes);
  const Result res = load(st, tries, roots, LOAD_FULL);
  printf("S %llu %u %llu %llu %zu %zu\n", res.code, res.rounds, (unsigned long long)res.rn,
         (unsigned long long)res.keys, res.heap.size(), res.miss.size());
  for (const auto& m : res.miss) {
    printf("M %u ", m.first);
    put_hex(m.second.data(), 32);
    printf("\n");
  }
  if (res.code == OPEN_OK) {
    Host H(res.recs, res.heap);
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
  const Result again = load(st, tries, roots, LOAD_FULL);
  printf("D %d\n", again.code == res.code && again.rn == res.rn && again.recs == res.recs && again.heap == res.heap);
  return 0;
}
