// Host replay of the commit witness (khipu_amd/csrc/witness.h), stand-alone: built with
// g++ -fsanitize=address,undefined by tests/test_witness_host.py and run as a child process.
//
//   witness_check FILE
// FILE, one record a line:
//   N enchex          a node of the store the tries are loaded from (the program hashes it)
//   T id roothex      a listed trie
//   U id keyhex       an upsert of a 32-byte trie key (the upserts come first, in file order)
//   D id keyhex       a delete
// The records are those of load.h's rounds over the store (a PARTIAL load: a hash the store lacks
// below a root is a stub).  The program then runs the driver's passes over the KH_HD bodies, every
// array of exactly the size the library gives it (a write past one is AddressSanitizer's): the
// deletes into their set, the count walk, the fill walk into the visited set, the visited branches
// binned by depth and judged deepest first.  It prints
//   S code                       the load's OPEN_* value (0 = loaded)
//   R trie hashhex               a stub an op's walk reaches (each once)
//   M trie hashhex               a stub of unknown kind a collapse would move
//   W trie hashhex               every node of the witness once, in table order (no R line only)
//   C n_collapse n_hits n_visits the collapse children, the walks' hits and visits
#include "../host_common/replay.h"

#include "../../khipu_amd/csrc/witness.h"

static uint64_t pow2_at_least(uint64_t v) {
  uint64_t p = 16;
  while (p < v) p <<= 1;
  return p;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream f(argv[1]);
  if (!f) return 2;
  std::vector<Bytes> nodes, roots;
  std::vector<uint32_t> tries;
  std::vector<std::pair<uint32_t, Bytes>> ups, dels;
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
    } else if (tag == "U" || tag == "D") {
      (tag == "U" ? ups : dels).push_back({(uint32_t)strtoul(a.c_str(), nullptr, 10), unhex(b)});
      if (unhex(b).size() != 32) return 2;
    }
  }
  const Store st(nodes);
  const Result res = load(st, tries, roots, LOAD_PARTIAL);
  printf("S %llu\n", res.code);
  if (res.code != OPEN_OK) return 0;
  Host H(res.recs, res.heap);
  const Recs& R = H.R;
  const AMap& M = H.M;
  // the ops: upserts [0, nup), deletes [nup, n)
  const uint64_t nup = ups.size(), n = nup + dels.size();
  std::vector<uint64_t> K(4 * n);
  std::vector<uint32_t> T(n);
  for (uint64_t i = 0; i < n; ++i) {
    const auto& op = i < nup ? ups[i] : dels[i - nup];
    T[i] = op.first;
    memcpy(&K[4 * i], op.second.data(), 32);
  }
  const bool join = nup && n > nup;
  std::vector<uint32_t> didx(join ? pow2_at_least(2 * (n - nup)) : 0, NONE);
  WDels D{didx.data(), didx.empty() ? 0 : didx.size() - 1};
  for (uint64_t i = nup; join && i < n; ++i) wdels_insert(D, K.data(), T.data(), i);
  // count
  std::vector<uint64_t> pos(n + 1, 0);
  uint64_t nv = 0;
  for (uint64_t i = 0; i < n; ++i) {
    uint64_t c = 0;
    if (H.rn) wit_walk(M, R, T[i], &K[4 * i], [&](uint64_t) { ++c; }, [&](uint32_t, uint32_t) { ++nv; });
    pos[i + 1] = pos[i] + c;
  }
  const uint64_t np = pos[n];
  // fill
  const uint64_t vcap = pow2_at_least(2 * nv);
  std::vector<uint32_t> vrec(vcap, NONE), vst(vcap, 0), vmk(vcap, 0);
  WSet V{vrec.data(), vst.data(), vmk.data(), vcap - 1};
  std::vector<uint64_t> hits(np + nv);
  std::vector<uint32_t> reached, moved;
  for (uint64_t i = 0; i < n && H.rn; ++i) {
    const bool del = i >= nup;
    const bool up = !del && !(join && wdels_has(D, K.data(), T.data(), T[i], &K[4 * i]));
    uint64_t at = pos[i];
    wit_op(
        M, R, V, T[i], &K[4 * i], up, del,
        [&](uint64_t h) {
          if (at >= pos[i + 1]) exit(7);  // the fill walk lists what the count walk counted
          hits[at++] = h;
        },
        [&](uint32_t r) { reached.push_back(r); });
    if (at != pos[i + 1]) return 7;
  }
  for (uint32_t r : reached) {
    printf("R %u ", R.rt[r]);
    put_hex((const uint8_t*)&R.rbref[4ull * r], 32);
    printf("\n");
  }
  // the visited branches by depth, deepest first
  std::vector<std::vector<uint32_t>> bins(64);
  uint64_t seen = 0;
  for (uint64_t s = 0; s < vcap; ++s) {
    if (vrec[s] == NONE) continue;
    ++seen;
    if (wit_is_branch(R, vrec[s])) bins[R.rdb[vrec[s]]].push_back((uint32_t)s);
  }
  if (seen > nv) return 8;  // (the distinct visited records are no more than the visits)
  uint64_t ncol = 0;
  for (int d = 63; d >= 0 && reached.empty(); --d)
    for (uint32_t s : bins[d])
      wit_eval(
          M, R, V, s,
          [&](uint64_t h) {
            if (np + ncol >= hits.size()) exit(9);
            hits[np + ncol++] = h;
          },
          [&](uint32_t r) { moved.push_back(r); });
  for (uint32_t r : moved) {
    printf("M %u ", R.rt[r]);
    put_hex((const uint8_t*)&R.rbref[4ull * r], 32);
    printf("\n");
  }
  if (reached.empty() && moved.empty()) {
    std::vector<uint64_t> all(hits.begin(), hits.begin() + np + ncol);
    std::sort(all.begin(), all.end());
    const uint64_t nall = std::unique(all.begin(), all.end()) - all.begin();
    std::vector<uint64_t> paths(hits.begin(), hits.begin() + np);
    std::sort(paths.begin(), paths.end());
    const uint64_t npaths = std::unique(paths.begin(), paths.end()) - paths.begin();
    if (nall != npaths + ncol) return 10;  // a collapse child is never on a path, and listed once
    for (uint64_t j = 0; j < nall; ++j) {
      printf("W %u ", R.rt[all[j] >> 1]);
      put_hex(exp_hash_of(R, all[j] >> 1, (all[j] & 1) ? EXP_LOWER : EXP_UPPER), 32);
      printf("\n");
    }
  }
  printf("C %llu %llu %llu\n", (unsigned long long)ncol, (unsigned long long)np, (unsigned long long)nv);
  return 0;
}
