// Host replay of the range scan (khipu_amd/csrc/range.h), stand-alone: built with
// g++ -fsanitize=address,undefined by tests/test_range_host.py and run as a child process.
//
//   range_check FILE
// FILE, one record a line:
//   P keyhex valuehex     a put (32-byte keys; later puts win)
//   B keyhex valuehex     a put that leaves khipu's value-only branch (forest.h VB_DEPTH): the key
//                         has a sibling sharing 63 nibbles, and its record is the depth-64 branch
//   R originhex limithex max_entries val_cap cut_slack
//                         a range; the frontier is cut at max_entries + cut_slack items (2 is the
//                         library's; 1 shows that the inputs can see the cut)
// The program builds the records of the trie bottom-up (the builder of
// tests/host_common/replay.h, with export.h's own bodies), prints
//   T roothex
// and replays every range through range.h's bodies as range_kernels.hip runs them: count, exclusive
// scan, 16 lanes an item in the fill, into a next frontier of exactly the items it takes (never
// more than the cut), then lengths, 64-bit scan, fit, and a write into outputs of exactly the
// scanned sizes -- a write anywhere else is AddressSanitizer's.  Per range:
//   A page k more nexthex|- rounds key_1 val_1 .. key_k val_k
//   A nospc size
//   A missing hashhex
#include "../host_common/replay.h"

#include "../../khipu_amd/csrc/range.h"

// one range, as kh_trie_range_host runs it (range_kernels.hip range_scan / page_write)
static void range(const Host& H, const Key& origin, const Key& limit, uint64_t max_entries, uint64_t val_cap,
                  uint64_t slack) {
  KeyRange g;
  memcpy(g.o, origin.data(), 32);
  memcpy(g.l, limit.data(), 32);
  const uint64_t me = std::min<uint64_t>(max_entries, std::max<uint64_t>(H.rn, 1));
  const uint64_t F = me + slack;
  std::vector<uint32_t> cur;
  uint32_t rounds = 0;
  if (H.rn && key_cmp(g.o, g.l) <= 0) {
    const uint64_t zero[4] = {0, 0, 0, 0};
    const uint32_t root = map_find(H.M, H.R, 0, 0, zero);
    if (root != NONE) cur.push_back(root);
    while (!cur.empty()) {
      if (rounds > 66) exit(7);
      const uint64_t ni = cur.size();
      uint64_t* pos = new uint64_t[ni];  // (no slack anywhere: an access past an end is ASan's)
      uint64_t total = 0;
      bool expand = false;
      for (uint64_t i = 0; i < ni; ++i) {
        const uint32_t sel = rng_select(H.R, cur[i], g);
        pos[i] = total;
        total += rng_count(sel);
        expand = expand || (sel & 0xFFFFu);
      }
      const uint64_t nn = std::min(total, F);
      uint32_t* nxt = new uint32_t[nn];
      std::fill(nxt, nxt + nn, NONE);
      for (uint64_t i = 0; i < ni; ++i) {
        if (pos[i] >= F) continue;
        for (uint32_t lane = 0; lane < EXP_LANES; ++lane)
          if (!rng_fill_lane(H.R, H.M, cur[i], rng_select(H.R, cur[i], g), lane, pos[i], F, nxt)) exit(8);
      }
      for (uint64_t i = 0; i < nn; ++i)
        if (nxt[i] == NONE) exit(9);  // every place before the cut is filled
      cur.assign(nxt, nxt + nn);
      delete[] nxt;
      delete[] pos;
      ++rounds;
      if (!expand) break;
    }
  }
  const uint64_t ni = cur.size(), n1 = std::min(ni, me + 1), nent = std::min(ni, me);
  if (n1 == 0) {
    printf("A page 0 0 - %u\n", rounds);
    return;
  }
  for (uint64_t i = 0; i < n1; ++i)
    if (rng_is_stub(H.R, cur[i])) {
      printf("A missing ");
      put_hex((const uint8_t*)&H.R.rbref[4ull * cur[i]], 32);
      printf("\n");
      return;
    }
  uint64_t* pos = new uint64_t[nent];
  uint64_t total = 0;
  for (uint64_t i = 0; i < nent; ++i) {
    pos[i] = total;
    total += H.R.rvl[cur[i]];
  }
  unsigned long long fit[2] = {~0ULL, ~0ULL};
  int writers = 0;
  for (uint64_t i = 0; i <= nent; ++i) {  // (one candidate a thread: exactly one of them writes)
    unsigned long long f[2] = {~0ULL, ~0ULL};
    rng_fit(pos, nent, total, val_cap, i, f);
    if (f[0] == ~0ULL) continue;
    ++writers;
    fit[0] = f[0];
    fit[1] = f[1];
  }
  if (writers != 1) exit(10);
  const uint64_t k = fit[0], bytes = fit[1];
  if (k == 0) {
    printf("A nospc %u\n", (unsigned)H.R.rvl[cur[0]]);
    delete[] pos;
    return;
  }
  uint8_t* keys32 = new uint8_t[32 * k];
  uint8_t* vals = new uint8_t[bytes];
  uint64_t* voff = new uint64_t[k + 1];
  for (uint64_t i = 0; i < k; ++i) rng_write(H.R, H.heap.data(), cur[i], i, pos[i], keys32, voff, vals);
  voff[k] = bytes;
  printf("A page %llu %d ", (unsigned long long)k, k < n1 ? 1 : 0);
  if (k < n1)
    put_hex((const uint8_t*)H.R.key(cur[k]), 32);
  else
    printf("-");
  printf(" %u", rounds);
  for (uint64_t i = 0; i < k; ++i) {
    printf(" ");
    put_hex(keys32 + 32 * i, 32);
    printf(" ");
    put_hex(vals + voff[i], voff[i + 1] - voff[i]);
  }
  printf("\n");
  delete[] keys32;
  delete[] vals;
  delete[] voff;
  delete[] pos;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream f(argv[1]);
  if (!f) return 2;
  std::vector<Put> in;
  std::vector<std::string> rlines;
  std::string line;
  while (std::getline(f, line)) {
    std::istringstream ss(line);
    std::string tag, a, b;
    ss >> tag;
    if (tag == "P" || tag == "B") {
      ss >> a >> b;
      const Bytes k = unhex(a);
      if (k.size() != 32) return 2;
      Put p;
      memcpy(p.k.data(), k.data(), 32);
      p.v = unhex(b);
      p.vb = tag == "B";
      in.push_back(p);
    } else if (tag == "R") {
      rlines.push_back(line);
    }
  }
  Builder H(in);
  uint8_t root[32];
  H.root_hash(root);
  printf("T ");
  put_hex(root, 32);
  printf("\n");
  for (const std::string& rl : rlines) {
    std::istringstream ss(rl);
    std::string tag, a, b;
    unsigned long long mx, cap, slack;
    ss >> tag >> a >> b >> mx >> cap >> slack;
    const Bytes ob = unhex(a), lb = unhex(b);
    if (ob.size() != 32 || lb.size() != 32 || !mx) return 2;
    Key o, l;
    memcpy(o.data(), ob.data(), 32);
    memcpy(l.data(), lb.data(), 32);
    range(H, o, l, mx, cap, slack);
  }
  return 0;
}
