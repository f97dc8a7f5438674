// Host replay of the trie diff (khipu_amd/csrc/diff.h), stand-alone: built with
// g++ -fsanitize=address,undefined by tests/test_diff_host.py and run as a child process.
//
//   diff_check FILE
// FILE, one record a line:
//   PA keyhex valuehex    a put into side a (32-byte keys; later puts win);  PB: into side b
//   BA keyhex valuehex    a put that leaves khipu's value-only branch (forest.h VB_DEPTH): the key
//                         has a sibling sharing 63 nibbles, and its record is the depth-64 branch;  BB
//   D originhex limithex max_entries val_cap cut_slack late_skip
//                         a diff; the frontier is cut at max_entries + cut_slack items (2 is the
//                         library's; 1 shows that the inputs can see the cut); late_skip = 1 makes
//                         the skip test after the cut instead of before it (0 is the library's)
// The program builds the records of both tries bottom-up (the builder of tests/host_common/replay.h,
// with export.h's own bodies), prints
//   T roothex_a roothex_b
// and replays every diff through diff.h's bodies as range_kernels.hip runs them: the root pair, then
// per round select (16 lanes an item), exclusive scan, 16 lanes an item in the fill, into a next
// frontier of exactly the items it takes (never more than the cut), then lengths, 64-bit scan, fit,
// and a write into outputs of exactly the scanned sizes -- a write anywhere else is
// AddressSanitizer's.  Per diff:
//   A page k more nexthex|- rounds visited key_1 kind_1 val_1 .. key_k kind_k val_k
//   A nospc size
//   A missing hashhex
#include "../host_common/replay.h"

#include "../../khipu_amd/csrc/diff.h"

struct Item {
  uint32_t a, b, d;
};

static void diff(const Host& HA, const Host& HB, const Key& origin, const Key& limit, uint64_t max_entries,
                 uint64_t val_cap, uint64_t slack, bool late_skip) {
  KeyRange g;
  memcpy(g.o, origin.data(), 32);
  memcpy(g.l, limit.data(), 32);
  const DSide A{HA.R, HA.M, HA.heap.data()}, B{HB.R, HB.M, HB.heap.data()};
  const uint64_t me = std::min<uint64_t>(max_entries, std::max<uint64_t>(HA.rn + HB.rn, 1));
  const uint64_t F = me + slack;
  std::vector<Item> cur;
  uint32_t rounds = 0;
  uint64_t visited = 0;
  if ((HA.rn || HB.rn) && key_cmp(g.o, g.l) <= 0) {
    const uint64_t zero[4] = {0, 0, 0, 0};
    const uint32_t ra = HA.rn ? map_find(HA.M, HA.R, 0, 0, zero) : NONE;
    const uint32_t rb = HB.rn ? map_find(HB.M, HB.R, 0, 0, zero) : NONE;
    if (!((ra == NONE && rb == NONE) || df_skip(A, ra, B, rb, 0))) cur.push_back(Item{ra, rb, 0});
    while (!cur.empty()) {
      if (rounds > 68) exit(7);
      const uint64_t ni = cur.size();
      visited += ni;
      uint32_t* sel = new uint32_t[ni];  // (no slack anywhere: an access past an end is ASan's)
      uint64_t* pos = new uint64_t[ni];
      uint64_t total = 0;
      bool expand = false;
      for (uint64_t i = 0; i < ni; ++i) {
        const uint32_t plan = df_plan(A, cur[i].a, B, cur[i].b, g);
        uint32_t kids = 0;
        for (uint32_t lane = 0; lane < EXP_LANES; ++lane) {
          const bool alive = late_skip ? ((plan >> lane) & 1) != 0 : df_lane_alive(A, cur[i].a, B, cur[i].b, plan, lane);
          kids |= (alive ? 1u : 0u) << lane;
        }
        sel[i] = (plan & ~0xFFFFu) | kids;
        pos[i] = total;
        total += df_count(sel[i]);
        expand = expand || df_expands(sel[i]);
      }
      const uint64_t nn = std::min(total, F);
      uint32_t *oa = new uint32_t[nn], *ob = new uint32_t[nn], *od = new uint32_t[nn];
      std::fill(od, od + nn, 0xFFFFFFFFu);
      for (uint64_t i = 0; i < ni; ++i) {
        if (pos[i] >= F) continue;
        for (uint32_t lane = 0; lane < EXP_LANES; ++lane)
          if (!df_fill_lane(A, cur[i].a, B, cur[i].b, cur[i].d, sel[i], lane, pos[i], F, oa, ob, od)) exit(8);
      }
      std::vector<Item> nxt;
      for (uint64_t i = 0; i < nn; ++i) {
        if (od[i] == 0xFFFFFFFFu) exit(9);  // every place before the cut is filled
        if (late_skip && df_skip(A, oa[i], B, ob[i], od[i])) continue;
        nxt.push_back(Item{oa[i], ob[i], od[i]});
      }
      cur.swap(nxt);
      delete[] oa;
      delete[] ob;
      delete[] od;
      delete[] sel;
      delete[] pos;
      ++rounds;
      if (!expand) break;
    }
  }
  const uint64_t ni = cur.size(), n1 = std::min(ni, me + 1), nent = std::min(ni, me);
  if (n1 == 0) {
    printf("A page 0 0 - %u %llu\n", rounds, (unsigned long long)visited);
    return;
  }
  for (uint64_t i = 0; i < n1; ++i)
    if (df_missing(A, cur[i].a, B, cur[i].b)) {
      const bool of_a = cur[i].a != NONE && df_stub(A.R, cur[i].a);
      printf("A missing ");
      put_hex(of_a ? (const uint8_t*)&A.R.rbref[4ull * cur[i].a] : (const uint8_t*)&B.R.rbref[4ull * cur[i].b], 32);
      printf("\n");
      return;
    }
  uint64_t* pos = new uint64_t[nent];
  uint64_t total = 0;
  for (uint64_t i = 0; i < nent; ++i) {
    pos[i] = total;
    total += df_len(A, cur[i].a, B, cur[i].b);
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
    printf("A nospc %llu\n", (unsigned long long)df_len(A, cur[0].a, B, cur[0].b));
    delete[] pos;
    return;
  }
  uint8_t* keys32 = new uint8_t[32 * k];
  uint8_t* kinds = new uint8_t[k];
  uint8_t* vals = new uint8_t[bytes];
  uint64_t* voff = new uint64_t[k + 1];
  for (uint64_t i = 0; i < k; ++i) df_write(A, cur[i].a, B, cur[i].b, i, pos[i], keys32, kinds, voff, vals);
  voff[k] = bytes;
  printf("A page %llu %d ", (unsigned long long)k, k < n1 ? 1 : 0);
  if (k < n1)
    put_hex((const uint8_t*)df_key(A, cur[k].a, B, cur[k].b), 32);
  else
    printf("-");
  printf(" %u %llu", rounds, (unsigned long long)visited);
  for (uint64_t i = 0; i < k; ++i) {
    printf(" ");
    put_hex(keys32 + 32 * i, 32);
    printf(" %u ", (unsigned)kinds[i]);
    put_hex(vals + voff[i], voff[i + 1] - voff[i]);
  }
  printf("\n");
  delete[] keys32;
  delete[] kinds;
  delete[] vals;
  delete[] voff;
  delete[] pos;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream f(argv[1]);
  if (!f) return 2;
  std::vector<Put> in[2];
  std::vector<std::string> dlines;
  std::string line;
  while (std::getline(f, line)) {
    std::istringstream ss(line);
    std::string tag, a, b;
    ss >> tag;
    if (tag == "PA" || tag == "BA" || tag == "PB" || tag == "BB") {
      ss >> a >> b;
      const Bytes k = unhex(a);
      if (k.size() != 32) return 2;
      Put p;
      memcpy(p.k.data(), k.data(), 32);
      p.v = unhex(b);
      p.vb = tag[0] == 'B';
      in[tag[1] == 'B'].push_back(p);
    } else if (tag == "D") {
      dlines.push_back(line);
    }
  }
  Builder HA(in[0]), HB(in[1]);
  uint8_t root[32];
  printf("T ");
  HA.root_hash(root);
  put_hex(root, 32);
  printf(" ");
  HB.root_hash(root);
  put_hex(root, 32);
  printf("\n");
  for (const std::string& dl : dlines) {
    std::istringstream ss(dl);
    std::string tag, a, b;
    unsigned long long mx, cap, slack, late;
    ss >> tag >> a >> b >> mx >> cap >> slack >> late;
    const Bytes ob = unhex(a), lb = unhex(b);
    if (ob.size() != 32 || lb.size() != 32 || !mx) return 2;
    Key o, l;
    memcpy(o.data(), ob.data(), 32);
    memcpy(l.data(), lb.data(), 32);
    diff(HA, HB, o, l, mx, cap, slack, late != 0);
  }
  return 0;
}
