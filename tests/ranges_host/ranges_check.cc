// Host replay of the batched range scan (khipu_amd/csrc/range.h "MANY RANGES A CALL"), stand-alone:
// built with g++ -fsanitize=address,undefined by tests/test_ranges_host.py and run as a child
// process.
//
//   ranges_check FILE
// FILE, one record a line:
//   T id                  the puts that follow belong to trie `id` of the forest
//   P keyhex valuehex     a put (32-byte keys; later puts win)
//   B keyhex valuehex     a put that leaves khipu's value-only branch (forest.h VB_DEPTH)
//   Q max_entries val_cap cut_less
//                         a batch: the requests that follow, answered under one budget; the
//                         frontiers are cut at max_entries + 2 * nq - cut_less items (0 is the
//                         library's; 1 shows that the inputs can see the cut)
//   R id originhex limithex
//                         a request of the batch: trie id and its range
// The program builds every trie's records bottom-up (the builder of tests/host_common/replay.h),
// puts them into ONE record store under their trie ids with one anchor map, prints
//   T id roothex
// per trie, and replays every batch through range.h's bodies as range_kernels.hip's frontier driver
// (ranges_scan's launches in run_rounds and fit_page) and k_ranges_* run them: the requests' KeyRanges into an nq-long array, round 0
// one map_find a request, then count, exclusive scan and the 16-lane fill into a next frontier --
// records and requests -- of exactly the items it takes (never more than the cut), then lengths,
// 64-bit scan, fit, and a write into outputs of exactly the scanned sizes: a write anywhere else
// is AddressSanitizer's.  Per batch:
//   A pages k n_done nexthex|- rounds ent_off_0 .. ent_off_nq key_1 val_1 .. key_k val_k
//   A nospc size
//   A missing hashhex request
#include "../host_common/replay.h"

#include "../../khipu_amd/csrc/range.h"

struct Req {
  uint32_t t;
  Key o, l;
};

static void batch(const Host& H, const std::vector<Req>& reqs, uint64_t max_entries, uint64_t val_cap, uint64_t less) {
  const uint64_t nq = reqs.size();
  const uint64_t me = std::min<uint64_t>(max_entries, nq * std::max<uint64_t>(H.rn, 1));
  const uint64_t F = me + 2 * nq - less;
  // the requests as the call takes them: packed, each array of exactly its size
  uint32_t* tries = new uint32_t[nq];
  uint8_t* origins = new uint8_t[32 * nq];
  uint8_t* limits = new uint8_t[32 * nq];
  for (uint64_t q = 0; q < nq; ++q) {
    tries[q] = reqs[q].t;
    memcpy(origins + 32 * q, reqs[q].o.data(), 32);
    memcpy(limits + 32 * q, reqs[q].l.data(), 32);
  }
  KeyRange* G = new KeyRange[nq];
  std::vector<uint32_t> cur, curq;
  uint32_t rounds = 0;
  if (H.rn) {
    const uint64_t zero[4] = {0, 0, 0, 0};
    for (uint64_t q = 0; q < nq; ++q) {  // k_ranges_root
      const bool ok = rng_request(origins, limits, q, &G[q]);
      cur.push_back(ok ? map_find(H.M, H.R, tries[q], 0, zero) : NONE);
      curq.push_back((uint32_t)q);
    }
    while (!cur.empty()) {
      if (rounds > 66) exit(7);
      const uint64_t ni = cur.size();
      uint64_t* pos = new uint64_t[ni];  // (no slack anywhere: an access past an end is ASan's)
      uint64_t total = 0;
      bool expand = false;
      for (uint64_t i = 0; i < ni; ++i) {
        if (curq[i] >= nq) exit(11);
        const uint32_t sel = rng_select(H.R, cur[i], G[curq[i]]);
        pos[i] = total;
        total += rng_count(sel);
        expand = expand || (sel & 0xFFFFu);
      }
      const uint64_t nn = std::min(total, F);
      uint32_t* nxt = new uint32_t[nn];
      uint32_t* nxtq = new uint32_t[nn];
      std::fill(nxt, nxt + nn, NONE);
      std::fill(nxtq, nxtq + nn, NONE);
      for (uint64_t i = 0; i < ni; ++i) {
        if (pos[i] >= F) continue;
        for (uint32_t lane = 0; lane < EXP_LANES; ++lane)
          if (!rng_fill_lane(H.R, H.M, cur[i], rng_select(H.R, cur[i], G[curq[i]]), lane, pos[i], F, nxt, nxtq,
                             curq[i]))
            exit(8);
      }
      for (uint64_t i = 0; i < nn; ++i) {
        if (nxt[i] == NONE || nxtq[i] == NONE) exit(9);  // every place before the cut is filled
        if (i && nxtq[i] < nxtq[i - 1]) exit(12);        // ordered by request
        if (i && nxtq[i] == nxtq[i - 1] && key_cmp(H.R.key(nxt[i - 1]), H.R.key(nxt[i])) >= 0) exit(13);  // then by key
      }
      cur.assign(nxt, nxt + nn);
      curq.assign(nxtq, nxtq + nn);
      delete[] nxt;
      delete[] nxtq;
      delete[] pos;
      ++rounds;
      if (!expand) break;
    }
  }
  delete[] tries;
  delete[] origins;
  delete[] limits;
  delete[] G;
  const uint64_t ni = cur.size(), n1 = std::min(ni, me + 1), nent = std::min(ni, me);
  if (n1 == 0) {
    printf("A pages 0 %llu - %u", (unsigned long long)nq, rounds);
    for (uint64_t q = 0; q <= nq; ++q) printf(" 0");
    printf("\n");
    return;
  }
  for (uint64_t i = 0; i < n1; ++i)
    if (rng_is_stub(H.R, cur[i])) {
      printf("A missing ");
      put_hex((const uint8_t*)&H.R.rbref[4ull * cur[i]], 32);
      printf(" %u\n", curq[i]);
      return;
    }
  // the first n1 things in arrays of exactly their sizes (k_range_lens, k_ranges_fit, k_ranges_write)
  uint32_t* items = new uint32_t[n1];
  uint32_t* iq = new uint32_t[n1];
  std::copy(cur.begin(), cur.begin() + n1, items);
  std::copy(curq.begin(), curq.begin() + n1, iq);
  uint64_t* pos = new uint64_t[nent];
  uint64_t total = 0;
  for (uint64_t i = 0; i < nent; ++i) {
    pos[i] = total;
    total += H.R.rvl[items[i]];
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
    printf("A nospc %u\n", (unsigned)H.R.rvl[items[0]]);
  } else {
    const uint64_t n_done = k < n1 ? iq[k] : nq;
    uint8_t* keys32 = new uint8_t[32 * k];
    uint8_t* vals = new uint8_t[bytes];
    uint64_t* voff = new uint64_t[k + 1];
    uint64_t* ent_off = new uint64_t[nq + 1];
    uint32_t* iqk = new uint32_t[k];  // (the search reads the returned items' requests alone)
    std::copy(iq, iq + k, iqk);
    for (uint64_t i = 0; i < k; ++i) rng_write(H.R, H.heap.data(), items[i], i, pos[i], keys32, voff, vals);
    voff[k] = bytes;
    for (uint64_t q = 0; q <= nq; ++q) ent_off[q] = rng_ent_off(iqk, k, q);
    printf("A pages %llu %llu ", (unsigned long long)k, (unsigned long long)n_done);
    if (k < n1)
      put_hex((const uint8_t*)H.R.key(items[k]), 32);
    else
      printf("-");
    printf(" %u", rounds);
    for (uint64_t q = 0; q <= nq; ++q) printf(" %llu", (unsigned long long)ent_off[q]);
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
    delete[] ent_off;
    delete[] iqk;
  }
  delete[] items;
  delete[] iq;
  delete[] pos;
}

static bool key_of(const std::string& s, Key& k) {
  const Bytes b = unhex(s);
  if (b.size() != 32) return false;
  memcpy(k.data(), b.data(), 32);
  return true;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream f(argv[1]);
  if (!f) return 2;
  std::vector<std::pair<uint32_t, std::vector<Put>>> tries;
  struct Batch {
    unsigned long long mx, cap, less;
    std::vector<Req> reqs;
  };
  std::vector<Batch> batches;
  std::string line;
  while (std::getline(f, line)) {
    std::istringstream ss(line);
    std::string tag, a, b;
    ss >> tag;
    if (tag == "T") {
      unsigned long long id;
      ss >> id;
      tries.push_back({(uint32_t)id, {}});
    } else if (tag == "P" || tag == "B") {
      ss >> a >> b;
      Put p;
      if (tries.empty() || !key_of(a, p.k)) return 2;
      p.v = unhex(b);
      p.vb = tag == "B";
      tries.back().second.push_back(p);
    } else if (tag == "Q") {
      Batch q;
      ss >> q.mx >> q.cap >> q.less;
      if (!q.mx) return 2;
      batches.push_back(q);
    } else if (tag == "R") {
      unsigned long long id;
      ss >> id >> a >> b;
      Req r;
      r.t = (uint32_t)id;
      if (batches.empty() || !key_of(a, r.o) || !key_of(b, r.l)) return 2;
      batches.back().reqs.push_back(r);
    }
  }
  // every trie's records under its id, in one store: the value offsets rebased to the shared heap
  Bytes recs, heap;
  for (auto& t : tries) {
    Builder B(t.second);
    uint8_t root[32];
    B.root_hash(root);
    printf("T %u ", t.first);
    put_hex(root, 32);
    printf("\n");
    for (uint32_t r = 0; r < B.rn; ++r) {
      B.R.rt[r] = t.first;
      if (B.R.rdb[r] == EL_LEAF || B.R.rdb[r] == VB_DEPTH) B.R.rvo[r] += heap.size();
    }
    recs.insert(recs.end(), B.recs, B.recs + B.rn * REC_BYTES);
    heap.insert(heap.end(), B.heap.begin(), B.heap.end());
  }
  Host* H = recs.empty() ? new Host() : new Host(recs, heap);  // (no record: no store is read)
  for (const Batch& q : batches) {
    if (q.reqs.empty()) return 2;
    batch(*H, q.reqs, q.mx, q.cap, q.less);
  }
  delete H;
  return 0;
}
