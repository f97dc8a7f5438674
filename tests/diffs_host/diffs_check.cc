// Host replay of the batched trie diff (khipu_amd/csrc/diff.h "MANY PAIRS A CALL"), stand-alone:
// built with g++ -fsanitize=address,undefined by tests/test_diffs_host.py and run as a child
// process.
//
//   diffs_check FILE
// FILE, one record a line:
//   TA id / TB id         the puts that follow belong to trie `id` of side a / of side b
//   P keyhex valuehex     a put (32-byte keys; later puts win)
//   B keyhex valuehex     a put that leaves khipu's value-only branch (forest.h VB_DEPTH)
//   Q max_entries val_cap cut_less late_skip same
//                         a batch: the requests that follow, answered under one budget; the
//                         frontiers are cut at max_entries + 2 * nq - cut_less items (0 is the
//                         library's; 1 shows that the inputs can see the cut); late_skip = 1 makes
//                         the skip test after the cut instead of before it (0 is the library's);
//                         same = 1: side b is side a's store (one handle on both sides)
//   R id_a id_b originhex limithex
//                         a request of the batch: the two trie ids and the range
// The program builds every trie's records bottom-up (the builder of tests/host_common/replay.h),
// puts them into ONE record store a side under their trie ids with one anchor map, prints
//   T a|b id roothex
// per trie, and replays every batch through diff.h's bodies as range_kernels.hip's frontier driver
// (diffs_scan's launches in run_rounds and fit_page) and k_diffs_* run them: round 0 one df_request a request, then per round select (16 lanes an item,
// each item against its own request's range), exclusive scan, the 16-lane fill into a next frontier
// -- records, depths and requests -- of exactly the items it takes (never more than the cut), then
// lengths, 64-bit scan, fit, and a write into outputs of exactly the scanned sizes: a write
// anywhere else is AddressSanitizer's.  Every planned place must be filled exactly once.  Per batch:
//   A pages k n_done nexthex|- rounds visited ent_off_0 .. ent_off_nq key_1 kind_1 val_1 .. key_k kind_k val_k
//   A nospc size
//   A missing hashhex request
#include "../host_common/replay.h"

#include "../../khipu_amd/csrc/diff.h"

struct Req {
  uint32_t ta, tb;
  Key o, l;
};

static void batch(const Host& HA, const Host& HB, bool same, const std::vector<Req>& reqs, uint64_t max_entries,
                  uint64_t val_cap, uint64_t less, bool late_skip) {
  const uint64_t nq = reqs.size();
  const DSide A{HA.R, HA.M, HA.heap.data()}, B{HB.R, HB.M, HB.heap.data()};
  const uint64_t me = std::min<uint64_t>(max_entries, nq * std::max<uint64_t>(HA.rn + HB.rn, 1));
  const uint64_t F = me + 2 * nq - less;
  // the requests as the call takes them: packed, each array of exactly its size
  uint32_t* ta = new uint32_t[nq];
  uint32_t* tb = new uint32_t[nq];
  uint8_t* origins = new uint8_t[32 * nq];
  uint8_t* limits = new uint8_t[32 * nq];
  for (uint64_t q = 0; q < nq; ++q) {
    ta[q] = reqs[q].ta;
    tb[q] = reqs[q].tb;
    memcpy(origins + 32 * q, reqs[q].o.data(), 32);
    memcpy(limits + 32 * q, reqs[q].l.data(), 32);
  }
  KeyRange* G = new KeyRange[nq];
  std::vector<uint32_t> ca, cb, cd, cq;
  uint32_t rounds = 0;
  uint64_t visited = 0;
  if (HA.rn || HB.rn) {
    uint64_t live = 0;
    {  // k_diffs_root: frontiers of exactly nq items
      uint32_t *ia = new uint32_t[nq], *ib = new uint32_t[nq], *id = new uint32_t[nq], *iq = new uint32_t[nq];
      for (uint64_t q = 0; q < nq; ++q)
        live += df_request(A, ta, HA.rn != 0, B, tb, HB.rn != 0, same, origins, limits, q, G, ia, ib, id, iq);
      if (live) {
        ca.assign(ia, ia + nq);
        cb.assign(ib, ib + nq);
        cd.assign(id, id + nq);
        cq.assign(iq, iq + nq);
      }
      delete[] ia;
      delete[] ib;
      delete[] id;
      delete[] iq;
    }
    while (!ca.empty()) {
      if (rounds > 68) exit(7);
      const uint64_t ni = ca.size();
      visited += rounds ? ni : live;
      uint32_t* sel = new uint32_t[ni];  // (no slack anywhere: an access past an end is ASan's)
      uint64_t* pos = new uint64_t[ni];
      uint64_t total = 0;
      bool expand = false;
      for (uint64_t i = 0; i < ni; ++i) {
        if (cq[i] >= nq) exit(11);
        const uint32_t plan = df_plan(A, ca[i], B, cb[i], G[cq[i]]);
        uint32_t kids = 0;
        for (uint32_t lane = 0; lane < EXP_LANES; ++lane) {
          const bool alive = late_skip ? ((plan >> lane) & 1) != 0 : df_lane_alive(A, ca[i], B, cb[i], plan, lane);
          kids |= (alive ? 1u : 0u) << lane;
        }
        sel[i] = (plan & ~0xFFFFu) | kids;
        pos[i] = total;
        total += df_count(sel[i]);
        expand = expand || df_expands(sel[i]);
      }
      const uint64_t nn = std::min(total, F);
      uint32_t *oa = new uint32_t[nn], *ob = new uint32_t[nn], *od = new uint32_t[nn], *oq = new uint32_t[nn];
      // (a filled place holds a depth <= 64 and a request < nq: each place counts its writes below)
      std::fill(od, od + nn, 0xFFFFFFFFu);
      std::fill(oq, oq + nn, 0xFFFFFFFFu);
      for (uint64_t i = 0; i < ni; ++i) {
        if (pos[i] >= F) continue;
        for (uint32_t lane = 0; lane < EXP_LANES; ++lane) {
          // exactly once: the lane's places are still unwritten before it runs
          const uint32_t s = sel[i];
          uint64_t first = pos[i], cnt = 0;
          if (s & DF_SELF)
            cnt = lane == 0;
          else if (s & (DF_SPLIT_A | DF_SPLIT_B))
            cnt = lane == 0 ? df_count(s) : 0;
          else if ((s >> lane) & 1) {
            first = pos[i] + kh_popc(s & ((1u << lane) - 1u));
            cnt = 1;
          }
          for (uint64_t p = first; p < first + cnt && p < nn; ++p)
            if (od[p] != 0xFFFFFFFFu || oq[p] != 0xFFFFFFFFu) exit(14);
          if (!df_fill_lane(A, ca[i], B, cb[i], cd[i], s, lane, pos[i], F, oa, ob, od, oq, cq[i])) exit(8);
          for (uint64_t p = first; p < first + cnt && p < nn; ++p)
            if (od[p] == 0xFFFFFFFFu || oq[p] != cq[i]) exit(15);
        }
      }
      std::vector<uint32_t> na, nb, nd, nqv;
      for (uint64_t i = 0; i < nn; ++i) {
        if (od[i] == 0xFFFFFFFFu || oq[i] == 0xFFFFFFFFu) exit(9);  // every place before the cut is filled
        if (i && oq[i] < oq[i - 1]) exit(12);                        // ordered by request
        if (i && oq[i] == oq[i - 1] &&
            key_cmp(df_key(A, oa[i - 1], B, ob[i - 1]), df_key(A, oa[i], B, ob[i])) > 0)
          exit(13);  // then by key (the two halves of a split and a carried record share prefixes: >=)
        if (late_skip && df_skip(A, oa[i], B, ob[i], od[i])) continue;
        na.push_back(oa[i]);
        nb.push_back(ob[i]);
        nd.push_back(od[i]);
        nqv.push_back(oq[i]);
      }
      ca.swap(na);
      cb.swap(nb);
      cd.swap(nd);
      cq.swap(nqv);
      delete[] oa;
      delete[] ob;
      delete[] od;
      delete[] oq;
      delete[] sel;
      delete[] pos;
      ++rounds;
      if (!expand) break;
    }
  }
  delete[] ta;
  delete[] tb;
  delete[] origins;
  delete[] limits;
  delete[] G;
  const uint64_t ni = ca.size(), n1 = std::min(ni, me + 1), nent = std::min(ni, me);
  if (n1 == 0) {
    printf("A pages 0 %llu - %u %llu", (unsigned long long)nq, rounds, (unsigned long long)visited);
    for (uint64_t q = 0; q <= nq; ++q) printf(" 0");
    printf("\n");
    return;
  }
  // the first n1 things in arrays of exactly their sizes (k_diff_lens, k_diffs_fit, k_diffs_write)
  uint32_t *ia = new uint32_t[n1], *ib = new uint32_t[n1], *iq = new uint32_t[n1];
  std::copy(ca.begin(), ca.begin() + n1, ia);
  std::copy(cb.begin(), cb.begin() + n1, ib);
  std::copy(cq.begin(), cq.begin() + n1, iq);
  bool done = false;
  for (uint64_t i = 0; i < n1 && !done; ++i)
    if (df_missing(A, ia[i], B, ib[i])) {
      const bool of_a = ia[i] != NONE && df_stub(A.R, ia[i]);
      printf("A missing ");
      put_hex(of_a ? (const uint8_t*)&A.R.rbref[4ull * ia[i]] : (const uint8_t*)&B.R.rbref[4ull * ib[i]], 32);
      printf(" %u\n", iq[i]);
      done = true;
    }
  if (!done) {
    uint64_t* pos = new uint64_t[nent];
    uint64_t total = 0;
    for (uint64_t i = 0; i < nent; ++i) {
      pos[i] = total;
      total += df_len(A, ia[i], B, ib[i]);
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
      printf("A nospc %llu\n", (unsigned long long)df_len(A, ia[0], B, ib[0]));
    } else {
      const uint64_t n_done = k < n1 ? iq[k] : nq;
      uint8_t* keys32 = new uint8_t[32 * k];
      uint8_t* kinds = new uint8_t[k];
      uint8_t* vals = new uint8_t[bytes];
      uint64_t* voff = new uint64_t[k + 1];
      uint64_t* ent_off = new uint64_t[nq + 1];
      uint32_t* iqk = new uint32_t[k];  // (the search reads the returned items' requests alone)
      std::copy(iq, iq + k, iqk);
      for (uint64_t i = 0; i < k; ++i) df_write(A, ia[i], B, ib[i], i, pos[i], keys32, kinds, voff, vals);
      voff[k] = bytes;
      for (uint64_t q = 0; q <= nq; ++q) ent_off[q] = rng_ent_off(iqk, k, q);
      printf("A pages %llu %llu ", (unsigned long long)k, (unsigned long long)n_done);
      if (k < n1)
        put_hex((const uint8_t*)df_key(A, ia[k], B, ib[k]), 32);
      else
        printf("-");
      printf(" %u %llu", rounds, (unsigned long long)visited);
      for (uint64_t q = 0; q <= nq; ++q) printf(" %llu", (unsigned long long)ent_off[q]);
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
      delete[] ent_off;
      delete[] iqk;
    }
    delete[] pos;
  }
  delete[] ia;
  delete[] ib;
  delete[] iq;
}

static bool key_of(const std::string& s, Key& k) {
  const Bytes b = unhex(s);
  if (b.size() != 32) return false;
  memcpy(k.data(), b.data(), 32);
  return true;
}

typedef std::vector<std::pair<uint32_t, std::vector<Put>>> Tries;

// every trie's records under its id, in one store: the value offsets rebased to the shared heap
static Host* store_of(Tries& tries, char side) {
  Bytes recs, heap;
  for (auto& t : tries) {
    Builder B(t.second);
    uint8_t root[32];
    B.root_hash(root);
    printf("T %c %u ", side, t.first);
    put_hex(root, 32);
    printf("\n");
    for (uint32_t r = 0; r < B.rn; ++r) {
      B.R.rt[r] = t.first;
      if (B.R.rdb[r] == EL_LEAF || B.R.rdb[r] == VB_DEPTH) B.R.rvo[r] += heap.size();
    }
    recs.insert(recs.end(), B.recs, B.recs + B.rn * REC_BYTES);
    heap.insert(heap.end(), B.heap.begin(), B.heap.end());
  }
  if (!recs.empty()) return new Host(recs, heap);
  Host* h = new Host();  // (no record: an empty map over one zeroed record, never read)
  h->init(1);
  return h;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream f(argv[1]);
  if (!f) return 2;
  Tries tries[2];
  Tries* into = nullptr;
  struct Batch {
    unsigned long long mx, cap, less, late, same;
    std::vector<Req> reqs;
  };
  std::vector<Batch> batches;
  std::string line;
  while (std::getline(f, line)) {
    std::istringstream ss(line);
    std::string tag, a, b;
    ss >> tag;
    if (tag == "TA" || tag == "TB") {
      unsigned long long id;
      ss >> id;
      into = &tries[tag[1] == 'B'];
      into->push_back({(uint32_t)id, {}});
    } else if (tag == "P" || tag == "B") {
      ss >> a >> b;
      Put p;
      if (!into || !key_of(a, p.k)) return 2;
      p.v = unhex(b);
      p.vb = tag == "B";
      into->back().second.push_back(p);
    } else if (tag == "Q") {
      Batch q;
      ss >> q.mx >> q.cap >> q.less >> q.late >> q.same;
      if (!q.mx) return 2;
      batches.push_back(q);
    } else if (tag == "R") {
      unsigned long long ida, idb;
      ss >> ida >> idb >> a >> b;
      Req r;
      r.ta = (uint32_t)ida;
      r.tb = (uint32_t)idb;
      if (batches.empty() || !key_of(a, r.o) || !key_of(b, r.l)) return 2;
      batches.back().reqs.push_back(r);
    }
  }
  Host* HA = store_of(tries[0], 'a');
  Host* HB = store_of(tries[1], 'b');
  for (const Batch& q : batches) {
    if (q.reqs.empty()) return 2;
    batch(*HA, q.same ? *HA : *HB, q.same != 0, q.reqs, q.mx, q.cap, q.less, q.late != 0);
  }
  delete HA;
  delete HB;
  return 0;
}
