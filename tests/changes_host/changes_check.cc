// Host replay of the changes since a savepoint (khipu_amd/csrc/changes.h), stand-alone: built with
// g++ -fsanitize=address,undefined by tests/test_changes_host.py and run as a child process.
//
//   changes_check FILE
// FILE, one record a line; the record arrays are hand-made, no trie is built:
//   F forest                      1: the handle is a forest (the order includes the trie id)
//   R trie keyhex kind valuehex   the next record of the handle's record array NOW.  kind: L a live
//                                 leaf, V a live value-only branch, B a live branch (no entry),
//                                 l / v a dead leaf / value-only branch, Z a cleared record
//   J idx trie keyhex kind valuehex   the next saved copy of the journal: taken from record idx
//                                 (-: none, jidx = NONE), kinds as above
//   S rn0 j0                      the savepoint: its record count and its journal fill
//   Q reverse from_trie fromhex|- max_entries val_cap
// Every value is appended to one heap, so equal bytes of two records still lie at two places.
// Per Q the program replays collect, order, join and page through changes.h's bodies as
// range_kernels.hip runs them -- the 16-byte word a record at collect, stable passes over 64-bit
// words (the first word and the trie id, all four words after a tie), a thread a sorted place in the
// join, the first max_entries + 1 differences as diff.h items, lengths, 64-bit scan, rng_fit, and
// df_write into outputs of exactly the scanned sizes (a write anywhere else is AddressSanitizer's):
//   A page k more next_trie nexthex|- n_total passes trie_1 key_1 kind_1 val_1 .. trie_k key_k kind_k val_k
//   A nospc size n_total
#include "../host_common/replay.h"

#include "../../khipu_amd/csrc/changes.h"

struct Rec {
  uint32_t t;
  Key k;
  char kind;
  Bytes v;
};

static uint8_t* image(const std::vector<Rec>& rs, Bytes& heap) {
  uint8_t* out = new uint8_t[rs.size() * REC_BYTES];  // (exactly the records)
  for (size_t i = 0; i < rs.size(); ++i) {
    const Rec& r = rs[i];
    RecVal v;
    memset(&v, 0, sizeof(v));
    if (r.kind != 'Z') {
      memcpy(v.k, r.k.data(), 32);
      v.t = r.t;
      v.d = 3;
      v.db = (r.kind == 'L' || r.kind == 'l') ? EL_LEAF : (r.kind == 'V' || r.kind == 'v') ? VB_DEPTH : 7;
      v.mask = r.kind == 'B' ? 0x0101 : 0;
      v.live = (r.kind == 'l' || r.kind == 'v') ? REC_DEAD : REC_LIVE;
      v.rl = v.brl = 32;
      v.vl = (uint32_t)r.v.size();
      v.vo = heap.size();
      heap.insert(heap.end(), r.v.begin(), r.v.end());
    }
    rec_store(out, i, v);
  }
  return out;
}

static bool entry_at(const uint8_t* base, uint64_t r) {
  uint64_t w[2];
  memcpy(w, base + r * REC_BYTES + 32, 16);
  return chg_entry_words(w[0], w[1]);
}

static void query(const ChgSrc& S, bool forest, bool reverse, uint32_t from_trie, const Bytes& from,
                  uint64_t max_entries, uint64_t val_cap) {
  const uint64_t N = chg_slots(S);
  // ---- collect
  std::vector<uint32_t> keep(N, 0);
  for (uint64_t g = 0; g < S.jn + S.an; ++g) {
    if (g < S.jn) {
      const uint64_t p = S.j0 + g;
      const uint32_t idx = S.jidx[p];
      const bool old = chg_keep_old(idx, S.rn0, entry_at(S.J.rk.b, p));
      keep[g] = old;
      keep[S.jn + g] = old && chg_keep_new(idx, S.rn0, true, entry_at(S.R.rk.b, idx));
    } else {
      keep[2 * S.jn + (g - S.jn)] = entry_at(S.R.rk.b, S.rn0 + (g - S.jn));
    }
  }
  for (uint64_t s = 0; s < N; ++s)  // the word test is the record test
    if (keep[s] && !chg_live_entry(chg_recs(S, s), chg_rec(S, s))) exit(7);
  uint64_t nc = 0;
  for (uint64_t s = 0; s < N; ++s) nc += keep[s];
  uint64_t fw[4] = {0, 0, 0, 0};
  if (!from.empty()) memcpy(fw, from.data(), 32);
  const uint32_t ft = forest ? from_trie : 0u;
  uint32_t passes = 0;
  std::vector<uint32_t> ia, ib;
  uint64_t nd = 0;
  const uint64_t me = std::min<uint64_t>(max_entries, std::max<uint64_t>(N, 1));
  for (int full = 0; nc && full < 2; ++full) {
    uint32_t* sv = new uint32_t[nc];  // (exactly the kept slots: an access past the end is ASan's)
    uint64_t at = 0;
    for (uint64_t s = 0; s < N; ++s)
      if (keep[s]) sv[at++] = (uint32_t)s;
    const uint32_t words[5] = {3, 2, 1, 0, CHG_WORD_TRIE};
    for (int i = full ? 0 : 3; i < (forest ? 5 : 4); ++i) {
      const uint32_t w = words[i];
      std::stable_sort(sv, sv + nc, [&](uint32_t a, uint32_t b) { return chg_sort_word(S, a, w) < chg_sort_word(S, b, w); });
      ++passes;
    }
    bool tie = false;
    ia.clear();
    ib.clear();
    nd = 0;
    for (uint64_t j = 0; j < nc; ++j) {
      bool t = false;
      uint32_t po, rn;
      if (chg_head(S, sv, j, &t) && chg_join(S, sv, nc, j, &po, &rn) &&
          (from.empty() || chg_from(S, sv[j], ft, fw))) {
        if (nd < me + 1) {
          uint32_t a, b;
          chg_item(po, rn, reverse, &a, &b);
          ia.push_back(a);
          ib.push_back(b);
        }
        ++nd;
      }
      tie = tie || t;
    }
    delete[] sv;
    if (full || !tie) break;
  }
  // ---- page
  const DSide A = chg_side(S, !reverse), B = chg_side(S, reverse);
  const uint64_t ni = ia.size(), n1 = std::min(ni, me + 1), nent = std::min(ni, me);
  if (n1 == 0) {
    printf("A page 0 0 0 - 0 %u\n", passes);
    return;
  }
  uint64_t* pos = new uint64_t[nent];
  uint64_t total = 0;
  for (uint64_t i = 0; i < nent; ++i) {
    if (df_missing(A, ia[i], B, ib[i])) exit(8);
    pos[i] = total;
    total += df_len(A, ia[i], B, ib[i]);
  }
  unsigned long long fit[2] = {~0ULL, ~0ULL};
  int writers = 0;
  for (uint64_t i = 0; i <= nent; ++i) {
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
    printf("A nospc %llu %llu\n", (unsigned long long)df_len(A, ia[0], B, ib[0]), (unsigned long long)nd);
    delete[] pos;
    return;
  }
  uint8_t* keys32 = new uint8_t[32 * k];
  uint8_t* kinds = new uint8_t[k];
  uint8_t* vals = new uint8_t[bytes];
  uint64_t* voff = new uint64_t[k + 1];
  uint32_t* tries = new uint32_t[k];
  for (uint64_t i = 0; i < k; ++i) {
    df_write(A, ia[i], B, ib[i], i, pos[i], keys32, kinds, voff, vals);
    tries[i] = chg_item_trie(A, ia[i], B, ib[i]);
  }
  voff[k] = bytes;
  printf("A page %llu %d ", (unsigned long long)k, k < n1 ? 1 : 0);
  if (k < n1) {
    printf("%u ", chg_item_trie(A, ia[k], B, ib[k]));
    put_hex((const uint8_t*)df_key(A, ia[k], B, ib[k]), 32);
  } else {
    printf("0 -");
  }
  printf(" %llu %u", (unsigned long long)nd, passes);
  for (uint64_t i = 0; i < k; ++i) {
    printf(" %u ", tries[i]);
    put_hex(keys32 + 32 * i, 32);
    printf(" %u ", (unsigned)kinds[i]);
    put_hex(vals + voff[i], voff[i + 1] - voff[i]);
  }
  printf("\n");
  delete[] keys32;
  delete[] kinds;
  delete[] vals;
  delete[] voff;
  delete[] tries;
  delete[] pos;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream f(argv[1]);
  if (!f) return 2;
  std::vector<Rec> recs, jrecs;
  std::vector<uint32_t> jidx;
  std::vector<std::string> qlines;
  uint64_t rn0 = 0, j0 = 0;
  bool forest = false;
  std::string line;
  while (std::getline(f, line)) {
    std::istringstream ss(line);
    std::string tag, a, b, c, d;
    ss >> tag;
    if (tag == "R" || tag == "J") {
      std::string idx;
      if (tag == "J") ss >> idx;
      Rec r;
      ss >> r.t >> a >> b >> c;
      const Bytes k = unhex(a);
      if (k.size() != 32 || b.size() != 1) return 2;
      memcpy(r.k.data(), k.data(), 32);
      r.kind = b[0];
      r.v = unhex(c);
      if (tag == "R") {
        recs.push_back(r);
      } else {
        jrecs.push_back(r);
        jidx.push_back(idx == "-" ? NONE : (uint32_t)strtoul(idx.c_str(), nullptr, 10));
      }
    } else if (tag == "S") {
      ss >> rn0 >> j0;
    } else if (tag == "F") {
      int x = 0;
      ss >> x;
      forest = x != 0;
    } else if (tag == "Q") {
      qlines.push_back(line);
    }
  }
  if (rn0 > recs.size() || j0 > jrecs.size()) return 2;
  Bytes heap;
  uint8_t* R = image(recs, heap);
  uint8_t* J = image(jrecs, heap);
  uint32_t* ji = new uint32_t[jidx.size()];
  std::copy(jidx.begin(), jidx.end(), ji);
  uint8_t* hp = new uint8_t[heap.size()];  // (exactly the heap: a value read past it is ASan's)
  std::copy(heap.begin(), heap.end(), hp);
  const ChgSrc S{recs_at(J), ji, recs_at(R), hp, j0, jrecs.size() - j0, rn0, recs.size() - rn0};
  for (const std::string& ql : qlines) {
    std::istringstream ss(ql);
    std::string tag, fr;
    unsigned long long rev, ft, mx, cap;
    ss >> tag >> rev >> ft >> fr >> mx >> cap;
    const Bytes from = unhex(fr);
    if ((from.size() != 32 && !from.empty()) || !mx) return 2;
    query(S, forest, rev != 0, (uint32_t)ft, from, mx, cap);
  }
  delete[] R;
  delete[] J;
  delete[] ji;
  delete[] hp;
  return 0;
}
