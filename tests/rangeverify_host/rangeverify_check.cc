// Host replay of range verification (khipu_amd/csrc/rangeverify.h), stand-alone: built with
// g++ -fsanitize=address,undefined by tests/test_rangeverify_host.py and run as a child process.
//
//   rangeverify_check FILE
// FILE, one record a line:
//   N enchex                                   a node of the call's one node set
//   R roothex originhex proved m key_1 val_1 .. key_m val_m    a range (val "-": empty)
// All ranges are one call.  The program replays what verify_ranges_dev (rangeverify_kernels.hip)
// launches up to the element build: the order check an entry, the count pass of the walk a (range, side), the
// plan a range, the exclusive scans, then the entries and the fill pass of the walk into element
// arrays of exactly the scanned total -- a write anywhere else is AddressSanitizer's -- and checks
// that every element was written exactly where the plan put it.  Per range:
//   A s status more misshex|- inbuild nkept {plen keyhex refhex side}*
// status: the plan's (final unless inbuild = 1: then the element build decides); the kept
// elements in element order: prefix length, key, reference bytes, 1 left / 2 right.
#include "../host_common/replay.h"

#include "../../khipu_amd/csrc/rangeverify.h"

struct Range {
  Bytes root, origin;
  int proved;
  std::vector<Bytes> keys, vals;
};

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream f(argv[1]);
  if (!f) return 2;
  std::vector<Bytes> nodes;
  std::vector<Range> rs;
  std::string line;
  while (std::getline(f, line)) {
    std::istringstream ss(line);
    std::string tag, a, b;
    ss >> tag;
    if (tag == "N") {
      ss >> a;
      nodes.push_back(unhex(a));
    } else if (tag == "R") {
      Range r;
      size_t m = 0;
      ss >> a >> b >> r.proved >> m;
      r.root = unhex(a);
      r.origin = unhex(b);
      if (r.root.size() != 32 || r.origin.size() != 32) return 2;
      for (size_t i = 0; i < m; ++i) {
        ss >> a >> b;
        r.keys.push_back(unhex(a));
        r.vals.push_back(unhex(b));
        if (r.keys.back().size() != 32) return 2;
      }
      rs.push_back(r);
    }
  }
  const Store st(nodes);
  const uint64_t nr = rs.size();
  uint64_t ne = 0;
  for (const Range& r : rs) ne += r.keys.size();
  // the call's arrays, each of exactly its size
  uint64_t* roots = new uint64_t[4 * nr];
  uint64_t* origins = new uint64_t[4 * nr];
  uint8_t* proved = new uint8_t[nr];
  uint64_t* keys = new uint64_t[4 * ne];
  uint64_t* voff = new uint64_t[ne + 1];
  uint64_t* ent_off = new uint64_t[nr + 1];
  uint64_t e = 0, vb = 0;
  for (uint64_t s = 0; s < nr; ++s) {
    memcpy(roots + 4 * s, rs[s].root.data(), 32);
    memcpy(origins + 4 * s, rs[s].origin.data(), 32);
    proved[s] = (uint8_t)rs[s].proved;
    ent_off[s] = e;
    for (size_t i = 0; i < rs[s].keys.size(); ++i, ++e) {
      memcpy(keys + 4 * e, rs[s].keys[i].data(), 32);
      voff[e] = vb;
      vb += rs[s].vals[i].size();
    }
  }
  ent_off[nr] = e;
  voff[ne] = vb;
  const RvIn I{roots, origins, proved, nr, keys, voff, ent_off, st.view()};
  // order
  uint32_t* bad = new uint32_t[nr]();
  for (uint64_t i = 0; i < ne; ++i) {
    const uint64_t s = rv_range_of(ent_off, nr, i);
    if (s >= nr || i < ent_off[s] || i >= ent_off[s + 1]) exit(7);
    if (rv_order_bad(I, s, i)) bad[s] = 1;
  }
  // count pass
  RvWalkOut W{new uint32_t[2 * nr], new uint32_t[2 * nr], new uint64_t[8 * nr]};
  for (uint64_t t = 0; t < 2 * nr; ++t) {
    const uint64_t s = t >> 1;
    uint64_t miss[4] = {0, 0, 0, 0};
    uint32_t code = RANGE_OK, n = 0;
    if (proved[s] && !bad[s]) {
      RvCount sink;
      code = rv_walk(I, s, (uint32_t)(t & 1), miss, sink);
      n = sink.n;
    }
    W.st[t] = code;
    W.cnt[t] = n;
    memcpy(W.miss + 4 * t, miss, 32);
  }
  // plan and scans
  uint8_t* status = new uint8_t[nr];
  uint8_t* more = new uint8_t[nr];
  uint64_t* miss32 = new uint64_t[4 * nr];
  uint64_t* base = new uint64_t[nr];
  uint32_t* inb = new uint32_t[nr];
  uint32_t* segid = new uint32_t[nr];
  uint64_t* cnt = new uint64_t[nr];
  uint64_t nel = 0;
  uint32_t nseg = 0;
  for (uint64_t s = 0; s < nr; ++s) {
    bool fin;
    const uint64_t n = rv_plan(I, s, bad[s], W, status + s, more + s, miss32 + 4 * s, &fin);
    cnt[s] = fin ? 0 : n;
    inb[s] = fin ? 0 : 1;
    base[s] = nel;
    segid[s] = nseg;
    nel += cnt[s];
    nseg += inb[s];
  }
  // elements: the entries, then the fill pass, into arrays of exactly nel
  RvElems E{new uint64_t[4 * nel], new uint32_t[nel], new uint8_t[nel], new uint64_t[4 * nel], new uint8_t[nel],
            new uint8_t[nel],      new uint64_t[nel], new uint32_t[nel], new uint8_t[nel], nel};
  std::fill(E.side, E.side + nel, (uint8_t)0xEE);
  for (uint64_t i = 0; i < ne; ++i) {
    const uint64_t s = rv_range_of(ent_off, nr, i);
    if (!inb[s]) continue;
    const uint64_t at = base[s] + (i - ent_off[s]);
    if (at >= nel || E.side[at] != 0xEE) exit(8);
    rv_entry_elem(I, i, E, at, segid[s]);
  }
  for (uint64_t t = 0; t < 2 * nr; ++t) {
    const uint64_t s = t >> 1;
    if (!inb[s] || !proved[s] || !W.cnt[t]) continue;
    const uint64_t m = ent_off[s + 1] - ent_off[s];
    RvFill sink{E, base[s] + m + ((t & 1) ? W.cnt[2 * s] : 0), segid[s]};
    for (uint64_t k = 0; k < W.cnt[t]; ++k)
      if (E.side[sink.at + k] != 0xEE) exit(9);
    uint64_t miss[4];
    const uint32_t code = rv_walk(I, s, (uint32_t)(t & 1), miss, sink);
    if (code != W.st[t] || sink.n != W.cnt[t]) exit(10);  // the passes agree
  }
  for (uint64_t k = 0; k < nel; ++k)
    if (E.side[k] == 0xEE) exit(11);  // every planned place is filled
  for (uint64_t s = 0; s < nr; ++s) {
    const uint64_t m = ent_off[s + 1] - ent_off[s];
    printf("A %llu %u %u ", (unsigned long long)s, status[s], more[s]);
    put_hex((const uint8_t*)(miss32 + 4 * s), status[s] == RANGE_MISSING ? 32 : 0);
    printf(" %u %llu", inb[s], (unsigned long long)(inb[s] ? cnt[s] - m : 0));
    for (uint64_t k = base[s] + m; inb[s] && k < base[s] + cnt[s]; ++k) {
      if (E.seg[k] != segid[s] || E.db[k] != E.oldd[k] || E.side[k] == 0) exit(12);
      printf(" %u ", E.db[k]);
      put_hex((const uint8_t*)(E.key + 4 * k), 32);
      printf(" ");
      put_hex((const uint8_t*)(E.ref + 4 * k), E.rl[k]);
      printf(" %u", E.side[k]);
    }
    for (uint64_t k = base[s]; inb[s] && k < base[s] + m; ++k)
      if (E.side[k] != 0 || E.db[k] != EL_LEAF || E.oldd[k] != EL_NEW || E.seg[k] != segid[s] ||
          E.vl[k] != voff[ent_off[s] + (k - base[s]) + 1] - voff[ent_off[s] + (k - base[s])])
        exit(13);
    printf("\n");
  }
  delete[] roots; delete[] origins; delete[] proved; delete[] keys; delete[] voff; delete[] ent_off; delete[] bad;
  delete[] W.st; delete[] W.cnt; delete[] W.miss; delete[] status; delete[] more; delete[] miss32; delete[] base;
  delete[] inb; delete[] segid; delete[] cnt;
  delete[] E.key; delete[] E.seg; delete[] E.db; delete[] E.ref; delete[] E.rl; delete[] E.oldd; delete[] E.vo;
  delete[] E.vl; delete[] E.side;
  return 0;
}
