// Range fills (kh_trie_fill_ranges_host, kh_dev_trie_fill_ranges): the receiving half of a range
// sync on a partial handle.  A range response (origin o, entries k_1 < .. < k_m, hi = k_m) replaces
// the stubs that lie INSIDE [o, hi] with the subtrees built from the entries, and is kept only if
// no root moves: the stub remembers the hash its parent holds, so the trie checks the rebuild.
//
//   order    the range verifier's check (rangeverify.h rv_order_bad), before the handle is read
//   plan     per range: is the trie resident (a live record at anchor (t, 0)), its root, the span
//   stubs    one streaming pass over the records (their first 64-byte line): per listed trie the
//            live stubs and the ones inside its span
//   commit   the entries as upserts of a forest commit in FILL MODE under a savepoint: the descent
//            that reaches an inside stub marks it touched and stops (the gather brings nothing for
//            a touched stub, the delete takes it out of the map), one that reaches any other stub
//            refuses the batch as a commit does; trie keys go to the sort unhashed
//   judge    per range: the new root against the old one (the given one for a trie loaded whole),
//            and the stubs the descent dropped against the inside stubs of the pass -- an inside
//            stub no entry reached would stand for keys the response left out
//
// KH_HD bodies only: the span test is shared by the kernels of load_kernels.hip and the host replay
// of tests/fillrange_host.
#pragma once
#include "forest.h"

namespace khst {

// The keys below nibble prefix k[0, md) are [k|0..0, k|f..f] (k is zero past md, as a stub's record
// keeps it): hi_out is the upper end.
KH_HD void fill_span_end(const uint64_t* k, uint32_t md, uint64_t hi_out[4]) {
  for (int q = 0; q < 4; ++q) {
    const uint32_t nib0 = 16u * (uint32_t)q;
    if (md <= nib0) {
      hi_out[q] = ~0ULL;
    } else if (md >= nib0 + 16) {
      hi_out[q] = k[q];
    } else {
      hi_out[q] = bswap64(bswap64(k[q]) | (~0ULL >> (4 * (md - nib0))));
    }
  }
}
// A stub whose missing node starts at depth md below prefix k is inside [lo, hi] when its whole
// span is (the plain form and STUB_BRANCH alike: md is the record's rmask low byte).
KH_HD bool fill_inside(const uint64_t* k, uint32_t md, const uint64_t* lo, const uint64_t* hi) {
  uint64_t a[4], b[4];
  for (int q = 0; q < 4; ++q) a[q] = prefix_word(k, md, q);
  fill_span_end(a, md, b);
  return key_cmp(a, lo) >= 0 && key_cmp(b, hi) <= 0;
}

// What a commit in fill mode reads and writes beside a commit's own arrays (device pointers).
// Sorted position j is the j-th listed trie in ascending id order; a trie is listed once.
struct FillMode {
  const uint32_t* tries;  // [nt] the listed trie ids, ascending ({0} on a single trie)
  const uint64_t* lo;     // [nt*4] the origin of trie j's range
  const uint64_t* hi;     // [nt*4] its last key (ff..ff for a range without entries)
  uint32_t nt;
  uint32_t* dropped;      // [nt] inside stubs the descent dropped (each counted once)
  uint32_t* miss;         // [nt] 1: an entry reached a stub that is not inside
};

}  // namespace khst
