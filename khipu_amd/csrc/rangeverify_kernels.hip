// Kernels of kh_verify_ranges / kh_dev_verify_ranges (rangeverify.h holds the bodies), a cold
// compilation unit of their own like range_kernels.hip: the hot kernels of khst.hip keep their
// placement (tests/test_code_layout.py).  Kernels only; khst.hip declares and launches them.
//
// One thread per entry, per range or per (range, side): the walk parses a node's 17 items one
// after the other whichever lane does it, and what it waits for is the binary search of the next
// hash and the first line of that node -- a chain of dependent reads per path, not a fan-out.
// No LDS, no atomics: the kept elements land at the scanned places of the count pass.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rangeverify.h"

using namespace khst;

namespace {
constexpr int BS = 256;
}  // namespace

// Order: entry i against its predecessor in its range (the first against the origin); every
// writer stores the same 1.
__global__ void __launch_bounds__(BS) k_rv_order(RvIn I, uint64_t ne, uint32_t* bad) {
  const uint64_t i = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (i >= ne) return;
  const uint64_t s = rv_range_of(I.ent_off, I.nr, i);
  if (rv_order_bad(I, s, i)) bad[s] = 1;
}

// Count pass of the boundary walk: thread t is side t & 1 of range t >> 1 (a proved range whose
// order held; every other one leaves zeros).
__global__ void __launch_bounds__(BS) k_rv_walk_count(RvIn I, const uint32_t* bad, RvWalkOut W) {
  const uint64_t t = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (t >= 2 * I.nr) return;
  const uint64_t s = t >> 1;
  uint64_t miss[4] = {0, 0, 0, 0};
  uint32_t st = RANGE_OK, n = 0;
  if (I.proved[s] && !bad[s]) {
    RvCount sink;
    st = rv_walk(I, s, (uint32_t)(t & 1), miss, sink);
    n = sink.n;
  }
  W.st[t] = st;
  W.cnt[t] = n;
  for (int q = 0; q < 4; ++q) W.miss[4 * t + q] = miss[q];
}

// Per range: the status so far, `more`, the missing hash, and what the range brings to the build
// (cnt[s] elements and inb[s] = 1, or nothing: it is decided).
__global__ void __launch_bounds__(BS) k_rv_plan(RvIn I, const uint32_t* bad, RvWalkOut W, uint8_t* status, uint8_t* more,
                                                uint64_t* miss32, uint64_t* cnt, uint32_t* inb) {
  const uint64_t s = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (s >= I.nr) return;
  uint64_t miss[4];
  bool final;
  uint8_t st, mo;
  const uint64_t n = rv_plan(I, s, bad[s], W, &st, &mo, miss, &final);
  status[s] = st;
  more[s] = mo;
  for (int q = 0; q < 4; ++q) miss32[4 * s + q] = miss[q];
  cnt[s] = final ? 0 : n;
  inb[s] = final ? 0u : 1u;
}

// Fill pass of the walk: the same body, the kept elements of (range, side) written behind the
// range's entries (base[s] + m, side 1 behind side 0) with the range's compact segment id.
__global__ void __launch_bounds__(BS) k_rv_walk_fill(RvIn I, RvWalkOut W, const uint32_t* inb, const uint64_t* base,
                                                     const uint32_t* segid, RvElems E) {
  const uint64_t t = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (t >= 2 * I.nr) return;
  const uint64_t s = t >> 1;
  if (!inb[s] || !I.proved[s] || !W.cnt[t]) return;
  const uint64_t m = I.ent_off[s + 1] - I.ent_off[s];
  RvFill sink{E, base[s] + m + ((t & 1) ? W.cnt[2 * s] : 0), segid[s]};
  uint64_t miss[4];
  rv_walk(I, s, (uint32_t)(t & 1), miss, sink);
}

// The entries of the ranges in the build, as leaf elements at the head of their range's span.
__global__ void __launch_bounds__(BS) k_rv_entries(RvIn I, uint64_t ne, const uint32_t* inb, const uint64_t* base,
                                                   const uint32_t* segid, RvElems E) {
  const uint64_t i = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (i >= ne) return;
  const uint64_t s = rv_range_of(I.ent_off, I.nr, i);
  if (!inb[s]) return;
  rv_entry_elem(I, i, E, base[s] + (i - I.ent_off[s]), segid[s]);
}

// After the element build (k_stub_moved's check on the element arrays): a kept element whose
// parent depth is not the one it hung at flags its segment; every writer stores the same 1.
__global__ void __launch_bounds__(BS) k_rv_moved(RvElems E, const uint32_t* sidx, const int8_t* pd, uint64_t m,
                                                 uint32_t* moved) {
  const uint64_t i = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (i >= m) return;
  const uint32_t in = sidx[i];
  if (rv_moved(E, in, pd[i])) moved[E.seg[in]] = 1;
}

// The ranges that went through the build: the segment's root against the given one.
__global__ void __launch_bounds__(BS) k_rv_final(RvIn I, const uint32_t* inb, const uint32_t* segid,
                                                 const uint32_t* moved, const uint64_t* res_hash,
                                                 const uint32_t* res_len, uint8_t* status) {
  const uint64_t s = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (s >= I.nr || !inb[s]) return;
  const uint32_t g = segid[s];
  bool ok = !moved[g] && res_len[g] != 0;
  for (int q = 0; q < 4 && ok; ++q) ok = res_hash[4 * g + q] == I.roots[4 * s + q];
  status[s] = ok ? RANGE_OK : RANGE_BAD_ROOT;
}
