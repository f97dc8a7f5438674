// kh_verify_ranges / kh_dev_verify_ranges: their kernels (rangeverify.h holds the bodies), then the
// host driver verify_ranges_dev and the C entry points (host.h).  A cold compilation unit of its
// own like range_kernels.hip: the hot kernels of khst.hip keep their placement
// (tests/test_code_layout.py).
//
// One thread per entry, per range or per (range, side): the walk parses a node's 17 items one
// after the other whichever lane does it, and what it waits for is the binary search of the next
// hash and the first line of that node -- a chain of dependent reads per path, not a fan-out.
// No LDS, no atomics: the kept elements land at the scanned places of the count pass.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rangeverify.h"
#include "host.h"

using namespace khst;

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

// ---------------------------------------------------------------------------
// host: range verification (rangeverify.h)
// ---------------------------------------------------------------------------
// nr ranges of ne entries in all against one node set, every input in HBM on c's stream; status,
// more and missing32 (nullable) are host arrays.  The node set is hashed and sorted as the forest
// load stages its store; the order check, the count pass of the boundary walk and the plan run
// over every range; the ranges still undecided bring their entries and kept subtrees to ONE
// segmented element build (run_build, the resident commit's), whose topology says which kept
// subtree would have moved and whose segment roots are compared with the given ones.  Host syncs:
// the store's sort (with nodes), the element total, run_build's own after its topology (with
// elements), the results; kh_dev_verify_ranges adds one before, reading ent_off[0] and ent_off[nr].
static void verify_ranges_dev(kh_ctx* c, const uint8_t* d_roots, const uint8_t* d_origins, const uint8_t* d_proved,
                              uint64_t nr, const uint8_t* d_keys, const uint8_t* d_vals, const uint64_t* d_voff,
                              const uint64_t* d_ent_off, uint64_t ne, const uint8_t* d_enc, const uint64_t* d_off,
                              uint64_t n_nodes, uint8_t* status, uint8_t* more, uint8_t* missing32) {
  hipStream_t st = c->st;
  // ---- the node set, keyed by kec256 of each encoding
  NStore NS{nullptr, nullptr, 0, d_enc, d_off};
  if (n_nodes) {
    Layout Ls;
    uint64_t* hs;
    SortIO S{};
    Ls.add(hs, n_nodes * 4 + 4);
    S.declare(Ls, n_nodes, n_nodes * 4 + 4, false, n_nodes + 1, n_nodes + 1, CTR_N);
    place(c->rv_store, Ls);
    S.K32 = hs;
    S.n = n_nodes;
    HIPCHK(hipMemsetAsync(S.ctr, 0, CTR_N * 8, st));
    hipLaunchKernelGGL(k_kec_batch, GRID(n_nodes, BS), dim3(BS), 0, st, d_enc, d_off, n_nodes, hs);
    LAUNCH_CHECK();
    sort_dedup(c, S);
    NS.hash = S.skey;
    NS.idx = S.sidx;
    NS.m = S.m;
  }
  const RvIn I{(const uint64_t*)d_roots, (const uint64_t*)d_origins, d_proved, nr, (const uint64_t*)d_keys, d_voff,
               d_ent_off, NS};
  // ---- order, the count pass of the walk, the plan
  Layout Lw;
  uint32_t *bad, *moved, *inb, *segid;
  uint64_t *cnt, *base, *dmiss, *tot;
  uint8_t *dst, *dmore;
  char* scr;
  RvWalkOut W{};
  Lw.add_all(nr, bad, moved);  // (back to back: one memset)
  Lw.add_all(2 * nr, W.st, W.cnt);
  Lw.add(W.miss, 8 * nr);
  Lw.add_all(nr + 1, cnt, base);
  Lw.add_all(nr + 1, inb, segid);
  Lw.add(dmiss, 4 * nr);
  Lw.add_all(nr, dst, dmore);
  Lw.add(scr, scan_scratch_size(nr + 1, 8));
  Lw.add(tot, 8);
  place(c->rv_ws, Lw);
  HIPCHK(hipMemsetAsync(bad, 0, (size_t)((char*)(moved + nr) - (char*)bad), st));
  HIPCHK(hipMemsetAsync(tot, 0, 64, st));
  if (ne) {
    hipLaunchKernelGGL(k_rv_order, GRID(ne, BS), dim3(BS), 0, st, I, ne, bad);
    LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_rv_walk_count, GRID(2 * nr, BS), dim3(BS), 0, st, I, (const uint32_t*)bad, W);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(k_rv_plan, GRID(nr, BS), dim3(BS), 0, st, I, (const uint32_t*)bad, W, dst, dmore, dmiss, cnt, inb);
  LAUNCH_CHECK();
  scan_u64(cnt, base, nr, tot, scr, st);
  scan_u32(inb, segid, nr, (uint32_t*)(tot + 1), scr, st);
  HIPCHK(hipMemcpyAsync(c->h_pinned, tot, 16, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  const uint64_t nel = c->h_pinned[0], nseg = (uint32_t)c->h_pinned[1];
  if (nel >= (1ULL << 31)) throw KhError{KH_EINVAL, "kh_verify_ranges: entries and kept subtrees must be < 2^31"};
  // ---- the rebuild: entries and kept subtrees of the undecided ranges, one segmented element build
  if (nel) {
    RvElems E{};
    Layout Le;
    Le.add(E.key, nel * 4);
    Le.add(E.seg, nel);
    Le.add(E.db, nel);
    Le.add(E.ref, nel * 4);
    Le.add_all(nel, E.rl, E.oldd);
    Le.add(E.vo, nel);
    Le.add(E.vl, nel);
    Le.add(E.side, nel);
    place(c->rv_el, Le);
    E.cap = nel;
    if (ne) {
      hipLaunchKernelGGL(k_rv_entries, GRID(ne, BS), dim3(BS), 0, st, I, ne, (const uint32_t*)inb, (const uint64_t*)base,
                         (const uint32_t*)segid, E);
      LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_rv_walk_fill, GRID(2 * nr, BS), dim3(BS), 0, st, I, W, (const uint32_t*)inb,
                       (const uint64_t*)base, (const uint32_t*)segid, E);
    LAUNCH_CHECK();
    ElemArgs EA{E.db, E.ref, E.rl, E.oldd, E.ref, E.rl, nullptr, &c->rv_elout, &c->rv_eloutb};
    BuildArgs A{(const uint8_t*)E.key, 32, d_vals, (const uint64_t*)E.vo, nel,
                nseg > 1 ? (const uint32_t*)E.seg : nullptr, nseg, 0, 0, false};
    A.vlen = E.vl;
    A.el = &EA;
    A.dev_results = true;
    BuildOut O;
    run_build(c, A, O, nullptr);
    const uint64_t m = c->T.m;
    if (m != nel) throw KhError{KH_EINTERNAL, "kh_verify_ranges: duplicate elements"};
    hipLaunchKernelGGL(k_rv_moved, GRID(m, BS), dim3(BS), 0, st, E, (const uint32_t*)c->T.sidx,
                       (const int8_t*)c->T.lf_pd, m, moved);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(k_rv_final, GRID(nr, BS), dim3(BS), 0, st, I, (const uint32_t*)inb, (const uint32_t*)segid,
                       (const uint32_t*)moved, (const uint64_t*)c->T.res_hash, (const uint32_t*)c->T.res_len, dst);
    LAUNCH_CHECK();
    HIPCHK(hipMemcpyAsync(c->h_pinned, c->T.ctr + CTR_ERR, 8, hipMemcpyDeviceToHost, st));
  } else {
    c->h_pinned[0] = 0;
  }
  // (the outputs are staged: an internal error writes nothing)
  std::vector<uint8_t> hst(nr), hmore(nr), hmiss(missing32 ? nr * 32 : 0);
  HIPCHK(hipMemcpyAsync(hst.data(), dst, nr, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(hmore.data(), dmore, nr, hipMemcpyDeviceToHost, st));
  if (missing32) HIPCHK(hipMemcpyAsync(hmiss.data(), dmiss, nr * 32, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (c->h_pinned[0]) throw KhError{KH_EINTERNAL, "kh_verify_ranges: the element build flagged an invariant"};
  memcpy(status, hst.data(), nr);
  memcpy(more, hmore.data(), nr);
  if (missing32) memcpy(missing32, hmiss.data(), nr * 32);
}

extern "C" {

int kh_dev_verify_ranges(kh_ctx* c, const uint8_t* d_roots32, const uint8_t* d_origins32, const uint8_t* d_proved,
                         uint64_t nr, const uint8_t* d_keys32, const uint8_t* d_vals, const uint64_t* d_voff,
                         const uint64_t* d_ent_off, const uint8_t* d_enc, const uint64_t* d_off, uint64_t n_nodes,
                         uint8_t* status, uint8_t* more, uint8_t* missing32) {
  if (nr >= (1ULL << 31) || n_nodes >= (1ULL << 31)) return set_err(KH_EINVAL, "kh_verify_ranges: batch too large");
  if (!d_ent_off || !d_voff || (nr && (!d_roots32 || !d_proved || !status || !more)) || (n_nodes && (!d_enc || !d_off)))
    return set_err(KH_EINVAL, "kh_verify_ranges: null array");
  // (roots, origins and keys are read as 64-bit words, the offsets are 64-bit words)
  if ((((uintptr_t)d_roots32 | (uintptr_t)d_origins32 | (uintptr_t)d_keys32 | (uintptr_t)d_voff | (uintptr_t)d_ent_off |
        (uintptr_t)d_off) & 7) != 0)
    return set_err(KH_EINVAL, "kh_dev_verify_ranges: roots, origins, keys and offsets must be 8-byte aligned");
  API_TRY({
    if (!c) c = shared_ctx(current_device());
    std::lock_guard<std::recursive_mutex> g(c->mu);
    HIPCHK(hipSetDevice(c->dev));
    if (nr == 0) return KH_OK;
    // the entry total: ent_off[nr] - ent_off[0] (the arrays are used from ent_off[0] on)
    uint64_t eo[2];
    HIPCHK(hipMemcpyAsync(&eo[0], d_ent_off, 8, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipMemcpyAsync(&eo[1], d_ent_off + nr, 8, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    if (eo[0] != 0) return set_err(KH_EINVAL, "kh_dev_verify_ranges: ent_off[0] must be 0");
    const uint64_t ne = eo[1];
    if (ne >= (1ULL << 31)) return set_err(KH_EINVAL, "kh_verify_ranges: batch too large");
    if (ne && !d_keys32) return set_err(KH_EINVAL, "kh_verify_ranges: null array");
    verify_ranges_dev(c, d_roots32, d_origins32, d_proved, nr, d_keys32, d_vals, d_voff, d_ent_off, ne, d_enc, d_off,
                      n_nodes, status, more, missing32);
  })
}

int kh_verify_ranges(const uint8_t* roots32, const uint8_t* origins32, const uint8_t* proved, uint64_t nr,
                     const uint8_t* keys32, const uint8_t* vals, const uint64_t* voff, const uint64_t* ent_off,
                     const uint8_t* enc, const uint64_t* off, uint64_t n_nodes, uint8_t* status, uint8_t* more,
                     uint8_t* missing32) {
  if (nr >= (1ULL << 31) || n_nodes >= (1ULL << 31)) return set_err(KH_EINVAL, "kh_verify_ranges: batch too large");
  if (!ent_off || !voff || (nr && (!roots32 || !proved || !status || !more)) || (n_nodes && (!enc || !off)))
    return set_err(KH_EINVAL, "kh_verify_ranges: null array");
  API_TRY({
    for (uint64_t s = 0; s < nr; ++s)
      if (ent_off[s + 1] < ent_off[s]) throw KhError{KH_EINVAL, "kh_verify_ranges: ent_off must not decrease"};
    const uint64_t e0 = ent_off[0], ne = ent_off[nr] - e0;
    if (ne >= (1ULL << 31)) throw KhError{KH_EINVAL, "kh_verify_ranges: batch too large"};
    if (ne && !keys32) throw KhError{KH_EINVAL, "kh_verify_ranges: null array"};
    for (uint64_t i = e0; i < e0 + ne; ++i) {
      if (voff[i + 1] < voff[i]) throw KhError{KH_EINVAL, "kh_verify_ranges: voff must not decrease"};
      if (voff[i + 1] - voff[i] > 0xFFFFFFFFull) throw KhError{KH_EINVAL, "kh_verify_ranges: a value longer than 2^32 - 1 bytes"};
    }
    for (uint64_t j = 0; j < n_nodes; ++j)
      if (off[j + 1] < off[j]) throw KhError{KH_EINVAL, "kh_verify_ranges: off must not decrease"};
    const uint64_t v0 = voff[e0], vb = voff[e0 + ne] - v0;
    const uint64_t b0 = n_nodes ? off[0] : 0, nb = n_nodes ? off[n_nodes] - b0 : 0;
    if (vb && !vals) throw KhError{KH_EINVAL, "kh_verify_ranges: null array"};
    if (nr == 0) return KH_OK;
    kh_ctx* c = shared_ctx(current_device());
    std::lock_guard<std::recursive_mutex> g(c->mu);
    HIPCHK(hipSetDevice(c->dev));
    hipStream_t st = c->st;
    // offsets rebased to zero; everything staged into one buffer
    std::vector<uint64_t> reo(nr + 1), rvo(ne + 1), rno(n_nodes + 1, 0);
    for (uint64_t s = 0; s <= nr; ++s) reo[s] = ent_off[s] - e0;
    for (uint64_t i = 0; i <= ne; ++i) rvo[i] = voff[e0 + i] - v0;
    for (uint64_t j = 0; j <= n_nodes && n_nodes; ++j) rno[j] = off[j] - b0;
    Layout Li;
    uint8_t *droots, *dorig, *dproved, *dkeys, *dvals, *denc;
    uint64_t *dvoff, *deo, *dno;
    Li.add(droots, nr * 32);
    Li.add(dorig, nr * 32, origins32 != nullptr);
    Li.add(dproved, nr);
    Li.add(dkeys, ne * 32 + 32);
    Li.add(dvals, vb + 64);
    Li.add(denc, nb + 64);
    Li.add(dvoff, ne + 1);
    Li.add(deo, nr + 1);
    Li.add(dno, n_nodes + 1);
    place(c->rv_in, Li);
    HIPCHK(hipMemcpyAsync(droots, roots32, nr * 32, hipMemcpyHostToDevice, st));
    if (origins32) HIPCHK(hipMemcpyAsync(dorig, origins32, nr * 32, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dproved, proved, nr, hipMemcpyHostToDevice, st));
    if (ne) HIPCHK(hipMemcpyAsync(dkeys, keys32 + 32 * e0, ne * 32, hipMemcpyHostToDevice, st));
    if (vb) HIPCHK(hipMemcpyAsync(dvals, vals + v0, vb, hipMemcpyHostToDevice, st));
    if (nb) HIPCHK(hipMemcpyAsync(denc, enc + b0, nb, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dvoff, rvo.data(), (ne + 1) * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(deo, reo.data(), (nr + 1) * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dno, rno.data(), (n_nodes + 1) * 8, hipMemcpyHostToDevice, st));
    verify_ranges_dev(c, droots, dorig, dproved, nr, dkeys, dvals, dvoff, deo, ne, denc, dno, n_nodes, status, more,
                      missing32);
  })
}

}  // extern "C"
