// The forest load, kh_forest_roots, kh_forest_evict and the partial handles' open, fill and need:
// their kernels (load.h holds the bodies), then the host drivers and the C entry points (host.h).
// A compilation unit of its own: a code object of its own cannot shift the placement of the hot
// kernels of khst.hip (tests/test_code_layout.py).  The kernels take the POD views and raw
// pointers, one thread per frontier node or record.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "load.h"
#include "host.h"
#include "wave.h"

using namespace khst;

// Round 0: the k listed tries' roots (hash references at anchor 0); a root equal to the empty
// trie's loads nothing.  flag[j] = 1 for a root to walk; pos: its exclusive scan.
__global__ void __launch_bounds__(BS) k_load_root_flags(const uint64_t* roots, uint64_t k, uint32_t* flag) {
  const uint64_t j = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (j >= k) return;
  const uint64_t E[4] = {0xa655cc1b171fe856ULL, 0x6ef8c092e64583ffULL, 0xc0ad6c991be0485bULL, 0x21b463e3b52f6201ULL};
  bool empty = true;
  for (int q = 0; q < 4; ++q) empty = empty && roots[4 * j + q] == E[q];
  flag[j] = empty ? 0u : 1u;
}
__global__ void __launch_bounds__(BS) k_load_roots(const uint64_t* roots, uint64_t k, const uint32_t* flag,
                                                   const uint32_t* pos, LItems N) {
  const uint64_t j = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (j >= k || !flag[j]) return;
  const uint64_t t = pos[j];
  if (t >= N.cap) return;
  for (int q = 0; q < 4; ++q) {
    N.pre[4 * t + q] = 0;
    N.ref[4 * t + q] = roots[4 * j + q];
    N.pref[4 * t + q] = roots[4 * j + q];
  }
  N.a[t] = 0;
  N.d[t] = 0;
  N.rl[t] = 32;
  N.prl[t] = 32;
  N.j[t] = (uint32_t)j;
}
// ids that already have a live record at anchor (t, 0)
__global__ void __launch_bounds__(BS) k_load_resident(AMap M, Recs R, const uint32_t* tries, uint64_t k,
                                                      unsigned long long* n_resident) {
  const uint64_t j = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (j >= k) return;
  const uint64_t zero[4] = {0, 0, 0, 0};
  const uint32_t r = map_find(M, R, tries[j], 0, zero);
  if (r != NONE && R.rlive[r] == REC_LIVE) atomicAdd(n_resident, 1ULL);
}

// Count pass of one round.  tot: [3] the largest error code met (OPEN_BAD / OPEN_VALUE; a missing
// node is counted, not an error code), [4] missing references, [5] keys (leaves and value-only
// branches) -- sums and a maximum, which do not depend on the order the threads run in.
// partial (kh_forest_load_partial below its roots, kh_trie_fill_nodes): an absent hash makes a
// stub, counted in tot[6]; tot[7]: the store nodes decoded (items referenced by hash and found).
__global__ void __launch_bounds__(BS) k_load_count(LItems I, uint64_t ni, NStore S, LCounts C,
                                                   unsigned long long* tot, int partial) {
  const uint64_t i = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (i >= ni) return;
  uint32_t is_key = 0;
  const unsigned long long code = load_count_item(I, i, S, C, &is_key, partial != 0);
  if (code == OPEN_MISSING)
    atomicAdd(tot + 4, 1ULL);
  else if (code != OPEN_OK)
    atomicMax(tot + 3, code);
  if (is_key) atomicAdd(tot + 5, 1ULL);
  if (partial && code == OPEN_OK && I.rl[i] == 32) atomicAdd(C.src[i] == NONE ? tot + 6 : tot + 7, 1ULL);
}
// Fill pass: C holds the scanned counts.
__global__ void __launch_bounds__(BS) k_load_fill(LItems I, uint64_t ni, NStore S, LCounts C, LItems N,
                                                  const uint32_t* tries, uint8_t* recs, uint64_t rbase, uint64_t rcap,
                                                  uint8_t* heap, uint64_t hbase, uint64_t heap_cap, int partial) {
  const uint64_t i = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (i >= ni) return;
  load_fill_item(I, i, S, C, N, tries, recs, rbase, rcap, heap, hbase, heap_cap, partial != 0);
}
// The missing references of a round, one entry per reference, at the scan of the miss flags
// (the first cap of them): the list index of the trie and the hash.
__global__ void __launch_bounds__(BS) k_load_missing(LItems I, uint64_t ni, const uint32_t* miss, const uint32_t* mpos,
                                                     uint64_t cap, uint32_t* out_idx, uint64_t* out_hash) {
  const uint64_t i = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (i >= ni || !miss[i]) return;
  const uint64_t t = mpos[i];
  if (t >= cap) return;
  out_idx[t] = I.j[i];
  for (int q = 0; q < 4; ++q) out_hash[4 * t + q] = I.ref[4 * i + q];
}

// kh_forest_roots: flag the root records, then write (trie id, root hash) at the scanned places
__global__ void __launch_bounds__(BS) k_roots_flags(Recs R, uint64_t n, uint32_t* flag) {
  const uint64_t r = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (r >= n) return;
  flag[r] = load_is_root(R, r) ? 1u : 0u;
}
__global__ void __launch_bounds__(BS) k_roots_write(Recs R, uint64_t n, const uint32_t* flag, const uint32_t* pos,
                                                    uint64_t cap, uint32_t* tries, uint64_t* roots) {
  const uint64_t r = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (r >= n || !flag[r]) return;
  const uint64_t t = pos[r];
  if (t >= cap) return;
  tries[t] = R.rt[r];
  for (int q = 0; q < 4; ++q) roots[4 * t + q] = R.rref[4 * r + q];
}

// kh_forest_evict: flag the live records of the nt sorted trie ids (cnt[0]: those holding a key,
// cnt[1]: the root records, i.e. the tries met, cnt[2]: the stubs), then list them at the scanned
// places
__global__ void __launch_bounds__(BS) k_evict_flags(Recs R, uint64_t n, const uint32_t* tries, uint32_t nt,
                                                    uint32_t* flag, unsigned long long* cnt) {
  const uint64_t r = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (r >= n) return;
  const bool in = load_in_list(R, r, tries, nt);
  flag[r] = in ? 1u : 0u;
  if (in && load_holds_key(R, r)) atomicAdd(cnt, 1ULL);
  if (in && R.rd[r] == 0) atomicAdd(cnt + 1, 1ULL);
  if (in && load_is_stub(R, r)) atomicAdd(cnt + 2, 1ULL);  // (a stub goes with its trie)
}
__global__ void __launch_bounds__(BS) k_evict_list(uint64_t n, const uint32_t* flag, const uint32_t* pos, uint64_t cap,
                                                   uint32_t* list) {
  const uint64_t r = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (r >= n || !flag[r]) return;
  if (pos[r] < cap) list[pos[r]] = (uint32_t)r;
}

// kh_trie_evict_subtrees (load.h): the probe, one thread a listed prefix ...
__global__ void __launch_bounds__(BS) k_evsub_probe(AMap M, Recs R, EvictList P, uint8_t* status, uint64_t* hash,
                                                    uint32_t* rec, uint8_t* is_key) {
  const uint64_t i = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (i >= P.m) return;
  uint64_t h[4];
  status[i] = evict_probe(M, R, P.trie[i], P.depth[i], P.path + 4 * i, rec + i, h, is_key + i);
  for (int q = 0; q < 4; ++q) hash[4 * i + q] = h[q];
}
// ... the flags of the records below an evicted prefix, one thread a record reading its first line
// (cnt[0]: those holding a key, cnt[1]: the stubs; a wave reduction and one atomic a wave; the list
// comes from the flags' scan through k_evict_list) ...
__global__ void __launch_bounds__(BS) k_evsub_flags(Recs R, uint64_t n, EvictList E, uint32_t* flag,
                                                    unsigned long long* cnt) {
  const uint64_t r = (uint64_t)blockIdx.x * BS + threadIdx.x;
  const bool in = r < n && evict_covers(R, r, E);
  if (r < n) flag[r] = in ? 1u : 0u;
  unsigned long long keys = (in && load_holds_key(R, r)) ? 1 : 0, stubs = (in && R.rdb[r] == EL_STUB) ? 1 : 0;
  keys = wave_sum(keys);
  stubs = wave_sum(stubs);
  if ((threadIdx.x & 63) == 0) {
    if (keys) atomicAdd(cnt, keys);
    if (stubs) atomicAdd(cnt + 1, stubs);
  }
}
// ... and the anchors' records rewritten as stubs
__global__ void __launch_bounds__(BS) k_evsub_stub(Recs R, const uint32_t* rec, const uint8_t* depth, uint64_t m,
                                                   uint64_t rn) {
  const uint64_t i = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (i >= m || rec[i] >= rn) return;
  evict_stub_record(R, rec[i], depth[i]);
}

// ---- partial handles (forest.h EL_STUB).  All of these run only on a handle that holds stubs, or
// on the refusal path of a commit; one thread per record, op or element, no LDS, no loop over
// anything but a map probe or a binary search.

// kh_trie_fill_nodes, round 0: flag the live stubs whose missing node (rbref) is in the store ...
__global__ void __launch_bounds__(BS) k_fill_flags(Recs R, uint64_t n, NStore S, uint32_t* flag) {
  const uint64_t r = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (r >= n) return;
  bool hit = false;
  if (load_is_stub(R, r) && S.m) {
    uint64_t h[4];
    for (int q = 0; q < 4; ++q) h[q] = R.rbref[4 * r + q];
    const uint64_t p = key_lower_bound(S.hash, S.m, h);
    hit = p < S.m && key_cmp(S.hash + 4 * p, h) == 0;
  }
  flag[r] = hit ? 1u : 0u;
}
// ... and make each one a frontier item at its scanned place t (record order: a fixed order); the
// item is its own entry of the call's trie list (tries[t]), list[t] the stub to swap out at the end
__global__ void __launch_bounds__(BS) k_fill_items(Recs R, uint64_t n, const uint32_t* flag, const uint32_t* pos,
                                                   LItems N, uint32_t* tries, uint32_t* list) {
  const uint64_t r = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (r >= n || !flag[r]) return;
  const uint64_t t = pos[r];
  if (t >= N.cap) return;
  load_stub_item(R, r, N, t, (uint32_t)t);
  tries[t] = R.rt[r];
  list[t] = (uint32_t)r;
}

// A refused commit: the stubs among the n records its descent marked (each is listed once), as
// (trie id, hash to fetch = rbref) at claimed places; cnt counts them all, the first cap are written.
__global__ void __launch_bounds__(BS) k_stub_missing(Recs R, const uint32_t* list, uint64_t n, uint64_t cap,
                                                     uint32_t* out_trie, uint64_t* out_hash,
                                                     unsigned long long* cnt) {
  const uint64_t i = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (i >= n) return;
  const uint32_t r = list[i];
  if (!load_is_stub(R, r)) return;
  const unsigned long long t = atomicAdd(cnt, 1ULL);
  if (t >= cap) return;
  out_trie[t] = R.rt[r];
  for (int q = 0; q < 4; ++q) out_hash[4 * t + q] = R.rbref[4ull * r + q];
}
// After the element topology, before the commit writes anything: a stub element whose anchor
// would move (sorted element i hangs at pd[i] + 1, its record at oldd) is a node the reference's
// fix would load (MerklePatriciaTrie.scala:430-477); listed like the ones above.  A missing branch
// under a present extension (STUB_BRANCH) moves freely: fix re-cuts the extension without its branch.
__global__ void __launch_bounds__(BS) k_stub_moved(Recs R, const uint32_t* sidx, const int8_t* pd, const uint32_t* src,
                                                   const uint8_t* oldd, uint64_t m, uint64_t cap, uint32_t* out_trie,
                                                   uint64_t* out_hash, unsigned long long* cnt) {
  const uint64_t i = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (i >= m) return;
  const uint32_t s = sidx[i], r = src[s];
  if (r == NONE || !load_is_stub(R, r) || (R.rmask[r] & STUB_BRANCH)) return;
  if ((uint32_t)(pd[i] + 1) == (uint32_t)oldd[s]) return;
  const unsigned long long t = atomicAdd(cnt, 1ULL);
  if (t >= cap) return;
  out_trie[t] = R.rt[r];
  for (int q = 0; q < 4; ++q) out_hash[4 * t + q] = R.rbref[4ull * r + q];
}
// kh_trie_need_host: the stub key o's walk reaches (flag 1, its rbref), or flag 0
__global__ void __launch_bounds__(BS) k_need(AMap M, Recs R, const uint64_t* K, const uint32_t* trie, uint64_t n,
                                             uint8_t* flag, uint64_t* hash) {
  const uint64_t o = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (o >= n) return;
  const uint32_t r = forest_get(M, R, trie ? trie[o] : 0u, K + 4 * o);
  const bool stub = r != NONE && R.rdb[r] == EL_STUB;
  flag[o] = stub ? 1 : 0;
  for (int q = 0; q < 4; ++q) hash[4 * o + q] = stub ? R.rbref[4ull * r + q] : 0;
}

// ---------------------------------------------------------------------------
// host: forest load, roots and eviction, partial handles (load.h)
// ---------------------------------------------------------------------------
static LItems litems_carve(DevBuf& b, uint64_t cap) {
  Layout L;
  LItems I{};
  L.add(I.pre, cap * 4);
  L.add_all(cap, I.a, I.d);
  L.add(I.ref, cap * 4);
  L.add(I.rl, cap);
  L.add(I.pref, cap * 4);
  L.add(I.prl, cap);
  L.add(I.j, cap);
  place(b, L);
  I.cap = cap;
  return I;
}

// k tries (ids tries[j], roots roots32[32j..), host arrays) decoded from n stored node encodings
// (device buffers) into forest h, beside what it holds.  All or nothing: a refusal or failure
// before the anchor map is touched leaves no record past the old count (the slots cleared) and
// every host-side field as it was.  With a savepoint open the map inserts are journaled.
// A single trie opens the same way (open_store): trie id 0 into a fresh non-forest handle.
//
// mode LOAD_PARTIAL (kh_forest_load_partial, kh_trie_open_partial): a hash absent from the store
// below a root makes a stub (forest.h EL_STUB) instead of ending the round; a missing root is
// reported as ever.  mode LOAD_FILL (kh_trie_fill_nodes; tries, roots32, k unused): round 0 is the
// live stubs whose missing node the store holds, in record order; the rounds append as a partial
// load does, and only after the last one do the listed stubs leave the map and die, the new
// records taking their anchors -- so a failure before that leaves the handle as it was.
enum LoadMode { LOAD_FULL = 0, LOAD_PARTIAL = 1, LOAD_FILL = 2 };
static void forest_load(kh_trie* h, const uint32_t* tries, const uint8_t* roots32, uint64_t k, const uint8_t* d_enc,
                        const uint64_t* d_off, uint64_t n, uint32_t* miss_idx, uint8_t* miss32, uint64_t miss_cap,
                        uint64_t* n_missing, kh_stats* stats, LoadMode mode = LOAD_FULL,
                        uint64_t* n_decoded = nullptr) {
  kh_ctx* c = h->c;
  hipStream_t st = c->st;
  if (stats) memset(stats, 0, sizeof(*stats));
  const bool fill = mode == LOAD_FILL;
  if (fill) k = 0;
  if (k >= (1ULL << 31) || n >= (1ULL << 31)) throw KhError{KH_EINVAL, "trie list or node store too large"};
  if (fill && !h->sps.empty()) throw KhError{KH_EINVAL, "kh_trie_fill_nodes: a savepoint is open"};
  if (!fill) {
    std::vector<uint32_t> ids(tries, tries + k);
    std::sort(ids.begin(), ids.end());
    if (std::adjacent_find(ids.begin(), ids.end()) != ids.end())
      throw KhError{KH_EINVAL, "kh_forest_load_nodes: a trie id is listed twice"};
  }
  trie_settle(h);
  if (fill ? (h->nstubs == 0 || n == 0 || h->rn == 0) : k == 0) {
    ++h->epoch;
    return;
  }
  HIPCHK(hipEventRecord(c->ev[6], st));
  const uint64_t nscan = fill ? h->rn : 0;  // fill: the records scanned for stubs
  // the list on the device, the roots to walk (not the empty trie's) and the resident check
  Layout Lr;
  uint32_t *dtries, *rflag, *rpos, *dmidx;
  uint64_t *droots, *dmhash;
  unsigned long long* tot;
  char* rscr;
  const uint64_t mcap = std::min<uint64_t>(miss_cap, 1ULL << 24);
  const uint64_t kk = fill ? nscan : k;  // (fill: a list entry per stub found, at most one per record)
  uint32_t* slist = nullptr;            // fill: the stubs of round 0
  Lr.add(dtries, kk);
  Lr.add(droots, k * 4);
  Lr.add_all(kk, rflag, rpos);
  Lr.add(rscr, scan_scratch_size(kk + 1, 4));
  Lr.add(tot, 8);
  Lr.add(dmidx, mcap + 1);
  Lr.add(dmhash, (mcap + 1) * 4);
  Lr.add(slist, nscan);
  place(h->gbuf, Lr);
  if (!fill) {
    HIPCHK(hipMemcpyAsync(dtries, tries, k * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(droots, roots32, k * 32, hipMemcpyHostToDevice, st));
  }
  HIPCHK(hipMemsetAsync(tot, 0, 64, st));
  uint64_t ni = 0;
  uint32_t max_id = 0;
  if (!fill) {
    if (h->rn && h->mcap) {
      hipLaunchKernelGGL(k_load_resident, GRID(k, BS), dim3(BS), 0, st, map_of(h), recs_of(h), (const uint32_t*)dtries,
                         k, tot + 6);
      LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_load_root_flags, GRID(k, BS), dim3(BS), 0, st, (const uint64_t*)droots, k, rflag);
    LAUNCH_CHECK();
    scan_u32(rflag, rpos, k, (uint32_t*)tot, rscr, st);
    HIPCHK(hipMemcpyAsync(c->h_pinned, tot, 64, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (c->h_pinned[6]) throw KhError{KH_EINVAL, "kh_forest_load_nodes: a listed trie is already resident"};
    ni = (uint32_t)c->h_pinned[0];
    for (uint64_t j = 0; j < k; ++j) max_id = std::max(max_id, tries[j]);
    if (ni == 0) {  // every root is the empty trie's
      ++h->epoch;
      return;
    }
  }
  // the store, keyed by kec256 of each encoding (content addressed)
  Layout L;
  uint64_t* hs;
  SortIO S{};
  L.add(hs, n * 4 + 4);
  S.declare(L, n, n * 4 + 4, false, n + 1, n + 1, CTR_N);
  place(h->ws, L);
  S.K32 = hs;
  S.n = n;
  HIPCHK(hipMemsetAsync(S.ctr, 0, CTR_N * 8, st));
  NStore NS{nullptr, nullptr, 0, d_enc, d_off};
  if (n) {
    hipLaunchKernelGGL(k_kec_batch, GRID(n, BS), dim3(BS), 0, st, d_enc, d_off, n, hs);
    LAUNCH_CHECK();
    sort_dedup(c, S);
    NS.hash = S.skey;
    NS.idx = S.sidx;
    NS.m = S.m;
  }
  HIPCHK(hipEventRecord(c->ev[0], st));  // (stats: the store is hashed and sorted)
  const uint64_t rn0 = h->rn;
  uint64_t heap_cur = h->heap_n, keys = 0, stubs_made = 0, decoded = 0, nfilled = 0;
  uint32_t rounds = 0;
  bool map_stage = false;
  try {
    DevBuf fa, fb, cb;
    LItems cur{};
    if (fill) {  // round 0: the stubs the store resolves, in record order
      hipLaunchKernelGGL(k_fill_flags, GRID(nscan, BS), dim3(BS), 0, st, recs_of(h), nscan, NS, rflag);
      LAUNCH_CHECK();
      scan_u32(rflag, rpos, nscan, (uint32_t*)tot, rscr, st);
      HIPCHK(hipMemcpyAsync(c->h_pinned, tot, 8, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      ni = nfilled = (uint32_t)c->h_pinned[0];
      if (ni == 0) {  // no stub names a node of the store: nothing to do
        ++h->epoch;
        if (n_decoded) *n_decoded = 0;
        return;
      }
      cur = litems_carve(fa, ni);
      hipLaunchKernelGGL(k_fill_items, GRID(nscan, BS), dim3(BS), 0, st, recs_of(h), nscan, (const uint32_t*)rflag,
                         (const uint32_t*)rpos, cur, dtries, slist);
      LAUNCH_CHECK();
    } else {
      cur = litems_carve(fa, ni);
      hipLaunchKernelGGL(k_load_roots, GRID(k, BS), dim3(BS), 0, st, (const uint64_t*)droots, k,
                         (const uint32_t*)rflag, (const uint32_t*)rpos, cur);
      LAUNCH_CHECK();
    }
    for (; ni && rounds < 80; ++rounds) {
      // (a root is never a stub: round 0 of a partial load reports a missing root as the full load does)
      const int partial = fill || (mode == LOAD_PARTIAL && rounds > 0);
      // count, scans, one sync
      Layout Lc;
      LCounts C{};
      uint32_t* mpos;
      char* scr;
      Lc.add_all(ni, C.child, C.rec);
      Lc.add(C.val, ni);
      Lc.add_all(ni, C.miss, C.src, mpos);
      Lc.add(scr, scan_scratch_size(ni + 1, 8));
      place(cb, Lc);
      HIPCHK(hipMemsetAsync(tot, 0, 64, st));
      hipLaunchKernelGGL(k_load_count, GRID(ni, BS), dim3(BS), 0, st, cur, ni, NS, C, tot, partial);
      LAUNCH_CHECK();
      scan_u32(C.child, C.child, ni, (uint32_t*)tot, scr, st);
      scan_u32(C.rec, C.rec, ni, (uint32_t*)(tot + 1), scr, st);
      scan_u64(C.val, C.val, ni, (uint64_t*)(tot + 2), scr, st);
      HIPCHK(hipMemcpyAsync(c->h_pinned, tot, 64, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      const uint64_t nchild = (uint32_t)c->h_pinned[0], nrec = (uint32_t)c->h_pinned[1], nval = c->h_pinned[2];
      const uint64_t code = c->h_pinned[3], nmiss = c->h_pinned[4];
      keys += c->h_pinned[5];
      stubs_made += c->h_pinned[6];
      decoded += c->h_pinned[7];
      if (code == OPEN_VALUE) throw KhError{KH_EINVAL, "a branch with a value: not a secure trie"};
      if (code) throw KhError{KH_EINVAL, "the store holds a node that is not a canonical secure-trie node"};
      if (nmiss) {  // every missing reference of this round (MPTNodeMissingException), then stop
        const uint64_t w = std::min(nmiss, mcap);
        if (w) {
          scan_u32(C.miss, mpos, ni, (uint32_t*)(tot + 7), scr, st);
          hipLaunchKernelGGL(k_load_missing, GRID(ni, BS), dim3(BS), 0, st, cur, ni, (const uint32_t*)C.miss,
                             (const uint32_t*)mpos, w, dmidx, dmhash);
          LAUNCH_CHECK();
          HIPCHK(hipMemcpyAsync(miss_idx, dmidx, w * 4, hipMemcpyDeviceToHost, st));
          HIPCHK(hipMemcpyAsync(miss32, dmhash, w * 32, hipMemcpyDeviceToHost, st));
          HIPCHK(hipStreamSynchronize(st));
        }
        if (n_missing) *n_missing = nmiss;
        throw KhError{KH_ENODE, "node missing from the store (MPTNodeMissingException)"};
      }
      if (h->rn + nrec >= (uint64_t)NONE) throw KhError{KH_EINVAL, "the load passes the forest's record limit"};
      // fill: the records, the values and the next frontier at exactly the scanned sizes
      recs_reserve(h, h->rn + nrec + 16);
      const uint64_t hneed = heap_cur + nval + 64;
      if (hneed > h->heap.cap) regrow(h->heap, heap_cur, hneed + hneed / 4, st);
      LItems nxt = litems_carve(rounds & 1 ? fa : fb, std::max<uint64_t>(nchild, 1));
      hipLaunchKernelGGL(k_load_fill, GRID(ni, BS), dim3(BS), 0, st, cur, ni, NS, C, nxt, (const uint32_t*)dtries,
                         (uint8_t*)h->recs.p, h->rn, h->rcap, (uint8_t*)h->heap.p, heap_cur, (uint64_t)h->heap.cap,
                         partial);
      LAUNCH_CHECK();
      h->rn += nrec;  // (a later regrow keeps the records of the earlier rounds)
      heap_cur += nval;
      cur = nxt;
      ni = nchild;
    }
    if (ni) throw KhError{KH_EINVAL, "node store deeper than a 32-byte key allows"};
    // the anchor map: only the new records enter it; rebuilt when it would pass half load
    const uint64_t nnew = h->rn - rn0;
    HIPCHK(hipEventRecord(c->ev[1], st));  // (stats: the rounds are done)
    map_stage = true;
    if (fill) {  // the resolved stubs leave the map and die; the new records take their anchors below
      hipLaunchKernelGGL(k_map_delete, GRID(nfilled, BS), dim3(BS), 0, st, map_of(h), recs_of(h),
                         (const uint32_t*)slist, nfilled, (const uint32_t*)nullptr, (uint64_t)0,
                         (uint32_t*)h->touched.p, (uint8_t*)h->replaced.p, (uint64_t*)nullptr);
      LAUNCH_CHECK();
      h->rdead += nfilled;
    }
    if (h->mcap == 0 || 2 * (h->mused + nnew + 1024) > h->mcap) {
      map_rebuild(h, 1024);  // (syncs; with a savepoint open its map_epoch bump is the journal entry)
    } else if (nnew) {
      uint64_t* ilog = nullptr;
      if (!h->sps.empty()) {  // journal: no saved records, the inserts' slot log
        JSeg js = journal_reserve(h, 0, nnew);
        js.dpos = js.ipos = h->jmap_n;
        js.dn = 0;
        js.in = nnew;
        ilog = (uint64_t*)h->jmap.p + 3 * js.ipos;
        h->jsegs.push_back(js);
        h->jmap_n += nnew;
      }
      h->merr.ensure(64);
      unsigned long long* err = (unsigned long long*)h->merr.p;
      HIPCHK(hipMemsetAsync(err, 0, 16, st));
      hipLaunchKernelGGL(k_map_insert, GRID(nnew, BS), dim3(BS), 0, st, map_of(h), recs_of(h), rn0, nnew,
                         (const uint32_t*)nullptr, (uint64_t)0, err, err + 1, ilog);
      LAUNCH_CHECK();
      HIPCHK(hipMemcpyAsync(c->h_pinned, err, 16, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      if (c->h_pinned[0]) throw KhError{KH_EINTERNAL, "anchor map insert failed"};
      h->mused += c->h_pinned[1];
    }
  } catch (...) {
    if (map_stage) {
      h->broken = true;  // the map may hold part of the load: only a rollback or a free from here
    } else {
      if (h->rn > rn0) {
        (void)hipMemsetAsync((uint8_t*)h->recs.p + rn0 * REC_BYTES, 0, (h->rn - rn0) * REC_BYTES, st);
        (void)hipStreamSynchronize(st);
      }
      h->rn = rn0;
    }
    throw;
  }
  h->heap_n = heap_cur;
  h->nleaves += keys;
  h->nstubs = h->nstubs + stubs_made - nfilled;
  if (n_decoded) *n_decoded = decoded;
  if (!fill) h->tid_bits = std::max(h->tid_bits, std::min(bits_for((uint64_t)max_id + 1) + 2, 32u));
  ++h->epoch;
  HIPCHK(hipEventRecord(c->ev[7], st));
  HIPCHK(hipEventSynchronize(c->ev[7]));
  if (stats) {
    stats->n_inputs = k;
    stats->n_leaves = h->nleaves;
    stats->n_levels = rounds;
    stats->n_node_hashes = n;
    stats->t_total_ms = ev_ms(c->ev[6], c->ev[7]);
    stats->t_sort_ms = ev_ms(c->ev[6], c->ev[0]);    // list checks, store hashing and sort
    stats->t_branch_ms = ev_ms(c->ev[0], c->ev[1]);  // the rounds
    stats->t_topo_ms = ev_ms(c->ev[1], c->ev[7]);    // the anchor map
  }
}

// every trie the forest holds, ascending ids, with its root (read-only on the handle)
static int forest_roots(kh_trie* h, uint32_t* h_tries, uint8_t* h_roots32, uint64_t cap, uint64_t* n_tries) {
  trie_settle(h);
  kh_ctx* c = h->c;
  hipStream_t st = c->st;
  const uint64_t n = h->rn;
  *n_tries = 0;
  if (n == 0) return KH_OK;
  Layout L;
  uint32_t *flag, *pos, *tot;
  char* scr;
  L.add_all(n, flag, pos);
  L.add(scr, scan_scratch_size(n + 1, 4));
  L.add(tot, 4);
  place(h->gbuf, L);
  const Recs R = recs_of(h);
  hipLaunchKernelGGL(k_roots_flags, GRID(n, BS), dim3(BS), 0, st, R, n, flag);
  LAUNCH_CHECK();
  scan_u32(flag, pos, n, tot, scr, st);
  HIPCHK(hipMemcpyAsync(c->h_pinned, tot, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  const uint64_t nt = (uint32_t)c->h_pinned[0];
  *n_tries = nt;
  if (nt > cap || (nt && (!h_tries || !h_roots32))) return set_err(KH_ENOSPC, "trie output too small");
  if (nt == 0) return KH_OK;
  Layout Lo;
  uint32_t* dt;
  uint64_t* dr;
  Lo.add(dt, nt);
  Lo.add(dr, nt * 4);
  place(h->xbuf, Lo);
  hipLaunchKernelGGL(k_roots_write, GRID(n, BS), dim3(BS), 0, st, R, n, (const uint32_t*)flag, (const uint32_t*)pos, nt,
                     dt, dr);
  LAUNCH_CHECK();
  std::vector<uint32_t> t(nt), order(nt);
  std::vector<uint8_t> r(nt * 32);
  HIPCHK(hipMemcpyAsync(t.data(), dt, nt * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(r.data(), dr, nt * 32, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  for (uint64_t i = 0; i < nt; ++i) order[i] = (uint32_t)i;
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return t[a] < t[b]; });
  for (uint64_t i = 0; i < nt; ++i) {
    h_tries[i] = t[order[i]];
    memcpy(h_roots32 + 32 * i, r.data() + 32ull * order[i], 32);
  }
  return KH_OK;
}

// drop whole tries: their live records listed (a scan: record order), out of the map, dead
static void forest_evict(kh_trie* h, const uint32_t* tries, uint64_t k, uint64_t* n_evicted) {
  if (!h->sps.empty()) throw KhError{KH_EINVAL, "kh_forest_evict: a savepoint is open"};
  trie_settle(h);
  kh_ctx* c = h->c;
  hipStream_t st = c->st;
  *n_evicted = 0;
  const uint64_t n = h->rn;
  if (k == 0 || n == 0 || h->mcap == 0) return;
  if (k >= (1ULL << 31)) throw KhError{KH_EINVAL, "trie list too large"};
  std::vector<uint32_t> ids(tries, tries + k);
  std::sort(ids.begin(), ids.end());
  ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
  const uint64_t nt = ids.size();
  Layout L;
  uint32_t *dt, *flag, *pos, *list;
  unsigned long long* tot;
  char* scr;
  L.add(dt, nt);
  L.add_all(n, flag, pos, list);
  L.add(scr, scan_scratch_size(n + 1, 4));
  L.add(tot, 8);
  place(h->gbuf, L);
  const Recs R = recs_of(h);
  HIPCHK(hipMemcpyAsync(dt, ids.data(), nt * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(tot, 0, 64, st));
  hipLaunchKernelGGL(k_evict_flags, GRID(n, BS), dim3(BS), 0, st, R, n, (const uint32_t*)dt, (uint32_t)nt, flag,
                     tot + 1);
  LAUNCH_CHECK();
  scan_u32(flag, pos, n, (uint32_t*)tot, scr, st);
  HIPCHK(hipMemcpyAsync(c->h_pinned, tot, 64, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));  // (ids is a host temporary)
  const uint64_t nl = (uint32_t)c->h_pinned[0], nkeys = c->h_pinned[1], ntries = c->h_pinned[2];
  const uint64_t nstub = c->h_pinned[3];
  if (nl == 0) return;
  ++h->epoch;
  hipLaunchKernelGGL(k_evict_list, GRID(n, BS), dim3(BS), 0, st, n, (const uint32_t*)flag, (const uint32_t*)pos, nl,
                     list);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(k_map_delete, GRID(nl, BS), dim3(BS), 0, st, map_of(h), R, (const uint32_t*)list, nl,
                     (const uint32_t*)nullptr, (uint64_t)0, (uint32_t*)h->touched.p, (uint8_t*)h->replaced.p,
                     (uint64_t*)nullptr);
  LAUNCH_CHECK();
  HIPCHK(hipStreamSynchronize(st));
  h->rdead += nl;
  h->nleaves -= nkeys;
  h->nstubs -= nstub;
  *n_evicted = ntries;
}

// subtrees back to stubs (kh_trie_evict_subtrees): every refusal is decided on the host before
// anything changes; the probe reads, and only the delete and the stub rewrite write
static void evict_subtrees(kh_trie* h, const uint32_t* tries, const uint8_t* paths32, const uint8_t* depths,
                           uint64_t n, uint8_t* status, uint8_t* hashes32, uint64_t out[3]) {
  out[0] = out[1] = out[2] = 0;
  if (!h->sps.empty()) throw KhError{KH_EINVAL, "kh_trie_evict_subtrees: a savepoint is open"};
  if (n >= (1ULL << 31)) throw KhError{KH_EINVAL, "prefix list too large"};
  for (uint64_t i = 0; i < n; ++i)
    if (depths[i] == 0 || depths[i] > 64)
      throw KhError{KH_EINVAL, "kh_trie_evict_subtrees: a depth of 0 (a root is never a stub) or above 64"};
  // the list sorted by (trie, zero-padded path, depth): a prefix that equals or extends another
  // shows between neighbours
  std::vector<uint64_t> pw(n * 4);
  std::vector<uint32_t> order(n);
  for (uint64_t i = 0; i < n; ++i) {
    uint64_t w[4];
    words_of(paths32 + 32 * i, 32, w);
    for (int q = 0; q < 4; ++q) pw[4 * i + q] = prefix_word(w, depths[i], q);
    order[i] = (uint32_t)i;
  }
  auto trie_of = [&](uint32_t i) { return h->forest ? tries[i] : 0u; };
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
    if (trie_of(a) != trie_of(b)) return trie_of(a) < trie_of(b);
    const int c = key_cmp(&pw[4ull * a], &pw[4ull * b]);
    if (c) return c < 0;
    return depths[a] != depths[b] ? depths[a] < depths[b] : a < b;
  });
  for (uint64_t s = 0; s + 1 < n; ++s) {
    const uint32_t a = order[s], b = order[s + 1];
    if (trie_of(a) == trie_of(b) && prefix_eq(&pw[4ull * a], &pw[4ull * b], std::min(depths[a], depths[b])))
      throw KhError{KH_EINVAL, "kh_trie_evict_subtrees: a listed prefix equals or extends another"};
  }
  trie_settle(h);
  if (n == 0) return;
  memset(status, EVICT_NONE, n);
  memset(hashes32, 0, n * 32);
  const uint64_t rn = h->rn;
  if (rn == 0 || h->mcap == 0) return;
  kh_ctx* c = h->c;
  hipStream_t st = c->st;
  // the probe, in sorted order; the DONE prefixes keep that order as the flag pass's list
  std::vector<uint32_t> ht(n);
  std::vector<uint64_t> hp(n * 4);
  std::vector<uint8_t> hd(n);
  for (uint64_t s = 0; s < n; ++s) {
    ht[s] = trie_of(order[s]);
    hd[s] = depths[order[s]];
    memcpy(&hp[4 * s], &pw[4ull * order[s]], 32);
  }
  Layout L;
  uint32_t *dt, *drec, *flag, *pos, *list;
  uint64_t *dp, *dhash;
  uint8_t *dd, *dstat, *dkey;
  unsigned long long* tot;
  char* scr;
  L.add_all(n, dt, drec);
  L.add_all(n * 4, dp, dhash);
  L.add_all(n, dd, dstat, dkey);
  L.add_all(rn, flag, pos, list);
  L.add(scr, scan_scratch_size(rn + 1, 4));
  L.add(tot, 8);
  place(h->gbuf, L);
  const Recs R = recs_of(h);
  HIPCHK(hipMemcpyAsync(dt, ht.data(), n * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(dp, hp.data(), n * 32, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(dd, hd.data(), n, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_evsub_probe, GRID(n, BS), dim3(BS), 0, st, map_of(h), R, EvictList{dt, dp, dd, n}, dstat, dhash,
                     drec, dkey);
  LAUNCH_CHECK();
  std::vector<uint8_t> sstat(n), skey(n);
  std::vector<uint32_t> srec(n);
  std::vector<uint64_t> shash(n * 4);
  HIPCHK(hipMemcpyAsync(sstat.data(), dstat, n, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(skey.data(), dkey, n, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(srec.data(), drec, n * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(shash.data(), dhash, n * 32, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  uint64_t m = 0, akeys = 0;
  for (uint64_t s = 0; s < n; ++s) {
    status[order[s]] = sstat[s];
    memcpy(hashes32 + 32ull * order[s], &shash[4 * s], 32);
    if (sstat[s] != EVICT_DONE) continue;
    ht[m] = ht[s];  // (m <= s: compacted in place, the order kept)
    hd[m] = hd[s];
    srec[m] = srec[s];
    memmove(&hp[4 * m], &hp[4 * s], 32);
    akeys += skey[s];
    ++m;
  }
  if (m == 0) return;
  ++h->epoch;  // (an export cursor ends)
  HIPCHK(hipMemcpyAsync(dt, ht.data(), m * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(dp, hp.data(), m * 32, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(dd, hd.data(), m, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(drec, srec.data(), m * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(tot, 0, 64, st));
  hipLaunchKernelGGL(k_evsub_flags, GRID(rn, BS), dim3(BS), 0, st, R, rn, EvictList{dt, dp, dd, m}, flag, tot + 1);
  LAUNCH_CHECK();
  scan_u32(flag, pos, rn, (uint32_t*)tot, scr, st);
  HIPCHK(hipMemcpyAsync(c->h_pinned, tot, 64, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));  // (the host vectors are read by now)
  const uint64_t nl = (uint32_t)c->h_pinned[0], nkeys = c->h_pinned[1] + akeys, nstub = c->h_pinned[2];
  try {
    if (nl) {
      hipLaunchKernelGGL(k_evict_list, GRID(rn, BS), dim3(BS), 0, st, rn, (const uint32_t*)flag, (const uint32_t*)pos,
                         nl, list);
      LAUNCH_CHECK();
      hipLaunchKernelGGL(k_map_delete, GRID(nl, BS), dim3(BS), 0, st, map_of(h), R, (const uint32_t*)list, nl,
                         (const uint32_t*)nullptr, (uint64_t)0, (uint32_t*)h->touched.p, (uint8_t*)h->replaced.p,
                         (uint64_t*)nullptr);
      LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_evsub_stub, GRID(m, BS), dim3(BS), 0, st, R, (const uint32_t*)drec, (const uint8_t*)dd, m, rn);
    LAUNCH_CHECK();
    HIPCHK(hipStreamSynchronize(st));
  } catch (...) {
    h->broken = true;  // the map may hold part of the eviction: only a free from here
    throw;
  }
  h->rdead += nl;
  h->nleaves -= nkeys;
  h->nstubs = h->nstubs + m - nstub;
  out[0] = m;
  out[1] = nkeys;
  out[2] = nl;
}

// a host node store into the context's staging buffers (in_vals, in_voff), checked first:
// KH_EINVAL before anything is staged
static int stage_store(kh_ctx* c, const uint8_t* enc, const uint64_t* off, uint64_t n) {
  if (n && !off) return set_err(KH_EINVAL, "null buffer");
  if (n >= (1ULL << 31)) return set_err(KH_EINVAL, "node store too large");
  for (uint64_t i = 0; i < n; ++i)
    if (off[i + 1] < off[i]) return set_err(KH_EINVAL, "node offsets must not decrease");
  if (n && off[n] > off[0] && !enc) return set_err(KH_EINVAL, "null buffer");
  std::vector<uint64_t> rel;
  stage_packed(c, enc, off, n, rel);
  HIPCHK(hipStreamSynchronize(c->st));
  return KH_OK;
}

// A single trie opened from (root hash, node store on the device): the forest load of the one
// trie id 0 into a fresh non-forest handle.  LOAD_FULL is kh_trie_open_nodes, LOAD_PARTIAL
// kh_trie_open_partial.  The first missing node in frontier order (a partial open: only the root)
// ends the open with KH_ENODE, its hash in missing32; a failed open leaves no handle.  own_ctx: the
// handle moves to a private context (the *_host entry points; kh_trie_open_partial without one).
static kh_trie* open_store(kh_ctx* c, const uint8_t* root32, const uint8_t* d_enc, const uint64_t* d_off, uint64_t n,
                           uint32_t flags, uint8_t* missing32, LoadMode mode, bool own_ctx) {
  if (n && (!d_enc || !d_off)) throw KhError{KH_EINVAL, "null buffer"};
  std::lock_guard<std::recursive_mutex> g(c->mu);
  HIPCHK(hipSetDevice(c->dev));
  kh_trie* h = trie_new(c, flags, false);
  try {
    const uint32_t id = 0;
    uint32_t midx = 0;
    uint8_t m32[32];
    uint64_t nm = 0;
    try {
      forest_load(h, &id, root32, 1, d_enc, d_off, n, &midx, m32, 1, &nm, nullptr, mode);
    } catch (...) {
      if (nm && missing32) memcpy(missing32, m32, 32);
      throw;
    }
    memcpy(h->root, root32, 32);
    if (own_ctx) make_private(h);
  } catch (...) {
    delete h;
    throw;
  }
  return h;
}
// the same from a host store, staged into the shared context
static int open_store_host(const uint8_t* root32, const uint8_t* enc, const uint64_t* off, uint64_t n, uint32_t flags,
                           uint8_t* missing32, kh_trie** out, LoadMode mode) {
  if (!out || !root32 || (n && (!enc || !off))) return set_err(KH_EINVAL, "null input");
  API_TRY({
    kh_ctx* c = shared_ctx(current_device());
    std::lock_guard<std::recursive_mutex> g(c->mu);
    HIPCHK(hipSetDevice(c->dev));
    const int rc = stage_store(c, enc, off, n);
    if (rc != KH_OK) return rc;
    *out = open_store(c, root32, (const uint8_t*)c->in_vals.p, (const uint64_t*)c->in_voff.p, n, flags, missing32, mode,
                      true);
  })
}

// The body of kh_forest_load_nodes, kh_forest_load_partial and kh_trie_fill_nodes (a fill: no trie
// list, no missing list, and any handle) and of their _host forms, whose store is staged first
// (stage_store makes its own checks of it).
static int load_entry(kh_trie* h, const uint32_t* tries, const uint8_t* roots32, uint64_t k, const uint8_t* enc,
                      const uint64_t* off, uint64_t n, uint32_t* miss_idx, uint8_t* miss32, uint64_t miss_cap,
                      uint64_t* n_missing, kh_stats* stats, LoadMode mode, uint64_t* n_decoded, bool host) {
  if (n_missing) *n_missing = 0;
  if (n_decoded) *n_decoded = 0;
  if (mode == LOAD_FILL) {
    if (!h) return set_err(KH_EINVAL, "null handle");
  } else if (!h || !h->forest) {
    return set_err(KH_EINVAL, "null handle or not a forest");
  }
  if ((k && (!tries || !roots32)) || (!host && n && (!enc || !off)) || (miss_cap && (!miss_idx || !miss32)))
    return set_err(KH_EINVAL, "null buffer");
  API_TRY({
    HANDLE_LOCK(h);
    kh_ctx* c = h->c;
    HIPCHK(hipSetDevice(c->dev));
    if (host) {
      const int rc = stage_store(c, enc, off, n);
      if (rc != KH_OK) return rc;
      enc = (const uint8_t*)c->in_vals.p;
      off = (const uint64_t*)c->in_voff.p;
    }
    forest_load(h, tries, roots32, k, enc, off, n, miss_idx, miss32, miss_cap, n_missing, stats, mode, n_decoded);
  })
}

extern "C" {

int kh_trie_open_nodes(kh_ctx* c, const uint8_t root32[32], const uint8_t* d_enc, const uint64_t* d_off, uint64_t n,
                       uint32_t flags, uint8_t missing32[32], kh_trie** out) {
  if (!c || !out || !root32) return set_err(KH_EINVAL, "null context, root or handle");
  API_TRY({ *out = open_store(c, root32, d_enc, d_off, n, flags, missing32, LOAD_FULL, false); })
}

int kh_trie_open_nodes_host(const uint8_t root32[32], const uint8_t* enc, const uint64_t* off, uint64_t n,
                            uint32_t flags, uint8_t missing32[32], kh_trie** out) {
  return open_store_host(root32, enc, off, n, flags, missing32, out, LOAD_FULL);
}

int kh_forest_load_nodes(kh_trie* f, const uint32_t* tries, const uint8_t* roots32, uint64_t k, const uint8_t* d_enc,
                         const uint64_t* d_off, uint64_t n, uint32_t* miss_idx, uint8_t* miss32, uint64_t miss_cap,
                         uint64_t* n_missing, kh_stats* stats) {
  return load_entry(f, tries, roots32, k, d_enc, d_off, n, miss_idx, miss32, miss_cap, n_missing, stats, LOAD_FULL,
                    nullptr, false);
}

int kh_forest_load_nodes_host(kh_trie* f, const uint32_t* tries, const uint8_t* roots32, uint64_t k,
                              const uint8_t* enc, const uint64_t* off, uint64_t n, uint32_t* miss_idx, uint8_t* miss32,
                              uint64_t miss_cap, uint64_t* n_missing, kh_stats* stats) {
  return load_entry(f, tries, roots32, k, enc, off, n, miss_idx, miss32, miss_cap, n_missing, stats, LOAD_FULL,
                    nullptr, true);
}

int kh_forest_roots(kh_trie* f, uint32_t* h_tries, uint8_t* h_roots32, uint64_t cap, uint64_t* n_tries) {
  if (!f || !f->forest || !n_tries) return set_err(KH_EINVAL, "null handle or output, or not a forest");
  API_TRY({
    HANDLE_LOCK(f);
    HIPCHK(hipSetDevice(f->c->dev));
    return forest_roots(f, h_tries, h_roots32, cap, n_tries);
  })
}

int kh_forest_evict(kh_trie* f, const uint32_t* tries, uint64_t k, uint64_t* n_evicted) {
  uint64_t dropped = 0;
  if (n_evicted) *n_evicted = 0;
  if (!f || !f->forest) return set_err(KH_EINVAL, "null handle or not a forest");
  if (k && !tries) return set_err(KH_EINVAL, "null buffer");
  API_TRY({
    HANDLE_LOCK(f);
    HIPCHK(hipSetDevice(f->c->dev));
    forest_evict(f, tries, k, &dropped);
    if (n_evicted) *n_evicted = dropped;
  })
}

int kh_trie_evict_subtrees(kh_trie* h, const uint32_t* tries, const uint8_t* paths32, const uint8_t* depths,
                           uint64_t n, uint8_t* status, uint8_t* hashes32, uint64_t* n_evicted, uint64_t* n_keys,
                           uint64_t* n_records) {
  if (n_evicted) *n_evicted = 0;
  if (n_keys) *n_keys = 0;
  if (n_records) *n_records = 0;
  if (!h) return set_err(KH_EINVAL, "null handle");
  if (n && (!paths32 || !depths || !status || !hashes32 || (h->forest && !tries)))
    return set_err(KH_EINVAL, "null buffer");
  API_TRY({
    HANDLE_LOCK(h);
    HIPCHK(hipSetDevice(h->c->dev));
    uint64_t out[3];
    evict_subtrees(h, tries, paths32, depths, n, status, hashes32, out);
    if (n_evicted) *n_evicted = out[0];
    if (n_keys) *n_keys = out[1];
    if (n_records) *n_records = out[2];
  })
}

// ---- partial handles: open / load from a witness, fill, and what a refused commit needs
int kh_trie_open_partial(kh_ctx* c, const uint8_t root32[32], const uint8_t* d_enc, const uint64_t* d_off, uint64_t n,
                         uint32_t flags, uint8_t missing32[32], kh_trie** out) {
  if (!out || !root32) return set_err(KH_EINVAL, "null root or handle");
  API_TRY({
    // (no context, as kh_forest_open: the one the *_host entry points use, and a private handle)
    const bool host = !c;
    if (host) c = shared_ctx(current_device());
    *out = open_store(c, root32, d_enc, d_off, n, flags, missing32, LOAD_PARTIAL, host);
  })
}

int kh_trie_open_partial_host(const uint8_t root32[32], const uint8_t* enc, const uint64_t* off, uint64_t n,
                              uint32_t flags, uint8_t missing32[32], kh_trie** out) {
  return open_store_host(root32, enc, off, n, flags, missing32, out, LOAD_PARTIAL);
}

int kh_forest_load_partial(kh_trie* f, const uint32_t* tries, const uint8_t* roots32, uint64_t k, const uint8_t* d_enc,
                           const uint64_t* d_off, uint64_t n, uint32_t* miss_idx, uint8_t* miss32, uint64_t miss_cap,
                           uint64_t* n_missing, kh_stats* stats) {
  return load_entry(f, tries, roots32, k, d_enc, d_off, n, miss_idx, miss32, miss_cap, n_missing, stats, LOAD_PARTIAL,
                    nullptr, false);
}

int kh_forest_load_partial_host(kh_trie* f, const uint32_t* tries, const uint8_t* roots32, uint64_t k,
                                const uint8_t* enc, const uint64_t* off, uint64_t n, uint32_t* miss_idx,
                                uint8_t* miss32, uint64_t miss_cap, uint64_t* n_missing, kh_stats* stats) {
  return load_entry(f, tries, roots32, k, enc, off, n, miss_idx, miss32, miss_cap, n_missing, stats, LOAD_PARTIAL,
                    nullptr, true);
}

int kh_trie_fill_nodes(kh_trie* h, const uint8_t* d_enc, const uint64_t* d_off, uint64_t n, uint64_t* n_decoded,
                       kh_stats* stats) {
  return load_entry(h, nullptr, nullptr, 0, d_enc, d_off, n, nullptr, nullptr, 0, nullptr, stats, LOAD_FILL, n_decoded,
                    false);
}

int kh_trie_fill_nodes_host(kh_trie* h, const uint8_t* enc, const uint64_t* off, uint64_t n, uint64_t* n_decoded,
                            kh_stats* stats) {
  return load_entry(h, nullptr, nullptr, 0, enc, off, n, nullptr, nullptr, 0, nullptr, stats, LOAD_FILL, n_decoded,
                    true);
}

int kh_trie_need_host(kh_trie* h, const uint32_t* trie, const uint8_t* keys, uint32_t klen, uint64_t n,
                      uint8_t* need_flag, uint8_t* need32) {
  if (!h) return set_err(KH_EINVAL, "null handle");
  if (n && (!keys || !need_flag || !need32)) return set_err(KH_EINVAL, "null buffer");
  API_TRY({
    HANDLE_LOCK(h);
    kh_ctx* c = h->c;
    HIPCHK(hipSetDevice(c->dev));
    hipStream_t st = c->st;
    query_check(h, trie, klen, n, h->flags & KH_HASH_KEYS);
    if (n == 0) return KH_OK;
    trie_settle(h);
    if (!(h->nstubs && h->rn && h->mcap)) {  // no stub to reach
      memset(need_flag, 0, n);
      memset(need32, 0, n * 32);
      return KH_OK;
    }
    Layout L;
    uint8_t *dk, *df;
    uint32_t* dt;
    uint64_t *K, *dh;
    L.add(K, n * 4 + 8);
    L.add(dh, n * 4);
    L.add(df, n + 64);
    place(h->gbuf, L);
    stage_query_keys(c, trie, keys, klen, n, dk, dt);
    if (h->flags & KH_HASH_KEYS) {
      hash_keys_to(st, (const uint8_t*)dk, klen, n, K);
    } else {
      HIPCHK(hipMemcpyAsync(K, dk, n * 32, hipMemcpyDeviceToDevice, st));
    }
    hipLaunchKernelGGL(k_need, GRID(n, BS), dim3(BS), 0, st, map_of(h), recs_of(h), (const uint64_t*)K,
                       (const uint32_t*)dt, n, df, dh);
    LAUNCH_CHECK();
    HIPCHK(hipMemcpyAsync(need_flag, df, n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(need32, dh, n * 32, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  })
}

}  // extern "C"
