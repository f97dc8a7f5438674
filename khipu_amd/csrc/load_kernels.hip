// The forest load, kh_forest_roots, kh_forest_evict, the partial handles' open, fill and need, and
// the range fills (kh_trie_fill_ranges: fillrange.h; a service of the partial handles, and this unit is theirs):
// their kernels (load.h holds the bodies), then the host drivers and the C entry points (host.h).
// A compilation unit of its own: a code object of its own cannot shift the placement of the hot
// kernels of khst.hip (tests/test_code_layout.py).  The kernels take the POD views and raw
// pointers, one thread per frontier node or record.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "load.h"
#include "rangeverify.h"
#include "keccak.h"
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

// ---- kh_trie_fill_ranges (fillrange.h): range responses into a partial handle.  Cold like the rest
// of this unit: one thread per range, entry, record, op or element.
__global__ void k_rv_order(RvIn I, uint64_t ne, uint32_t* bad);  // rangeverify_kernels.hip's order check

// the call as the kernels see it: arrays by range s (input order), or by sorted position j = pos[s]
// (the listed tries in ascending id order, as FillMode wants them)
struct FillPlan {
  const uint32_t* tries;    // [nr] nullable: trie 0
  const uint64_t* roots;    // [nr*4] nullable: no claim
  const uint64_t* origins;  // [nr*4] nullable: all zero
  const uint64_t* keys;     // [ne*4]
  const uint64_t* ent_off;  // [nr+1]
  uint64_t nr;
  const uint32_t* pos;      // [nr]
  uint64_t *lo, *hi;        // [nr*4] by j: the span
  uint32_t* resident;       // [nr] by s
  uint64_t* oldroot;        // [nr*4] by s: a resident trie's root
  uint32_t *live, *inside, *dropped, *miss;  // [nr] by j
  uint8_t* status;          // [nr] by s
};
KH_HD bool words_eq4(const uint64_t* a, const uint64_t* b) {
  return a[0] == b[0] && a[1] == b[1] && a[2] == b[2] && a[3] == b[3];
}
// Per range: residency (a live record at anchor (t, 0)) and the root that record stands for, the
// span, and what is decided before the commit: the order, the root claim, an empty trie's root.
__global__ void __launch_bounds__(BS) k_fill_plan(FillPlan P, AMap M, Recs R, bool has_map, const uint32_t* bad) {
  const uint64_t s = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (s >= P.nr) return;
  const uint32_t t = P.tries ? P.tries[s] : 0u, j = P.pos[s];
  const uint64_t e0 = P.ent_off[s], e1 = P.ent_off[s + 1];
  const uint64_t zero[4] = {0, 0, 0, 0};
  const uint32_t r = has_map ? map_find(M, R, t, 0, zero) : NONE;
  uint64_t root[4] = {0, 0, 0, 0};
  if (r != NONE) {
    const uint32_t rl = R.rrl[r];
    if (rl >= 32) {
      for (int q = 0; q < 4; ++q) root[q] = R.rref[4ull * r + q];
    } else {  // a root node shorter than a hash is referenced by its encoding; the root is its hash
      kec256_msg<false>((const uint8_t*)&R.rref[4ull * r], rl, root);
    }
  }
  for (int q = 0; q < 4; ++q) {
    P.lo[4 * j + q] = P.origins ? P.origins[4 * s + q] : 0;
    P.hi[4 * j + q] = e1 > e0 ? P.keys[4 * (e1 - 1) + q] : ~0ULL;
    P.oldroot[4 * s + q] = root[q];
  }
  P.resident[s] = r != NONE ? 1u : 0u;
  uint8_t st = RANGE_OK;
  if (bad[s]) {
    st = RANGE_BAD_ORDER;
  } else if (r == NONE) {
    if (e1 == e0 && P.roots && !bytes_eq32((const uint8_t*)(P.roots + 4 * s), empty_root_hash())) st = RANGE_BAD_ROOT;
  } else if (P.roots && !words_eq4(P.roots + 4 * s, root)) {
    st = RANGE_BAD_ROOT;
  }
  P.status[s] = st;
}
// a forest's op trie ids: entry i names its range's trie
__global__ void __launch_bounds__(BS) k_fill_optrie(const uint32_t* tries, const uint64_t* ent_off, uint64_t nr,
                                                    uint64_t ne, uint32_t* out) {
  const uint64_t i = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (i >= ne) return;
  out[i] = tries[rv_range_of(ent_off, nr, i)];
}
// The streaming pass: one thread a record, reading its first 64-byte line (key prefix, trie, db,
// rmask, live).  Stubs are few among the records and a wave's stubs mostly of one trie: the lanes
// of one trie are counted by ballot and their first lane adds once per counter.
__global__ void __launch_bounds__(BS) k_fill_stubs(Recs R, uint64_t n, FillMode F, uint32_t* live, uint32_t* inside) {
  const uint64_t r = (uint64_t)blockIdx.x * BS + threadIdx.x;
  uint32_t j = NONE;
  bool in = false;
  if (r < n && load_is_stub(R, r)) {
    const uint32_t t = R.rt[r];
    j = seg_of(F.tries, F.nt, t);
    if (j >= F.nt || F.tries[j] != t) {
      j = NONE;
    } else {
      in = fill_inside(R.key(r), R.rmask[r] & 0xFF, F.lo + 4 * j, F.hi + 4 * j);
    }
  }
  for (uint64_t pend = __ballot(j != NONE); pend;) {  // (wave-uniform: every lane stays for the ballots)
    const int leader = __ffsll((long long)pend) - 1;
    const uint32_t lj = (uint32_t)__shfl((int)j, leader);
    const uint64_t grp = __ballot(j == lj), gin = __ballot(j == lj && in);
    if ((int)__lane_id() == leader) {
      atomicAdd(&live[lj], (uint32_t)__popcll(grp));
      if (gin) atomicAdd(&inside[lj], (uint32_t)__popcll(gin));
    }
    pend &= ~grp;
  }
}
// a range without entries is complete only if no stub of its trie lies at or after its origin
__global__ void __launch_bounds__(BS) k_fill_pre(FillPlan P) {
  const uint64_t s = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (s >= P.nr || P.status[s] != RANGE_OK) return;
  if (P.ent_off[s + 1] == P.ent_off[s] && P.resident[s] && P.inside[P.pos[s]]) P.status[s] = RANGE_INCOMPLETE;
}
// After the commit: a range with entries keeps RANGE_OK only if its trie's new root is the old one
// (the given one for a trie loaded whole) and the descent dropped every inside stub of the pass.
__global__ void __launch_bounds__(BS) k_fill_judge(FillPlan P, const uint32_t* ctries, const uint64_t* croots,
                                                   uint32_t nct) {
  const uint64_t s = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (s >= P.nr || P.status[s] != RANGE_OK || P.ent_off[s + 1] == P.ent_off[s]) return;
  const uint32_t t = P.tries ? P.tries[s] : 0u, j = P.pos[s];
  const uint32_t g = seg_of(ctries, nct, t);
  const uint64_t* want = P.resident[s] ? P.oldroot + 4 * s : P.roots + 4 * s;
  const bool ok = g < nct && ctries[g] == t && words_eq4(croots + 4 * g, want) && P.inside[j] == P.dropped[j];
  if (!ok) P.status[s] = RANGE_BAD_ROOT;
}

// The descent of a commit in fill mode: khst.hip's k_f_descend, but a stub the walk reaches is
// tested against its trie's span.  Inside: marked touched (the gather brings nothing for it, the
// delete takes it out of the map) and counted once, by the lane whose exchange marked it.  Not
// inside: a missing node as in a commit (ctr[3] bit 1), its trie flagged.  A leaf under a depth-63
// branch is replaced like any leaf: a response re-delivers keys, it makes no value-only branch.
__global__ void __launch_bounds__(BS) k_fill_descend(FOps O, AMap M, Recs R, FillMode F, uint32_t* touched,
                                                     uint8_t* replaced, uint32_t* tlist, unsigned long long* ctr,
                                                     uint8_t* vbf) {
  const uint64_t o = (uint64_t)blockIdx.x * BS + threadIdx.x;
  auto mark = [&](bool want, uint32_t r) {  // (k_f_descend's: the first lane of a run of one record exchanges)
    const uint32_t rr = want ? r : NONE;
    const uint32_t prev = __shfl_up(rr, 1);
    const bool lead = want && ((threadIdx.x & 63) == 0 || prev != rr);
    bool first = false;
    if (lead && __hip_atomic_load(&touched[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u)
      first = atomicExch(&touched[r], 1u) == 0u;
    const uint64_t slot = wave_claim(&ctr[0], first);
    if (first) tlist[slot] = r;
    return first;
  };
  const bool live = o < O.n;
  const uint64_t* K = O.key + 4 * (live ? o : 0);
  const uint32_t t = live ? O.trie[o] : 0;
  uint32_t d = 0;
  bool active = live, repl = false, lost = live, vb = false;
  for (int step = 0; step < 70 && __ballot(active); ++step) {
    uint32_t r = NONE, drop_j = NONE;
    if (active) {
      r = map_find(M, R, t, d, K);
      if (r == NONE) {
        active = lost = false;
      } else {
        const uint32_t db = R.rdb[r];
        if (db == EL_LEAF) {
          if (words_eq4(R.key(r), K)) {
            replaced[r] = 1;  // keys are unique in the batch: one op per leaf
            repl = true;
          }
          active = lost = false;
        } else if (db == VB_DEPTH) {  // a value-only branch: only its own key reaches it, and stays one
          if (words_eq4(R.key(r), K))
            vb = repl = true;
          else
            r = NONE;
          active = lost = false;
        } else if (const int lcp = lcp_nibbles(load_key(K, 0), load_key(R.key(r), 0)); lcp < (int)db) {
          // leaves the extension (the subtree is gathered whole), or a stub
          const uint32_t md = R.rmask[r] & 0xFF;
          if (db == EL_STUB && !(md > d && lcp < (int)md)) {
            const uint32_t j = seg_of(F.tries, F.nt, t);  // (every op's trie is listed)
            if (j < F.nt && fill_inside(R.key(r), md, F.lo + 4 * j, F.hi + 4 * j)) {
              drop_j = j;
            } else {
              atomicOr(&ctr[3], 2ULL);
              if (j < F.nt) F.miss[j] = 1;  // (every writer stores the same 1)
            }
          } else {
            r = NONE;
          }
          active = lost = false;
        } else {
          d = db + 1;
        }
      }
    }
    const bool first = mark(r != NONE, r);
    if (first && drop_j != NONE) atomicAdd(&F.dropped[drop_j], 1u);
  }
  wave_atomic_add(&ctr[1], repl ? 1ULL : 0ULL);
  wave_atomic_add(&ctr[6], vb ? 1ULL : 0ULL);
  if (live) vbf[o] = vb ? 1 : 0;
  if (lost) ctr[2] = 3;
}
// the refused fill's missing list: k_stub_missing without the inside stubs (dropped, not missing)
__global__ void __launch_bounds__(BS) k_fill_missing(Recs R, FillMode F, const uint32_t* list, uint64_t n, uint64_t cap,
                                                     uint32_t* out_trie, uint64_t* out_hash,
                                                     unsigned long long* cnt) {
  const uint64_t i = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (i >= n) return;
  const uint32_t r = list[i];
  if (!load_is_stub(R, r)) return;
  const uint32_t j = seg_of(F.tries, F.nt, R.rt[r]);
  if (j < F.nt && fill_inside(R.key(r), R.rmask[r] & 0xFF, F.lo + 4 * j, F.hi + 4 * j)) return;
  const unsigned long long t = atomicAdd(cnt, 1ULL);
  if (t >= cap) return;
  out_trie[t] = R.rt[r];
  for (int q = 0; q < 4; ++q) out_hash[4 * t + q] = R.rbref[4ull * r + q];
}
// The write-back selection of a fill (after k_f_elem_flags, before the old anchors leave the map):
// the set is the nodes the handle did not hold.  A commit selects every upsert's leaf; one that
// replaces the resident leaf of its key (a re-delivered boundary key) was held.  It selects the
// extension of a branch built where a stub stood; a STUB_BRANCH stub's own extension was held.
__global__ void __launch_bounds__(BS) k_fill_sel(Topo T, Elems E, const uint32_t* tries, AMap M, Recs R, uint64_t B,
                                                 uint8_t* sel) {
  const uint64_t g = (uint64_t)blockIdx.x * BS + threadIdx.x;
  if (g < T.m) {
    if (E.src[T.sidx[g]] != NONE) return;
    const uint32_t t = tries[T.sseg ? T.sseg[g] : 0], a = (uint32_t)(T.lf_pd[g] + 1);
    const uint32_t old = map_find(M, R, t, a, T.skey + 4 * g);
    if (old != NONE && R.rdb[old] == EL_LEAF && words_eq4(R.key(old), T.skey + 4 * g)) sel[g] = 0;
    return;
  }
  const uint64_t j = g - T.m;
  if (j >= B || !T.br_ext[j]) return;
  const uint64_t f = T.br_first[j];
  const uint32_t t = tries[T.sseg ? T.sseg[f] : 0], db = T.br_depth[j], d = db - T.br_ext[j];
  const uint32_t old = map_find(M, R, t, d, T.skey + 4 * f);
  if (old == NONE || R.rdb[old] != EL_STUB || (R.rmask[old] & 0xFFu) != db) return;
  const uint32_t xrl = T.ex_rlen[j] >= 32 ? 32 : T.ex_rlen[j];
  if (R.rrl[old] == xrl && words_eq4(&R.rref[4ull * old], T.ex_ref + 4 * j)) sel[T.m + 2 * j + 1] = 0;
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

// ---------------------------------------------------------------------------
// host: range fills (fillrange.h)
// ---------------------------------------------------------------------------
// nr ranges of ne entries in all into handle h, every input in HBM on its stream; ht: the trie ids
// on the host (a single trie: empty).  The ranges are judged in stages -- order, root claims and
// completeness before the commit; missing nodes at its descent; roots and dropped stubs after it --
// and a call refused at one stage reports the ranges later stages would judge as they stand.
// Host syncs: one before the commit (statuses, residency), the commit's own, one after it.
// what refuses the call whatever the ranges hold (checked before anything is staged)
static void fill_precheck(const kh_trie* h, std::vector<uint32_t> ht, uint64_t nr) {
  if (!h->sps.empty()) throw KhError{KH_EINVAL, "kh_trie_fill_ranges: a savepoint is open"};
  if (!h->forest && nr > 1)
    throw KhError{KH_EINVAL, "kh_trie_fill_ranges: a trie id listed twice (a single trie takes one range a call)"};
  std::sort(ht.begin(), ht.end());
  if (std::adjacent_find(ht.begin(), ht.end()) != ht.end())
    throw KhError{KH_EINVAL, "kh_trie_fill_ranges: a trie id listed twice"};
}
static void fill_ranges_dev(kh_trie* h, const uint32_t* d_tries, const std::vector<uint32_t>& ht, const uint8_t* d_roots,
                            const uint8_t* d_orig, uint64_t nr, const uint8_t* d_keys, const uint8_t* d_vals,
                            const uint64_t* d_voff, const uint64_t* d_eo, uint64_t ne, uint8_t* status,
                            uint64_t* stubs_left, uint64_t* n_keys, uint64_t* n_stubs) {
  fill_precheck(h, ht, nr);
  trie_settle(h);
  kh_ctx* c = h->c;
  hipStream_t st = c->st;
  const bool forest = h->forest;
  // the listed tries in ascending order: sorted position j of range s, no id twice
  std::vector<uint32_t> order(nr), pos(nr), strie(nr, 0);
  for (uint64_t s = 0; s < nr; ++s) order[s] = (uint32_t)s;
  if (forest) {
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return ht[a] < ht[b]; });
    for (uint64_t j = 0; j < nr; ++j) strie[j] = ht[order[j]];
  }
  for (uint64_t j = 0; j < nr; ++j) pos[order[j]] = (uint32_t)j;
  Layout L;
  uint32_t *dstrie, *dpos, *bad, *resident, *live, *inside, *dropped, *miss, *optrie;
  uint64_t *lo, *hi, *oldroot;
  uint8_t* dst;
  L.add_all(nr, dstrie, dpos);
  L.add_all(nr, bad, resident, live, inside, dropped, miss);  // (back to back: one memset)
  L.add_all(nr * 4, lo, hi, oldroot);
  L.add(optrie, ne + 1, forest);
  L.add(dst, nr);
  place(h->gbuf, L);
  HIPCHK(hipMemcpyAsync(dstrie, strie.data(), nr * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(dpos, pos.data(), nr * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(bad, 0, (size_t)((char*)(miss + nr) - (char*)bad), st));
  const RvIn I{(const uint64_t*)d_roots, (const uint64_t*)d_orig, nullptr, nr, (const uint64_t*)d_keys, d_voff, d_eo,
               NStore{}};
  const FillPlan P{forest ? d_tries : nullptr, (const uint64_t*)d_roots, (const uint64_t*)d_orig,
                   (const uint64_t*)d_keys, d_eo, nr, dpos, lo, hi, resident, oldroot, live, inside, dropped, miss, dst};
  const FillMode FM{dstrie, lo, hi, (uint32_t)nr, dropped, miss};
  const bool has_map = h->rn && h->mcap;
  if (ne) {
    hipLaunchKernelGGL(k_rv_order, GRID(ne, BS), dim3(BS), 0, st, I, ne, bad);
    LAUNCH_CHECK();
    if (forest) {
      hipLaunchKernelGGL(k_fill_optrie, GRID(ne, BS), dim3(BS), 0, st, d_tries, d_eo, nr, ne, optrie);
      LAUNCH_CHECK();
    }
  }
  hipLaunchKernelGGL(k_fill_plan, GRID(nr, BS), dim3(BS), 0, st, P, has_map ? map_of(h) : AMap{}, recs_of(h), has_map,
                     (const uint32_t*)bad);
  LAUNCH_CHECK();
  if (has_map && h->nstubs) {
    hipLaunchKernelGGL(k_fill_stubs, GRID(h->rn, BS), dim3(BS), 0, st, recs_of(h), h->rn, FM, live, inside);
    LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_fill_pre, GRID(nr, BS), dim3(BS), 0, st, P);
  LAUNCH_CHECK();
  // (the outputs are staged: an error writes nothing)
  std::vector<uint8_t> hst(nr), hroots(nr * 32), hclaim(d_roots ? nr * 32 : 0);
  std::vector<uint32_t> hres(nr), hlive(nr), hdrop(nr, 0), hmiss(nr);
  HIPCHK(hipMemcpyAsync(hst.data(), dst, nr, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(hres.data(), resident, nr * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(hlive.data(), live, nr * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(hroots.data(), oldroot, nr * 32, hipMemcpyDeviceToHost, st));
  if (d_roots) HIPCHK(hipMemcpyAsync(hclaim.data(), d_roots, nr * 32, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  for (uint64_t s = 0; s < nr; ++s) {
    if (hres[s]) continue;
    if (!forest) throw KhError{KH_EINVAL, "kh_trie_fill_ranges: the trie is not resident (open it partial first)"};
    if (!d_roots) throw KhError{KH_EINVAL, "kh_trie_fill_ranges: a trie that is not resident needs its root"};
  }
  auto all_ok = [&] { return std::all_of(hst.begin(), hst.end(), [](uint8_t x) { return x == RANGE_OK; }); };
  auto finish = [&](uint64_t keys, uint64_t stubs) {
    memcpy(status, hst.data(), nr);
    for (uint64_t s = 0; s < nr && stubs_left; ++s) stubs_left[s] = hlive[pos[s]] - hdrop[pos[s]];
    if (n_keys) *n_keys = keys;
    if (n_stubs) *n_stubs = stubs;
  };
  if (!all_ok()) return finish(0, 0);
  const uint64_t leaves0 = h->nleaves;
  if (ne) {
    const FillResult fr =
        commit_fill(h, forest ? optrie : nullptr, d_keys, d_vals, d_voff, ne, FM, [&] {
          hipLaunchKernelGGL(k_fill_judge, GRID(nr, BS), dim3(BS), 0, st, P, (const uint32_t*)h->d_tries,
                             (const uint64_t*)h->d_roots, (uint32_t)h->tries.size());
          LAUNCH_CHECK();
          HIPCHK(hipMemcpyAsync(hst.data(), dst, nr, hipMemcpyDeviceToHost, st));
          HIPCHK(hipMemcpyAsync(hdrop.data(), dropped, nr * 4, hipMemcpyDeviceToHost, st));
          HIPCHK(hipStreamSynchronize(st));
          return all_ok();
        });
    if (fr == FILL_MISSING) {  // kh_trie_missing lists the hashes, as after a refused commit
      HIPCHK(hipMemcpyAsync(hmiss.data(), miss, nr * 4, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      for (uint64_t s = 0; s < nr; ++s)
        if (hmiss[pos[s]]) hst[s] = RANGE_MISSING;
    } else if (fr == FILL_MOVED) {  // a stub of unknown kind re-anchored: the entries do not rebuild that trie
      for (uint64_t s = 0; s < nr; ++s)
        if (std::find(h->miss_tries.begin(), h->miss_tries.end(), forest ? ht[s] : 0u) != h->miss_tries.end())
          hst[s] = RANGE_BAD_ROOT;
      h->miss_tries.clear();
      h->miss_hashes.clear();
    }
    if (fr != FILL_KEPT) {
      std::fill(hdrop.begin(), hdrop.end(), 0u);
      if (all_ok()) throw KhError{KH_EINTERNAL, "kh_trie_fill_ranges: a refused fill names no range"};
      return finish(0, 0);
    }
  } else {  // nothing to ingest; cursors end and the write-back set is the (empty) call's
    ++h->epoch;
    h->em_n = h->em_bytes = 0;
    h->em_valid = (h->flags & KH_EMIT_NODES) != 0;
  }
  uint64_t ndrop = 0;
  for (uint64_t j = 0; j < nr; ++j) ndrop += hdrop[j];
  h->nstubs -= ndrop;
  // the last roots: the call's tries, ascending, each with the root it kept
  h->tries.assign(strie.begin(), strie.end());
  h->roots.resize(nr * 32);
  for (uint64_t j = 0; j < nr; ++j) {
    const uint64_t s = order[j];
    memcpy(h->roots.data() + 32 * j, (hres[s] ? hroots.data() : hclaim.data()) + 32 * s, 32);
  }
  h->d_tries = nullptr;
  h->d_roots = nullptr;
  finish(h->nleaves - leaves0, ndrop);
}

extern "C" {

int kh_dev_trie_fill_ranges(kh_trie* h, const uint32_t* d_tries, const uint8_t* d_roots32, const uint8_t* d_origins32,
                            uint64_t nr, const uint8_t* d_keys32, const uint8_t* d_vals, const uint64_t* d_voff,
                            const uint64_t* d_ent_off, uint8_t* status, uint64_t* stubs_left, uint64_t* n_keys,
                            uint64_t* n_stubs) {
  if (n_keys) *n_keys = 0;
  if (n_stubs) *n_stubs = 0;
  if (!h) return set_err(KH_EINVAL, "null handle");
  if (nr >= (1ULL << 31)) return set_err(KH_EINVAL, "kh_trie_fill_ranges: batch too large");
  if (!d_ent_off || !d_voff || (nr && (!status || (h->forest && !d_tries))))
    return set_err(KH_EINVAL, "kh_trie_fill_ranges: null array");
  // (roots, origins and keys are read as 64-bit words, the offsets are 64-bit words)
  if ((((uintptr_t)d_roots32 | (uintptr_t)d_origins32 | (uintptr_t)d_keys32 | (uintptr_t)d_voff | (uintptr_t)d_ent_off) &
       7) != 0 || ((uintptr_t)d_tries & 3) != 0)
    return set_err(KH_EINVAL, "kh_dev_trie_fill_ranges: roots, origins, keys and offsets must be 8-byte aligned");
  API_TRY({
    HANDLE_LOCK(h);
    kh_ctx* c = h->c;
    HIPCHK(hipSetDevice(c->dev));
    if (nr == 0) return KH_OK;
    uint64_t eo[2];
    std::vector<uint32_t> ht(h->forest ? nr : 0);
    HIPCHK(hipMemcpyAsync(&eo[0], d_ent_off, 8, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipMemcpyAsync(&eo[1], d_ent_off + nr, 8, hipMemcpyDeviceToHost, c->st));
    if (h->forest) HIPCHK(hipMemcpyAsync(ht.data(), d_tries, nr * 4, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    if (eo[0] != 0) return set_err(KH_EINVAL, "kh_dev_trie_fill_ranges: ent_off[0] must be 0");
    const uint64_t ne = eo[1];
    if (ne >= (1ULL << 31)) return set_err(KH_EINVAL, "kh_trie_fill_ranges: batch too large");
    if (ne && !d_keys32) return set_err(KH_EINVAL, "kh_trie_fill_ranges: null array");
    fill_ranges_dev(h, d_tries, ht, d_roots32, d_origins32, nr, d_keys32, d_vals, d_voff, d_ent_off, ne, status,
                    stubs_left, n_keys, n_stubs);
  })
}

int kh_trie_fill_ranges_host(kh_trie* h, const uint32_t* tries, const uint8_t* roots32, const uint8_t* origins32,
                             uint64_t nr, const uint8_t* keys32, const uint8_t* vals, const uint64_t* voff,
                             const uint64_t* ent_off, uint8_t* status, uint64_t* stubs_left, uint64_t* n_keys,
                             uint64_t* n_stubs) {
  if (n_keys) *n_keys = 0;
  if (n_stubs) *n_stubs = 0;
  if (!h) return set_err(KH_EINVAL, "null handle");
  if (nr >= (1ULL << 31)) return set_err(KH_EINVAL, "kh_trie_fill_ranges: batch too large");
  if (!ent_off || !voff || (nr && (!status || (h->forest && !tries))))
    return set_err(KH_EINVAL, "kh_trie_fill_ranges: null array");
  API_TRY({
    for (uint64_t s = 0; s < nr; ++s)
      if (ent_off[s + 1] < ent_off[s]) throw KhError{KH_EINVAL, "kh_trie_fill_ranges: ent_off must not decrease"};
    const uint64_t e0 = ent_off[0], ne = ent_off[nr] - e0;
    if (ne >= (1ULL << 31)) throw KhError{KH_EINVAL, "kh_trie_fill_ranges: batch too large"};
    if (ne && !keys32) throw KhError{KH_EINVAL, "kh_trie_fill_ranges: null array"};
    for (uint64_t i = e0; i < e0 + ne; ++i) {
      if (voff[i + 1] < voff[i]) throw KhError{KH_EINVAL, "kh_trie_fill_ranges: voff must not decrease"};
      if (voff[i + 1] - voff[i] > 0xFFFFFFFFull)
        throw KhError{KH_EINVAL, "kh_trie_fill_ranges: a value longer than 2^32 - 1 bytes"};
    }
    const uint64_t v0 = voff[e0], vb = voff[e0 + ne] - v0;
    if (vb && !vals) throw KhError{KH_EINVAL, "kh_trie_fill_ranges: null array"};
    if (nr == 0) return KH_OK;
    HANDLE_LOCK(h);
    kh_ctx* c = h->c;
    HIPCHK(hipSetDevice(c->dev));
    hipStream_t st = c->st;
    // offsets rebased to zero; everything staged into one buffer
    std::vector<uint64_t> reo(nr + 1), rvo(ne + 1);
    for (uint64_t s = 0; s <= nr; ++s) reo[s] = ent_off[s] - e0;
    for (uint64_t i = 0; i <= ne; ++i) rvo[i] = voff[e0 + i] - v0;
    std::vector<uint32_t> ht;
    if (h->forest) ht.assign(tries, tries + nr);
    fill_precheck(h, ht, nr);
    Layout Li;
    uint8_t *droots, *dorig, *dkeys, *dvals;
    uint64_t *dvoff, *deo;
    uint32_t* dtries;
    Li.add(droots, nr * 32, roots32 != nullptr);
    Li.add(dorig, nr * 32, origins32 != nullptr);
    Li.add(dkeys, ne * 32 + 32);
    Li.add(dvals, vb + 64);
    Li.add(dvoff, ne + 1);
    Li.add(deo, nr + 1);
    Li.add(dtries, nr, h->forest);
    place(c->rv_in, Li);
    if (roots32) HIPCHK(hipMemcpyAsync(droots, roots32, nr * 32, hipMemcpyHostToDevice, st));
    if (origins32) HIPCHK(hipMemcpyAsync(dorig, origins32, nr * 32, hipMemcpyHostToDevice, st));
    if (ne) HIPCHK(hipMemcpyAsync(dkeys, keys32 + 32 * e0, ne * 32, hipMemcpyHostToDevice, st));
    if (vb) HIPCHK(hipMemcpyAsync(dvals, vals + v0, vb, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dvoff, rvo.data(), (ne + 1) * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(deo, reo.data(), (nr + 1) * 8, hipMemcpyHostToDevice, st));
    if (h->forest) HIPCHK(hipMemcpyAsync(dtries, tries, nr * 4, hipMemcpyHostToDevice, st));
    fill_ranges_dev(h, h->forest ? dtries : nullptr, ht, roots32 ? droots : nullptr, origins32 ? dorig : nullptr, nr,
                    dkeys, dvals, dvoff, deo, ne, status, stubs_left, n_keys, n_stubs);
  })
}

}  // extern "C"
