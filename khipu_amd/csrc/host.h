// What the host side of every unit of libkhst.so shares: the error type and launch macros, the
// device buffers and workspace layouts, the context and the resident handle, the build's argument
// structs, and the helpers of khst.hip that the service units call (export_, prove_, load_, range_
// and rangeverify_kernels.hip hold their services' drivers and C entry points).  Host code only:
// no kernel is defined or instantiated here, and prims.h (kernel templates) is khst.hip's alone --
// a service unit reaches the scans and the radix sort through the wrappers declared below
// (DESIGN.md "Source layout").
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <exception>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <string>
#include <vector>

#include "../../include/khst.h"
#include "trie_ops.h"
#include "forest.h"
#include "fillrange.h"
#include "layout.h"

struct HostStage;  // khst.hip: host inputs still streaming in (BuildArgs::hs)

namespace khst {

// ---------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------
// the calling thread's message for kh_last_error (khst.hip holds the string); returns code
int set_err(int code, const std::string& msg);

struct KhError {
  int code;
  std::string msg;
};
#define HIPCHK(x)                                                                                  \
  do {                                                                                             \
    hipError_t e_ = (x);                                                                           \
    if (e_ != hipSuccess) {                                                                        \
      (void)hipGetLastError(); /* clear it, or the next launch check reports it again */           \
      throw KhError{e_ == hipErrorOutOfMemory ? KH_ENOMEM : KH_EDEVICE,                            \
                    std::string(#x) + ": " + hipGetErrorString(e_)};                               \
    }                                                                                              \
  } while (0)
#define LAUNCH_CHECK() HIPCHK(hipGetLastError())

#define GRID(n, bs) dim3((unsigned)(((n) + (bs)-1) / (bs)))
constexpr int BS = 256;

// ---------------------------------------------------------------------------
// device workspace
// ---------------------------------------------------------------------------
// selects device d (d >= 0) for the guard's scope, restoring the caller's device after
struct DevScope {
  int prev = -1;
  explicit DevScope(int d) {
    int cur = -1;
    if (d >= 0 && hipGetDevice(&cur) == hipSuccess && cur != d && hipSetDevice(d) == hipSuccess) prev = cur;
  }
  ~DevScope() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
  DevScope(const DevScope&) = delete;
  DevScope& operator=(const DevScope&) = delete;
};

// A device buffer that remembers the GPU it lives on: growth drains and frees on THAT
// device, and allocates on `on` (or on the current device when on < 0).
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  int dev = -1;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }  // a throw between ensure() and release() does not leak HBM
  void ensure(size_t bytes, int on = -1) {
    if (on < 0) {
      if (hipGetDevice(&on) != hipSuccess) on = 0;
    }
    if (bytes <= cap && dev == on) return;
    if (p) {
      // work still reading the old buffer may be in flight (kh_dev_partition_ev returns before
      // its value copy ends): drain its device before the buffer goes (growth is rare)
      DevScope ds(dev);
      HIPCHK(hipDeviceSynchronize());
      HIPCHK(hipFree(p));
    }
    p = nullptr;
    cap = 0;
    size_t want = bytes + bytes / 8 + 4096;
    DevScope ds(on);
    HIPCHK(hipMalloc(&p, want));
    cap = want;
    dev = on;
  }
  void release() {
    if (p) {
      DevScope ds(dev);
      (void)hipFree(p);
    }
    p = nullptr;
    cap = 0;
    dev = -1;
  }
};

// the arrays carved out of one DevBuf, each declared once (layout.h)
[[noreturn]] inline void layout_fail(const char* msg) { throw KhError{KH_EINTERNAL, msg}; }
using Layout = BasicLayout<layout_fail>;
inline void place(DevBuf& b, const Layout& L) {
  b.ensure(L.bytes());
  L.place(b.p, b.cap);
}

struct BuildInfo {  // the last build's sizes, for build_stats
  uint64_t n = 0, m = 0, B = 0, key_perms = 0, arena = 0;
  uint32_t levels = 0;
  bool full_sort = false, early = false, stage_ev = true;
};
// A host thread kept for a context (kh_block_commit's storage phase): post() hands it one job,
// join() waits for the job; no thread is started per call.
struct Worker {
  std::thread th;
  std::mutex mu;
  std::condition_variable cv;
  std::function<void()> job;
  bool has_job = false, stop = false;
  void post(std::function<void()> f) {
    std::unique_lock<std::mutex> lk(mu);
    if (!th.joinable()) th = std::thread([this] { loop(); });
    job = std::move(f);
    has_job = true;
    cv.notify_all();
  }
  void join() {
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [this] { return !has_job; });
  }
  void loop() {
    std::unique_lock<std::mutex> lk(mu);
    for (;;) {
      cv.wait(lk, [this] { return has_job || stop; });
      if (stop) return;
      std::function<void()> f = std::move(job);
      lk.unlock();
      f();  // (the job catches its own exceptions)
      lk.lock();
      has_job = false;
      cv.notify_all();
    }
  }
  ~Worker() {
    {
      std::lock_guard<std::mutex> lk(mu);
      stop = true;
    }
    cv.notify_all();
    if (th.joinable()) th.join();
  }
};
constexpr int RING_SLOTS = 4;
constexpr size_t RING_CHUNK = 64u << 20;  // 64 MB chunks: 56 GB/s end to end in the probe (32-128 MB alike)

}  // namespace khst

using namespace khst;  // (as every unit that includes this: kh_ctx and kh_trie are the C ABI's, global)

struct kh_ctx {
  int dev = 0;
  int n_cu = 256;  // compute units of the device
  hipStream_t own = nullptr;
  hipStream_t st = nullptr;
  hipStream_t st2 = nullptr;  // leaf hashing, concurrent with the branch topology
  // every entry point that uses the context holds it (recursive: a *_host entry point locks,
  // then calls its device variant, which locks again); a resident handle's calls lock the
  // context the handle was opened on (kh_trie::home)
  std::recursive_mutex mu;
  DevBuf ws_list;  // element builds: the list of leaves to hash (k_leaf_prep -> k_leaf_hash_list)
  DevBuf ws_inject;                    // kh_block_commit: the injection's error word
  unsigned long long inject_tok = 0;   //   and the token the last call writes there on error
  DevBuf ws_arena;  // the build's long leaves (sized once the leaves are hashed)
  DevBuf ws1, ws2, ws3, in_keys, in_vals, in_voff, in_seg, in_kn, in_aux, in_block, out_emit, emit_dev;
  hipEvent_t ev[11] = {};  // [0..5] build stages (st), [6] / [7] forest commit marks, [8] boundaries
                          // ready (st), [9] / [10] leaf kernel start / end (st2)
  unsigned long long* h_pinned = nullptr;  // small pinned staging for syncs
  uint8_t* h_res = nullptr;                // pinned staging of the per-result outputs (grown; a pageable
  size_t h_res_cap = 0;                    // copy of 100k roots cost 20-30 ms of page pinning per build)
  // kh_block_commit: the second context its storage phase runs on, beside the account phase on
  // this one, and the event of the storage roots' injection into the account bodies
  kh_ctx* bsub = nullptr;
  hipEvent_t bev = nullptr;
  std::unique_ptr<Worker> bworker;
  // plain builds on the 32-bit-prefix path do not wait for the tie kernel's flags (SortIO::
  // speculate); a build whose flags were set (repeated keys, a long run) is redone without, and
  // the next spec_off builds do not speculate
  uint32_t spec_off = 0;
  // last build (for emission)
  Topo T{};
  uint64_t last_B = 0;
  uint64_t last_nres = 0;
  BuildInfo binfo;
  // host-input staging (HostStage): a copy stream, a ring of pinned chunks with the event of
  // each chunk's last DMA, the events the stager records (key parts, keys + offsets, values) and
  // the thread that streams the inputs behind the build (created on first use)
  hipStream_t cs = nullptr;
  uint8_t* ring = nullptr;
  hipEvent_t ring_ev[RING_SLOTS] = {};
  bool ring_busy[RING_SLOTS] = {};
  uint32_t ring_next = 0;
  std::vector<hipEvent_t> part_ev;
  std::unique_ptr<Worker> hworker;
  // small host inputs (a commit's ops: HostPack): packed into one pinned buffer, one DMA into
  // in_block; pack_ev marks that DMA (the next pack waits for it before reusing the buffer)
  uint8_t* h_pack = nullptr;
  size_t h_pack_cap = 0;
  hipEvent_t pack_ev = nullptr;
  bool pack_busy = false;
  bool pack_for_block = false;  // kh_block_commit_host -> kh_block_commit: its phases wait for pack_ev
  // kh_verify_ranges: the staged inputs, the hashed node set, the per-range work arrays, the
  // elements and the element build's outputs (none of them a buffer run_build carves itself)
  DevBuf rv_in, rv_store, rv_ws, rv_el, rv_elout, rv_eloutb;
};

namespace khst {

// ---------------------------------------------------------------------------
// the build
// ---------------------------------------------------------------------------
struct BuildArgs {
  const uint8_t* keys;
  uint32_t klen;
  const uint8_t* vals;
  const uint64_t* voff;  // [n+1] offsets, or with vlen: [n] offsets of spans anywhere in vals
  uint64_t n;
  const uint32_t* seg;  // nullable
  uint64_t nseg;
  uint32_t depth0;
  uint32_t flags;
  bool emit;
  const uint32_t* vlen = nullptr;  // per-input value lengths (element builds: spans in a value heap)
  const uint8_t* kn = nullptr;     // variable-length keys (zero-padded to 32 B): nibble counts (list tries)
  struct ElemArgs* el = nullptr;   // element build of a resident forest commit (forest.h; nullable)
  hipEvent_t vals_ready = nullptr; // the values / offsets land later (multi-GPU exchange): wait before reading them
  bool dev_results = false;        // results and counters stay on the device (no host sync at the end)
  bool no_spec = false;            // no speculative sort (SortIO::speculate): the retry of one that failed
  std::function<void()> before_leaves;  // element builds: called (host) right before the leaves are encoded
  std::function<bool()> late_ready;     // ... late values (ElemArgs::late) already on the device: one leaf pass
  HostStage* hs = nullptr;  // host inputs still streaming in (keys in parts, values last; vals_ready unset)
};
// element build (forest.h): inputs are leaves and subtree elements; the capped reference
// of every element node, branch and extension is kept for the forest's records
struct ElemArgs {
  const uint8_t* db;     // [n] EL_LEAF or subtree branch depth (input order)
  const uint64_t* bref;  // [n*4]
  const uint8_t* brl;    // [n]
  const uint8_t* oldd;   // [n] previous anchor depth (EL_NEW: none)
  const uint64_t* cref;  // [n*4] previous capped reference
  const uint8_t* crl;    // [n]
  // [n] nullable: the element's value arrives late (kh_block_commit: an account body that gets
  // its storage root): the other leaves are encoded and hashed before before_leaves
  const uint8_t* late = nullptr;
  DevBuf* out;           // sorted el_db / el_bref / el_brl and lf_ref / lf_rlen (sized by m)
  DevBuf* outb;          // br_ref / br_rlen, ex_ref / ex_rlen (sized by B)
};
struct BuildOut {
  std::vector<uint64_t> res_hash;  // nres*4
  std::vector<uint32_t> res_len;
  std::vector<uint64_t> res_inl;
};

inline uint32_t bits_for(uint64_t nseg) {
  uint32_t b = 0;
  while (b < 64 && (1ULL << b) < nseg) ++b;
  return b;
}

inline float ev_ms(hipEvent_t a, hipEvent_t b) {
  float ms = 0;
  if (hipEventElapsedTime(&ms, a, b) != hipSuccess) return 0;
  return ms;
}

// prims.h for the service units, defined in khst.hip: the scratch a scan / a radix sort needs, the
// exclusive scans of 32- and 64-bit words and the radix sort of (64-bit key, index) pairs
size_t scan_scratch_size(uint64_t n, size_t elem);
size_t radix_scratch_size(uint64_t n);
void scan_u32(const uint32_t* in, uint32_t* out, uint64_t n, uint32_t* total, void* scratch, hipStream_t st);
void scan_u64(const uint64_t* in, uint64_t* out, uint64_t n, uint64_t* total, void* scratch, hipStream_t st);
bool sort_pairs_u64(uint64_t* k0, uint32_t* v0, uint64_t* k1, uint32_t* v1, uint64_t n, int lo_bit, int hi_bit,
                    void* scratch, hipStream_t st);

// Sort n 32-byte keys (with optional segment ids) and drop duplicates, keeping the
// last of equal keys.  Outputs the sorted keys, the input index of each and m.
struct SortIO {
  const uint64_t* K32;
  const uint32_t* seg;
  uint32_t sb;
  uint64_t n;
  uint64_t *ck0, *ck1;
  uint32_t *idx0, *idx1;
  uint64_t* skey;
  uint32_t* sseg;
  void* rs_scratch;
  void* scan_scratch;
  unsigned long long* ctr;
  const uint8_t* kn;  // variable-length keys: nibble counts (input order; nullable)
  bool ck_ready = false;  // ck_path: ck0/idx0 already hold the 32-bit sort keys (k_hash_keys_ck)
  bool ck_path = false;   // unsegmented plain build: sort (32-bit prefix, idx) only, never gather the keys
  bool ck_made = false;   // composite path: ck0 / idx0 and the radix header already made (k_f_keys_ck)
  // 64-bit composite path: the radix range is bits [rs_lo, 64) -- 40 (the leading 24 bits) where
  // keys are few per segment, the tie kernel then orders the runs of equal leading 24 bits
  int rs_lo = 32;
  // ck path: the words are sorted on their bits from tsh up (8: hashed keys, few enough that
  // runs of equal top-24 bits stay rare; the tie kernel orders them)
  uint32_t tsh = 0;
  // a device word copied to the host with the first sync's flags (c->h_pinned[1]): the
  // caller's check of earlier stream work, read without a sync of its own (nullable)
  const unsigned long long* chk = nullptr;
  // ck_path: no sync for the tie kernel's flags: the sort proceeds as if no key repeats and no
  // run is too long (hashed keys: the rule); the caller reads the flags at its next sync
  // (CTR_TIE) and redoes the build without speculating if either is set
  bool speculate = false;
  // out
  uint8_t* u = nullptr;  // ck_path: boundary values, written for the tie runs' inner boundaries
  uint32_t depth0 = 0;
  const uint32_t* sck = nullptr;  // ck_path: the sorted 32-bit key prefixes (skey not gathered)
  bool ties_u = false;            // u holds the tie runs' boundaries (k_lcp skips them)
  bool all_u = false;             // u holds every boundary (k_lcp only clears a too-long run's)
  uint64_t m;
  uint32_t* sidx;
  bool fallback;
  // Declares the sort's scratch into the caller's workspace: nk keys and their indices, skey of
  // skey_words words, sseg for a segmented sort, the radix and scan scratch for radix_n and
  // scan_n entries, and ctr_n counters (0: ctr is part of the caller's own counter block)
  void declare(Layout& L, uint64_t nk, uint64_t skey_words, bool segmented, uint64_t radix_n, uint64_t scan_n,
               uint64_t ctr_n) {
    L.add_all(nk, ck0, ck1, idx0, idx1);
    L.add(skey, skey_words);
    L.add(sseg, nk, segmented);
    L.add(rs_scratch, radix_scratch_size(radix_n));
    L.add(scan_scratch, scan_scratch_size(scan_n, 8));
    if (ctr_n) L.add(ctr, ctr_n);
  }
};
void sort_dedup(kh_ctx* c, SortIO& S);
void run_build(kh_ctx* c, const BuildArgs& A, BuildOut& O, kh_stats* stats);
// kec256 of n raw keys of klen bytes into K (KH_HASH_KEYS)
void hash_keys_to(hipStream_t st, const uint8_t* keys, uint32_t klen, uint64_t n, uint64_t* K);

// the context the *_host entry points share on a device, and the calling thread's device
kh_ctx* shared_ctx(int dev);
int current_device();

#define API_TRY(...)                                                    \
  try {                                                                 \
    __VA_ARGS__;                                                        \
    return KH_OK;                                                       \
  } catch (KhError & e) {                                               \
    return set_err(e.code, e.msg);                                      \
  } catch (std::bad_alloc&) {                                           \
    return set_err(KH_ENOMEM, "host allocation failed");                \
  } catch (std::exception & e) {                                        \
    return set_err(KH_EINTERNAL, e.what());                             \
  }

// packed host bytes and their offsets, rebased, into the context's in_vals / in_voff
void stage_packed(kh_ctx* c, const uint8_t* data, const uint64_t* off, uint64_t n, std::vector<uint64_t>& rel);

// an emitted node set of tn nodes and tb encoding bytes in one device buffer: hashes | rlp | off
struct EmitLayout {
  uint8_t* hashes;
  uint8_t* rlp;
  uint64_t* off;
};
inline EmitLayout emit_layout(DevBuf& out, uint64_t tn, uint64_t tb) {
  uint8_t* oh = (uint8_t*)out.p;
  uint8_t* orlp = oh + ((tn * 32 + 255) & ~255ULL);
  uint64_t* ooff = (uint64_t*)(orlp + ((tb + 255) & ~255ULL));
  return EmitLayout{oh, orlp, ooff};
}

// ---- versioned commits (Ledger.executeBlock flushes a parallel attempt and, when
// its root does not validate, re-executes sequentially from the SAME parent state,
// Ledger.scala:237-271; validateBlockAfterExecution rejects a block, :603-620; TrieAccounts.rootHash
// flushes a COPY, TrieAccounts.scala:73-80).  A savepoint opens an undo journal: every commit
// after it saves the records it rewrites in place and logs the anchor-map slots it changes, so a
// rollback restores the version of the savepoint in O(changed records), not O(resident trie).
// New records, heap bytes and node ids are appended past the savepoint's ends and simply cut off.
struct JSeg {  // one journaled commit: its saved records and map-slot log ranges (entries)
  uint64_t rpos = 0, rn = 0;  // saved records [rpos, rpos + rn) of jidx / jrec
  uint64_t dpos = 0, dn = 0;  // map log: the deletes (tombstones) ...
  uint64_t ipos = 0, in = 0;  // ... and the inserts, 3 words per entry (slot, old tag, old record)
};
struct Savepoint {
  uint64_t rn = 0, heap_n = 0, nleaves = 0, mused = 0, rdead = 0, map_epoch = 0, nstubs = 0;
  uint8_t root[32] = {};
  std::vector<uint32_t> tries;  // the last commit's touched tries and roots (kh_forest_last_roots)
  std::vector<uint8_t> roots;
  size_t seg0 = 0;              // journal fill at the savepoint
  uint64_t jrec0 = 0, jmap0 = 0;
  bool em_saved = false;        // the write-back set of the savepoint's version, kept when a later
  bool em_valid = false;        // commit replaced it (kh_trie_emit_nodes after a rollback)
  DevBuf em;
  uint64_t em_n = 0, em_bytes = 0;
};

}  // namespace khst

struct kh_trie {
  kh_ctx* c = nullptr;     // the context its commits run on (kh_block_commit moves the storage phase for a call)
  kh_ctx* home = nullptr;  // the context it was opened on
  // Handles opened through the host entry points (the shared context: the JVM's tries) run on a
  // private context of their own (priv: streams and workspaces) and serialise on their own
  // mutex, so commits on different handles overlap on the GPU (TxProcessor.scala:28-35 drives
  // tries from many workers; SURVEY §8b: each handle its own HIP stream).  Handles opened on a
  // caller's context run on it and hold its mutex (the caller owns that stream's ordering).
  std::recursive_mutex own_mu;
  std::recursive_mutex* lk = nullptr;  // every call on the handle holds *lk
  kh_ctx* priv = nullptr;
  uint32_t flags = 0;  // KH_HASH_KEYS: the trie's key encoder; KH_EMIT_NODES: keep each commit's write-back set
  bool forest = false;
  uint32_t tid_bits = 0;  // forests: bits of the trie ids committed so far (+ headroom; 0: none yet)
  uint32_t lo24_off = 0;  // commits left without the 24-bit op sort (a run past the tie kernel fell back)
  DevBuf recs, touched, replaced;  // node records (forest.h Recs: 128 B each), per-commit flags
  uint64_t rcap = 0, rn = 0, rdead = 0;
  DevBuf mslots;  // anchor map: 16-byte (tag, record) slots
  uint64_t mcap = 0, mused = 0;
  DevBuf heap;
  uint64_t heap_n = 0;
  uint64_t nleaves = 0;
  // a partial handle (forest.h EL_STUB): its live stubs, and the (trie id, hash to fetch) pairs of
  // the last commit if it was refused with KH_ENODE (kh_trie_missing)
  uint64_t nstubs = 0;
  std::vector<uint32_t> miss_tries;
  std::vector<uint8_t> miss_hashes;
  uint8_t root[32] = {};
  DevBuf ws, elout, eloutb, em;  // commit scratch, element-build outputs, last write-back set
  DevBuf tlb, ebuf, tbuf, ubuf, selb, merr;  // touched list, elements, trie ids + roots, upsert offsets, selections
  DevBuf gbuf;                                // batched get: keys, records, lengths, scan scratch
  DevBuf xbuf;                                // node export / nodes by hash: the emitted set (hashes | rlp | off)
  uint64_t epoch = 1;  // commits, rollbacks and compactions so far (+ 1): what a kh_export_cursor is bound to
  uint64_t em_n = 0, em_bytes = 0;
  bool em_valid = false;
  uint64_t ntl_hint = 0;  // touched records of the last commit (sizes the next element buffer)
  std::vector<uint32_t> tries;  // last commit: touched tries and their roots
  std::vector<uint8_t> roots;
  uint32_t* d_tries = nullptr;  // ... the same on the device (in tbuf; the block commit's injection reads them)
  uint64_t* d_roots = nullptr;
  // versioned commits: open savepoints (innermost last) and the journal of the commits since the
  // outermost one
  std::vector<std::unique_ptr<Savepoint>> sps;
  std::vector<JSeg> jsegs;
  DevBuf jidx, jrec, jmap;  // saved record ids (u32), saved records (128 B), map-slot log (3 u64)
  uint64_t jrec_n = 0, jmap_n = 0;
  uint64_t map_epoch = 0;   // anchor-map rebuilds so far (a rebuild voids the slot log)
  bool flags_dirty = false; // a descent marked records and its commit did not finish
  DevBuf em_spare;          // the write-back buffer a savepoint's saved set rotates with
  // a commit's tail left in flight (Commit::early_roots, no write-back set): its records and anchor
  // map are written after the call returned; pend (pinned) gets the map's error flag and fresh
  // slot count, read by trie_settle before the host next needs them
  hipEvent_t ev_roots = nullptr, pend_ev = nullptr;
  unsigned long long* pend = nullptr;
  bool pend_valid = false, pend_fresh = false;
  // such a tail failed (its anchor map is not trustworthy): every later call refuses the
  // handle (KH_EINTERNAL) except kh_trie_free
  bool broken = false;
  kh_trie() = default;
  kh_trie(const kh_trie&) = delete;
  kh_trie& operator=(const kh_trie&) = delete;
  ~kh_trie() {
    if (ev_roots) (void)hipEventDestroy(ev_roots);
    if (pend_ev) (void)hipEventDestroy(pend_ev);
    if (pend) (void)hipHostFree(pend);
    if (priv) (void)kh_ctx_destroy(priv);
  }
};

namespace khst {

// the in-flight tail of the last commit: its map error and fresh slots (before mused is read)
void trie_settle(kh_trie* h);

// every entry point on a resident handle serialises on its home context (khst.h: reentrant)
#define HANDLE_LOCK(h) std::lock_guard<std::recursive_mutex> handle_lock_(*(h)->lk)
// both handles of a block commit: one mutex when they share a context, else both (std::lock:
// no deadlock against another call locking them in the other order)
struct PairLock {
  std::unique_lock<std::recursive_mutex> a, b;
  PairLock(std::recursive_mutex* x, std::recursive_mutex* y) : a(*x, std::defer_lock), b(*y, std::defer_lock) {
    if (x == y)
      a.lock();
    else
      std::lock(a, b);
  }
};

inline Recs recs_of(kh_trie* h) {
  return recs_at((uint8_t*)h->recs.p);
}
inline AMap map_of(kh_trie* h) { return AMap{{(uint8_t*)h->mslots.p}, {(uint8_t*)h->mslots.p}, h->mcap - 1}; }

// a handle's arrays: growth (keeping the first `keep` bytes), the anchor map rebuilt with headroom, journal room
void regrow(DevBuf& b, size_t keep, size_t bytes, hipStream_t st);
void recs_reserve(kh_trie* h, uint64_t need);
void map_rebuild(kh_trie* h, uint64_t headroom);
JSeg journal_reserve(kh_trie* h, uint64_t nrec, uint64_t nmap);
// a fresh handle on c; a handle moved to a private context of its own
kh_trie* trie_new(kh_ctx* c, uint32_t flags, bool forest);
void make_private(kh_trie* h);
// a batched query's arguments checked, its keys and trie ids staged on the device
void query_check(const kh_trie* h, const uint32_t* trie, uint32_t klen, uint64_t n, bool hash);
void stage_query_keys(kh_ctx* c, const uint32_t* trie, const uint8_t* keys, uint32_t klen, uint64_t n,
                      uint8_t*& dk, uint32_t*& dt);
// kh_trie_fill_ranges (fillrange.h): n entries (device arrays; trie ids for a forest) as the upserts
// of one commit in fill mode, under a savepoint of its own.  accept() runs after the commit, the
// new roots in h->d_tries / h->d_roots, and says keep or roll back.  Returns FILL_KEPT, or with the
// handle as it was: FILL_MISSING (an entry reached a stub that is not inside: FillMode::miss, the
// hashes in the handle's missing list), FILL_MOVED (a stub of unknown kind would have been
// re-anchored: the tries in the missing list), FILL_REFUSED (accept said no).
enum FillResult { FILL_KEPT = 0, FILL_MISSING = 1, FILL_MOVED = 2, FILL_REFUSED = 3 };
FillResult commit_fill(kh_trie* h, const uint32_t* d_trie, const uint8_t* d_keys, const uint8_t* d_vals,
                       const uint64_t* d_voff, uint64_t n, const FillMode& fm, const std::function<bool()>& accept);

}  // namespace khst

// Kernels one unit defines and another launches, declared once (none is a template).  khst.hip's:
__global__ void k_kec_batch(const uint8_t* data, const uint64_t* off, uint64_t n, uint64_t* out);
__global__ void k_u32_to_u64(const uint32_t* in, uint64_t n, uint64_t* out);
__global__ void k_map_delete(AMap M, Recs R, const uint32_t* list, uint64_t n, const uint32_t* list2, uint64_t n2,
                             uint32_t* touched, uint8_t* replaced, uint64_t* mlog);
__global__ void k_map_insert(AMap M, Recs R, uint64_t base, uint64_t nb, const uint32_t* list, uint64_t n,
                             unsigned long long* err, unsigned long long* used, uint64_t* mlog);
// load_kernels.hip's, which a commit in fill mode (kh_trie_fill_ranges) runs in place of k_f_descend
// and k_stub_missing, and after k_f_elem_flags on the write-back selection:
__global__ void k_fill_descend(FOps O, AMap M, Recs R, FillMode F, uint32_t* touched, uint8_t* replaced,
                               uint32_t* tlist, unsigned long long* ctr, uint8_t* vbf);
__global__ void k_fill_missing(Recs R, FillMode F, const uint32_t* list, uint64_t n, uint64_t cap, uint32_t* out_trie,
                               uint64_t* out_hash, unsigned long long* cnt);
__global__ void k_fill_sel(Topo T, Elems E, const uint32_t* tries, AMap M, Recs R, uint64_t B, uint8_t* sel);
// export_kernels.hip's, which kh_trie_prove runs in list mode over its hits:
__global__ void k_export_sizes(AMap M, Recs R, const uint8_t* heap, const uint64_t* list, uint64_t r0, uint64_t n,
                               uint32_t filter, uint32_t* stash, uint32_t* cnt, uint32_t* bytes);
__global__ void k_export_write(Recs R, const uint8_t* heap, const uint64_t* list, uint64_t r0, uint64_t n,
                               uint32_t filter, const uint32_t* stash, const uint32_t* cpos, const uint32_t* bpos,
                               uint8_t* hashes, uint8_t* rlp, uint64_t* off, uint8_t* found, const uint64_t* bpos64);
