// Device check of khipu_amd/csrc/prims.h (the stable LSD radix sort and the exclusive scans) and
// of the wave helpers of wave.h against plain host code.  Test infrastructure only
// (tests/test_prims_plan.py, tests/test_gpu_prims.py; built by __graft_entry__.build()).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -o scripts/prims_check scripts/prims_check.hip
//   scripts/prims_check plan     -> the case table and the header's constants, one JSON document
//                                   (no HIP call: runs without a device)
//   scripts/prims_check sort32 | sort64 | scan | wave
//                                -> one JSON line per case (name, n, parameters, ok; on a mismatch
//                                   the first differing position with the expected and the actual
//                                   values), then a summary line with the launches per kernel;
//                                   exit status 1 if a case failed
// Every device buffer lies between two 4,096-byte guards of a sentinel that are verified after
// each case; the scratch buffers have exactly the sizes radix_scratch_bytes / scan_scratch_bytes
// give.  After the first HIP error the program reports it and exits without another launch.
#include <hip/hip_runtime.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

static std::map<std::string, uint64_t> g_launches;

[[noreturn]] static void die_hip(hipError_t e, const char* what) {
  printf("{\"hip_error\": \"%s\", \"at\": \"%s\"}\n", hipGetErrorString(e), what);
  fflush(stdout);
  _exit(3);  // (no destructor, no further HIP call)
}
#define CK(x)                               \
  do {                                      \
    hipError_t e_ = (x);                    \
    if (e_ != hipSuccess) die_hip(e_, #x);  \
  } while (0)

// launches per kernel, keyed by the kernel's address (labels: kernel_labels() below, once
// prims.h is known; a kernel without a label counts under the launch site's spelling)
static void count_launch(const void* kernel, const char* spelled);

// prims.h launches through hipLaunchKernelGGL: counted and checked here
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(k, g, b, sh, st, ...)          \
  do {                                                    \
    count_launch((const void*)(k), #k);                   \
    (k)<<<(g), (b), (sh), (st)>>>(__VA_ARGS__);           \
    hipError_t le_ = hipGetLastError();                   \
    if (le_ != hipSuccess) die_hip(le_, #k);              \
  } while (0)

#include "../khipu_amd/csrc/prims.h"

using namespace khst;

// ---------------------------------------------------------------------------
// host helpers
// ---------------------------------------------------------------------------
__global__ void k_w_reduce(const uint32_t*, const uint64_t*, uint32_t*, uint32_t*, uint64_t*);
__global__ void k_w_claim(unsigned long long*, const uint8_t*, uint64_t*, int);
__global__ void k_w_atomic(unsigned long long*, const uint64_t*);
__global__ void k_w_bscan(const uint32_t*, const uint32_t*, uint32_t*, uint32_t*, uint32_t*);

// every kernel of prims.h in every form radix_sort_pairs and scan_exclusive launch: name<width,
// keys per thread> (k_rs_pass<uint64_t, RS_BIG_ITEMS> does not exist: its LDS would not fit)
static const std::map<const void*, std::string>& kernel_labels() {
  static std::map<const void*, std::string> m;
  if (!m.empty()) return m;
  auto rs = [&](const void* f, const char* name, int bits, int items) {
    char b[64];
    snprintf(b, sizeof b, "%s<u%d,%d>", name, bits, items);
    m[f] = b;
  };
  rs((const void*)k_rs_hist_all<uint32_t, RS_SMALL_ITEMS>, "k_rs_hist_all", 32, RS_SMALL_ITEMS);
  rs((const void*)k_rs_hist_all<uint32_t, RS_ITEMS>, "k_rs_hist_all", 32, RS_ITEMS);
  rs((const void*)k_rs_hist_all<uint64_t, RS_SMALL_ITEMS>, "k_rs_hist_all", 64, RS_SMALL_ITEMS);
  rs((const void*)k_rs_hist_all<uint64_t, RS_ITEMS>, "k_rs_hist_all", 64, RS_ITEMS);
  rs((const void*)k_rs_pass<uint32_t, RS_SMALL_ITEMS>, "k_rs_pass", 32, RS_SMALL_ITEMS);
  rs((const void*)k_rs_pass<uint32_t, RS_ITEMS>, "k_rs_pass", 32, RS_ITEMS);
  rs((const void*)k_rs_pass<uint32_t, RS_BIG_ITEMS>, "k_rs_pass", 32, RS_BIG_ITEMS);
  rs((const void*)k_rs_pass<uint64_t, RS_SMALL_ITEMS>, "k_rs_pass", 64, RS_SMALL_ITEMS);
  rs((const void*)k_rs_pass<uint64_t, RS_ITEMS>, "k_rs_pass", 64, RS_ITEMS);
  m[(const void*)k_scan_small<uint32_t>] = "k_scan_small<u32>";
  m[(const void*)k_scan_small<uint64_t>] = "k_scan_small<u64>";
  m[(const void*)k_scan_tiles<uint32_t>] = "k_scan_tiles<u32>";
  m[(const void*)k_scan_tiles<uint64_t>] = "k_scan_tiles<u64>";
  m[(const void*)k_scan_add_sums<uint32_t>] = "k_scan_add_sums<u32>";
  m[(const void*)k_scan_add_sums<uint64_t>] = "k_scan_add_sums<u64>";
  m[(const void*)k_scan_add<uint32_t>] = "k_scan_add<u32>";
  m[(const void*)k_scan_add<uint64_t>] = "k_scan_add<u64>";
  m[(const void*)k_scan_total<uint32_t>] = "k_scan_total<u32>";
  m[(const void*)k_scan_total<uint64_t>] = "k_scan_total<u64>";
  m[(const void*)k_scan_small3] = "k_scan_small3";
  m[(const void*)k_w_reduce] = "k_w_reduce";
  m[(const void*)k_w_claim] = "k_w_claim";
  m[(const void*)k_w_atomic] = "k_w_atomic";
  m[(const void*)k_w_bscan] = "k_w_bscan";
  return m;
}
static void count_launch(const void* kernel, const char* spelled) {
  auto it = kernel_labels().find(kernel);
  ++g_launches[it != kernel_labels().end() ? it->second : std::string("unlabelled ") + spelled];
}

struct Rng {
  uint64_t s;
  explicit Rng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 0x1234567ull) {}
  uint64_t next() {  // splitmix64
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
};

constexpr size_t GUARD = 4096;
constexpr int GUARD_BYTE = 0xA5;

// A device buffer of up to `cap` bytes between two guards.  set(bytes) places the end guard
// right after the first `bytes` bytes; check() reads both guards back.
struct Arena {
  char* base = nullptr;
  size_t cap = 0, cur = 0;
  const char* name = "";
  void init(const char* nm, size_t cap_bytes) {
    name = nm;
    cap = cap_bytes;
    CK(hipMalloc((void**)&base, cap + 2 * GUARD));
    CK(hipMemset(base, GUARD_BYTE, GUARD));
  }
  void* set(size_t bytes) {
    if (bytes > cap) {
      printf("{\"error\": \"arena %s: %zu > %zu\"}\n", name, bytes, cap);
      fflush(stdout);
      _exit(4);
    }
    cur = bytes;
    CK(hipMemset(base + GUARD + bytes, GUARD_BYTE, GUARD));
    return base + GUARD;
  }
  void* ptr() const { return base + GUARD; }
  bool check() const {
    unsigned char h[2 * GUARD];
    CK(hipMemcpy(h, base, GUARD, hipMemcpyDeviceToHost));
    CK(hipMemcpy(h + GUARD, base + GUARD + cur, GUARD, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < 2 * GUARD; ++i)
      if (h[i] != GUARD_BYTE) return false;
    return true;
  }
};

static std::string fmt(const char* f, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, f);
  vsnprintf(buf, sizeof buf, f, ap);
  va_end(ap);
  return buf;
}

static void print_launches() {
  bool first = true;
  for (auto& kv : g_launches) {
    printf("%s\"%s\": %llu", first ? "" : ", ", kv.first.c_str(), (unsigned long long)kv.second);
    first = false;
  }
}

static double now_ms() {
  using namespace std::chrono;
  return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}

// ---------------------------------------------------------------------------
// the case tables (sizes from the header's constants)
// ---------------------------------------------------------------------------
static const char* const DISTS[] = {"uniform", "equal",   "two_digits", "absent_digit",
                                    "sorted",  "reverse", "ties16",     "low_byte"};
enum { D_UNIFORM, D_EQUAL, D_TWO, D_ABSENT, D_SORTED, D_REVERSE, D_TIES16, D_LOWBYTE, N_DISTS };
static const char* const SCRATCH_MODES[] = {"filled_ff", "hdr_zeroed"};

struct SortCase {
  uint64_t n;
  int lo, hi, dist, scratch;     // scratch: 0 whole scratch 0xFF, hdr_zeroed = false; 1 header zeroed by the caller
  std::vector<uint64_t> steps;   // a sequence of sorts on one untouched scratch (n: the largest)
};

static std::vector<uint64_t> sort_small_sizes() {
  return {0,    1,    2,    63,   64,   65,   255,  256,  257,  1023, 1024, 1025,
          4095, 4096, 4097, RS_SMALL_N - 1, RS_SMALL_N, RS_SMALL_N + 1};
}

static std::vector<SortCase> sort_cases(int key_bytes) {
  std::vector<std::pair<int, int>> ranges;
  if (key_bytes == 4)
    ranges = {{0, 32}, {8, 32}};
  else
    ranges = {{32, 64}, {40, 64}, {0, 64}, {0, 8}, {0, 24}, {0, 40}};
  std::vector<SortCase> cs;
  for (uint64_t n : sort_small_sizes())
    for (auto r : ranges)
      for (int d = 0; d < N_DISTS; ++d)
        for (int sm = 0; sm < 2; ++sm) cs.push_back({n, r.first, r.second, d, sm, {}});
  if (key_bytes == 4) {  // the 8,192-key tiles: five cases and the sequence's middle step
    cs.push_back({RS_BIG_N - 1, 0, 32, D_UNIFORM, 0, {}});
    cs.push_back({RS_BIG_N, 8, 32, D_UNIFORM, 1, {}});
    cs.push_back({RS_BIG_N, 0, 32, D_TIES16, 0, {}});
    cs.push_back({RS_BIG_N + 1, 0, 32, D_TIES16, 1, {}});
    cs.push_back({RS_BIG_N + 1, 8, 32, D_ABSENT, 0, {}});
    cs.push_back({RS_BIG_N, 0, 32, D_TIES16, 0, {RS_SMALL_N, RS_BIG_N, 4097}});
    cs.push_back({RS_SMALL_N + 1, 8, 32, D_UNIFORM, 0, {1025, RS_SMALL_N + 1, 257}});
  } else {  // the same sizes once: 64-bit keys stay on RS_ITEMS keys per thread
    cs.push_back({RS_BIG_N - 1, 32, 64, D_UNIFORM, 0, {}});
    cs.push_back({RS_BIG_N, 0, 64, D_TIES16, 1, {}});
    cs.push_back({RS_BIG_N + 1, 40, 64, D_UNIFORM, 0, {}});
    cs.push_back({RS_BIG_N, 32, 64, D_TIES16, 0, {RS_SMALL_N, RS_BIG_N, 4097}});
    cs.push_back({RS_SMALL_N + 1, 0, 64, D_UNIFORM, 0, {1025, RS_SMALL_N + 1, 257}});
  }
  return cs;
}

static std::string sort_name(int key_bytes, const SortCase& c) {
  return fmt("sort%d/%s/n%llu/b%d-%d/%s%s", key_bytes * 8, DISTS[c.dist], (unsigned long long)c.n, c.lo, c.hi,
             SCRATCH_MODES[c.scratch], c.steps.empty() ? "" : "/sequence");
}

static const char* const SCAN_INPUTS[] = {"ones", "random20", "large"};  // large: u32 sums pass 2^32, u64 elements above 2^32
struct ScanCase {
  uint64_t n;
  int elem_bytes, input;
  bool small_ok;
};
constexpr uint64_t SCAN_TWO_MAX = SCAN_TWO_MAX_TILES * SCAN_TILE;

static std::vector<uint64_t> scan_small_sizes() {
  return {0,    1,    2,    1023, 1024, 1025, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1,
          8191, 8192, 8193, SCAN_SMALL_MAX - 1, SCAN_SMALL_MAX, SCAN_SMALL_MAX + 1};
}

static std::vector<ScanCase> scan_cases() {
  std::vector<ScanCase> cs;
  for (uint64_t n : scan_small_sizes())
    for (int eb : {4, 8})
      for (int in = 0; in < 3; ++in)
        for (int so = 1; so >= 0; --so) cs.push_back({n, eb, in, so != 0});
  // two launches -> recursive: each size once per width (the inputs spread over them)
  cs.push_back({SCAN_TWO_MAX - 1, 4, 0, true});
  cs.push_back({SCAN_TWO_MAX - 1, 8, 2, true});
  cs.push_back({SCAN_TWO_MAX, 4, 2, true});
  cs.push_back({SCAN_TWO_MAX, 8, 1, true});
  cs.push_back({SCAN_TWO_MAX + 1, 4, 1, true});
  cs.push_back({SCAN_TWO_MAX + 1, 8, 2, true});
  return cs;
}
static std::string scan_name(const ScanCase& c) {
  return fmt("scan%d/%s/n%llu/%s", c.elem_bytes * 8, SCAN_INPUTS[c.input], (unsigned long long)c.n,
             c.small_ok ? "small_ok" : "no_small");
}
static std::vector<uint64_t> small3_sizes() { return {1, 1025, SCAN_SMALL_MAX}; }

static const char* const WAVE_CASES[] = {"wave_max_u32",          "wave_sum_u32",           "wave_sum_u64",
                                         "wave_claim/all",        "wave_claim/none",        "wave_claim/one",
                                         "wave_claim/alternating", "wave_claim/divergent_all", "wave_claim/divergent_third",
                                         "wave_atomic_add",       "wave_atomic_add/zero",   "block_exclusive_scan_u32"};
static const int MAX_LANES[] = {0, 15, 16, 31, 32, 63};

static int do_plan() {
  int bad = 0;
  printf("{\"constants\": {\"RS_SMALL_N\": %llu, \"RS_BIG_N\": %llu, \"RS_SMALL_ITEMS\": %d, \"RS_ITEMS\": %d, "
         "\"RS_BIG_ITEMS\": %d, \"RS_HDR_BYTES\": %zu, \"SCAN_TILE\": %d, \"SCAN_SMALL_MAX\": %llu, "
         "\"SCAN_TWO_MAX_TILES\": %llu},\n",
         (unsigned long long)RS_SMALL_N, (unsigned long long)RS_BIG_N, RS_SMALL_ITEMS, RS_ITEMS, RS_BIG_ITEMS,
         RS_HDR_BYTES, SCAN_TILE, (unsigned long long)SCAN_SMALL_MAX, (unsigned long long)SCAN_TWO_MAX_TILES);
  printf(" \"modes\": {\n");
  for (int kb : {4, 8}) {
    printf("  \"sort%d\": [\n", kb * 8);
    auto cs = sort_cases(kb);
    for (size_t i = 0; i < cs.size(); ++i) {
      const SortCase& c = cs[i];
      const int items = radix_items(c.n, kb);
      // 64-bit keys never take the RS_BIG_ITEMS tiles (their LDS staging would not fit)
      if (kb == 8 && c.n >= RS_BIG_N && items != RS_ITEMS) bad = 1;
      printf("   {\"name\": \"%s\", \"n\": %llu, \"lo\": %d, \"hi\": %d, \"dist\": \"%s\", \"scratch\": \"%s\", "
             "\"items\": %d, \"tiles\": %llu, \"scratch_bytes\": %zu, \"steps\": [",
             sort_name(kb, c).c_str(), (unsigned long long)c.n, c.lo, c.hi, DISTS[c.dist], SCRATCH_MODES[c.scratch],
             items, (unsigned long long)radix_tiles(c.n, kb), radix_scratch_bytes(c.n));
      for (size_t j = 0; j < c.steps.size(); ++j)
        printf("%s{\"n\": %llu, \"items\": %d}", j ? ", " : "", (unsigned long long)c.steps[j],
               radix_items(c.steps[j], kb));
      printf("]}%s\n", i + 1 < cs.size() ? "," : "");
    }
    printf("  ],\n");
  }
  printf("  \"scan\": [\n");
  for (const ScanCase& c : scan_cases())
    printf("   {\"name\": \"%s\", \"n\": %llu, \"elem_bytes\": %d, \"input\": \"%s\", \"small_ok\": %s, "
           "\"scratch_bytes\": %zu},\n",
           scan_name(c).c_str(), (unsigned long long)c.n, c.elem_bytes, SCAN_INPUTS[c.input],
           c.small_ok ? "true" : "false", scan_scratch_bytes(c.n, c.elem_bytes));
  {
    auto s3 = small3_sizes();
    for (size_t i = 0; i < s3.size(); ++i)
      printf("   {\"name\": \"scan_small3/n%llu\", \"n\": %llu, \"elem_bytes\": 0, \"input\": \"mixed\", "
             "\"small_ok\": true, \"scratch_bytes\": 0}%s\n",
             (unsigned long long)s3[i], (unsigned long long)s3[i], i + 1 < s3.size() ? "," : "");
  }
  printf("  ],\n  \"wave\": [\n");
  const size_t nw = sizeof WAVE_CASES / sizeof *WAVE_CASES;
  for (size_t i = 0; i < nw; ++i)
    printf("   {\"name\": \"%s\", \"n\": %d}%s\n", WAVE_CASES[i], RS_THREADS, i + 1 < nw ? "," : "");
  printf("  ]\n },\n \"radix_items_64bit_big_ok\": %s}\n", bad ? "false" : "true");
  return bad;
}

// ---------------------------------------------------------------------------
// sorts
// ---------------------------------------------------------------------------
static uint64_t field_mask(int bits) { return bits >= 64 ? ~0ull : ((1ull << bits) - 1); }

// n keys whose bits [lo, hi) follow `dist` and whose other bits are random (the sort must
// ignore and keep them); tile: the keys of one radix tile at this n (absent_digit)
template <typename K>
static void gen_keys(std::vector<K>& keys, uint64_t n, int lo, int hi, int dist, uint64_t tile, uint64_t seed) {
  const int fb = hi - lo;
  const uint64_t fm = field_mask(fb);
  Rng r(seed);
  uint64_t pool[16];
  for (auto& p : pool) p = r.next();
  keys.resize(n);
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t junk = r.next();
    uint64_t f = 0;
    switch (dist) {
      case D_UNIFORM: f = r.next(); break;
      case D_EQUAL: f = 0x5A5A5A5A5A5A5A5Aull; break;
      case D_TWO: f = (r.next() & 1) ? 0x1111111111111111ull : 0xEEEEEEEEEEEEEEEEull; break;
      case D_ABSENT: {  // digit 0x37: half the keys of an even tile, none of an odd tile (every pass's digit)
        f = r.next();
        if ((i / tile) & 1) {
          for (int b = 0; b < 8; ++b)
            if (((f >> (8 * b)) & 0xFF) == 0x37) f ^= 0x0Full << (8 * b);  // 0x37 -> 0x38
        } else if (r.next() & 1) {
          f = 0x3737373737373737ull;
        }
        break;
      }
      case D_SORTED: f = (uint64_t)((((unsigned __int128)i) << fb) / n); break;
      case D_REVERSE: f = (uint64_t)((((unsigned __int128)(n - 1 - i)) << fb) / n); break;
      case D_TIES16: f = pool[r.next() & 15]; break;
      case D_LOWBYTE: f = (0x5A5A5A5A5A5A5A5Aull & ~0xFFull) | (r.next() & 0xFF); break;
    }
    keys[i] = (K)((junk & ~(fm << lo)) | ((f & fm) << lo));
  }
}

template <typename K>
struct SortBufs {
  Arena k0, k1, v0, v1, scr;
  void init(uint64_t max_n) {
    k0.init("k0", max_n * sizeof(K));
    k1.init("k1", max_n * sizeof(K));
    v0.init("v0", max_n * 4);
    v1.init("v1", max_n * 4);
    scr.init("scratch", radix_scratch_bytes(max_n));
  }
};

constexpr int PREFILL = 0xEE;

// One sort of `keys` with identity values on bits [lo, hi).  Returns "" or the mismatch as JSON
// fields.  The scratch is the caller's (placed and filled, or left as the sort before left it).
template <typename K>
static std::string sort_once(SortBufs<K>& B, const std::vector<K>& keys, int lo, int hi, bool hdr_zeroed) {
  const uint64_t n = keys.size();
  const int fb = hi - lo;
  const uint64_t fm = field_mask(fb);
  const int npass = n <= 1 ? 0 : (fb + 7) / 8;
  std::vector<uint32_t> vals(n);
  for (uint64_t i = 0; i < n; ++i) vals[i] = (uint32_t)i;
  K* k0 = (K*)B.k0.set(n * sizeof(K));
  K* k1 = (K*)B.k1.set(n * sizeof(K));
  uint32_t* v0 = (uint32_t*)B.v0.set(n * 4);
  uint32_t* v1 = (uint32_t*)B.v1.set(n * 4);
  if (n) {
    CK(hipMemcpy(k0, keys.data(), n * sizeof(K), hipMemcpyHostToDevice));
    CK(hipMemcpy(v0, vals.data(), n * 4, hipMemcpyHostToDevice));
    CK(hipMemset(k1, PREFILL, n * sizeof(K)));
    CK(hipMemset(v1, PREFILL, n * 4));
  }
  const bool flip = radix_sort_pairs<K>(k0, v0, k1, v1, n, lo, hi, B.scr.ptr(), (hipStream_t)0, hdr_zeroed);
  CK(hipDeviceSynchronize());
  std::vector<K> hk[2] = {std::vector<K>(n), std::vector<K>(n)};
  std::vector<uint32_t> hv[2] = {std::vector<uint32_t>(n), std::vector<uint32_t>(n)};
  if (n) {
    CK(hipMemcpy(hk[0].data(), k0, n * sizeof(K), hipMemcpyDeviceToHost));
    CK(hipMemcpy(hk[1].data(), k1, n * sizeof(K), hipMemcpyDeviceToHost));
    CK(hipMemcpy(hv[0].data(), v0, n * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(hv[1].data(), v1, n * 4, hipMemcpyDeviceToHost));
  }
  for (const Arena* a : {&B.k0, &B.k1, &B.v0, &B.v1, &B.scr})
    if (!a->check()) return fmt("\"what\": \"guard of %s overwritten\"", a->name);
  if (flip != (bool)(npass & 1))
    return fmt("\"what\": \"flip\", \"expected\": %d, \"actual\": %d", npass & 1, (int)flip);
  // reference: std::stable_sort of (sort field, input index)
  struct E {
    uint64_t f;
    uint32_t i;
  };
  std::vector<E> ref(n);
  for (uint64_t i = 0; i < n; ++i) ref[i] = {((uint64_t)keys[i] >> lo) & fm, (uint32_t)i};
  if (npass) std::stable_sort(ref.begin(), ref.end(), [](const E& a, const E& b) { return a.f < b.f; });
  const std::vector<K>& rk = hk[flip ? 1 : 0];
  const std::vector<uint32_t>& rv = hv[flip ? 1 : 0];
  for (uint64_t j = 0; j < n; ++j) {
    const K ek = keys[ref[j].i];
    if (rk[j] != ek || rv[j] != ref[j].i)
      return fmt("\"what\": \"result\", \"pos\": %llu, \"expected\": [%llu, %u], \"actual\": [%llu, %u]",
                 (unsigned long long)j, (unsigned long long)ek, ref[j].i, (unsigned long long)rk[j], rv[j]);
  }
  // the other buffer pair: untouched (no pass ran: the prefill), else the stable order on the
  // low npass - 1 digits (the input for one pass) -- a permutation of the input pairs in
  // ascending (stage field, input index) is that order and nothing else
  const std::vector<K>& ok = hk[flip ? 0 : 1];
  const std::vector<uint32_t>& ov = hv[flip ? 0 : 1];
  if (npass == 0) {
    K pf;
    memset(&pf, PREFILL, sizeof pf);
    uint32_t pv;
    memset(&pv, PREFILL, sizeof pv);
    for (uint64_t j = 0; j < n; ++j)
      if (ok[j] != pf || ov[j] != pv)
        return fmt("\"what\": \"unused buffer written\", \"pos\": %llu, \"expected\": [%llu, %u], \"actual\": [%llu, %u]",
                   (unsigned long long)j, (unsigned long long)pf, pv, (unsigned long long)ok[j], ov[j]);
    return "";
  }
  const uint64_t sm = field_mask(8 * (npass - 1)) & fm;
  std::vector<bool> seen(n, false);
  for (uint64_t j = 0; j < n; ++j) {
    const uint32_t v = ov[j];
    bool good = v < n && !seen[v] && ok[j] == keys[v];
    if (good && j) {
      const uint64_t a = ((uint64_t)ok[j - 1] >> lo) & sm, b = ((uint64_t)ok[j] >> lo) & sm;
      good = a < b || (a == b && ov[j - 1] < v);
    }
    if (!good)
      return fmt("\"what\": \"stage buffer is not the stable order of pass %d\", \"pos\": %llu, \"actual\": [%llu, %u]",
                 npass - 1, (unsigned long long)j, (unsigned long long)ok[j], v);
    seen[v] = true;
  }
  return "";
}

static void fill_scratch(Arena& scr, size_t bytes, int mode) {
  void* p = scr.set(bytes);
  CK(hipMemset(p, 0xFF, bytes));
  if (mode == 1) CK(hipMemset(p, 0, RS_HDR_BYTES));
}

template <typename K>
static int do_sort() {
  const double t0 = now_ms();
  const int kb = sizeof(K);
  SortBufs<K> B;
  B.init(RS_BIG_N + 1);
  int failed = 0, ncases = 0;
  std::vector<K> keys;
  for (const SortCase& c : sort_cases(kb)) {
    std::string err;
    uint64_t seed = c.n * 1315423911ull + c.lo * 131 + c.hi * 31 + c.dist * 7 + c.scratch;
    if (c.steps.empty()) {
      gen_keys<K>(keys, c.n, c.lo, c.hi, c.dist, (uint64_t)RS_THREADS * radix_items(c.n, kb), seed);
      fill_scratch(B.scr, radix_scratch_bytes(c.n), c.scratch);
      err = sort_once<K>(B, keys, c.lo, c.hi, c.scratch == 1);
    } else {  // as a context reuses its scratch: sized for the largest sort, never touched between
      fill_scratch(B.scr, radix_scratch_bytes(c.n), 0);
      for (size_t s = 0; s < c.steps.size() && err.empty(); ++s) {
        const uint64_t n = c.steps[s];
        gen_keys<K>(keys, n, c.lo, c.hi, c.dist, (uint64_t)RS_THREADS * radix_items(n, kb), seed + s);
        err = sort_once<K>(B, keys, c.lo, c.hi, false);
        if (!err.empty()) err += fmt(", \"step\": %zu, \"step_n\": %llu", s, (unsigned long long)n);
      }
    }
    ++ncases;
    failed += !err.empty();
    printf("{\"name\": \"%s\", \"n\": %llu, \"lo\": %d, \"hi\": %d, \"dist\": \"%s\", \"scratch\": \"%s\", \"ok\": %s%s%s}\n",
           sort_name(kb, c).c_str(), (unsigned long long)c.n, c.lo, c.hi, DISTS[c.dist], SCRATCH_MODES[c.scratch],
           err.empty() ? "true" : "false", err.empty() ? "" : ", ", err.c_str());
  }
  printf("{\"summary\": \"sort%d\", \"cases\": %d, \"failed\": %d, \"elapsed_ms\": %.0f, \"launches\": {", kb * 8, ncases,
         failed, now_ms() - t0);
  print_launches();
  printf("}}\n");
  return failed ? 1 : 0;
}

// ---------------------------------------------------------------------------
// scans
// ---------------------------------------------------------------------------
constexpr int OUT_FILL = 0xC3;
struct ScanBufs {
  Arena in, out, total, scr, ndev;
  void init(uint64_t max_n) {
    in.init("in", max_n * 8);
    out.init("out", max_n * 8);
    total.init("total", 8);
    scr.init("scratch", scan_scratch_bytes(max_n, 8));
    ndev.init("n_dev", 4);
  }
};

template <typename T>
static T poison() {
  return (T)0xDEADBEEFCAFEF00Dull;
}

template <typename T>
static void gen_scan_input(std::vector<T>& v, uint64_t n, int input, uint64_t seed) {
  Rng r(seed);
  v.resize(n);
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t x = r.next();
    if (input == 0) v[i] = 1;
    else if (input == 1) v[i] = (T)(x & 0xFFFFF);
    else v[i] = sizeof(T) == 4 ? (T)(0x70000000u + (x & 0x1FFFFFFF)) : (T)((1ull << 32) + (x & 0xFFFFFFFFFFull));
  }
}

// One scan_exclusive call.  count < 0: no n_dev; else the device count under the host bound n
// (the inputs past it are poison).  Returns "" or the mismatch.
template <typename T>
static std::string scan_once(ScanBufs& B, const std::vector<T>& in0, bool want_total, bool alias, bool small_ok,
                             long long count) {
  const uint64_t n = in0.size();
  const uint64_t cnt = count < 0 ? n : (uint64_t)count;
  std::vector<T> in = in0;
  for (uint64_t i = cnt; i < n; ++i) in[i] = poison<T>();
  T* d_in = (T*)B.in.set(n * sizeof(T));
  T* d_out = (T*)B.out.set(n * sizeof(T));
  T* d_tot = (T*)B.total.set(sizeof(T));
  uint32_t* d_nd = (uint32_t*)B.ndev.set(4);
  const size_t sb = scan_scratch_bytes(n, sizeof(T));
  void* d_scr = B.scr.set(sb);
  CK(hipMemset(d_scr, 0xFF, sb));
  if (n) {
    CK(hipMemcpy(d_in, in.data(), n * sizeof(T), hipMemcpyHostToDevice));
    CK(hipMemset(d_out, OUT_FILL, n * sizeof(T)));
  }
  CK(hipMemset(d_tot, OUT_FILL, sizeof(T)));
  const uint32_t c32 = (uint32_t)cnt;
  CK(hipMemcpy(d_nd, &c32, 4, hipMemcpyHostToDevice));
  scan_exclusive<T>(d_in, alias ? d_in : d_out, n, want_total ? d_tot : (T*)nullptr, d_scr, (hipStream_t)0, small_ok,
                    count < 0 ? (const uint32_t*)nullptr : d_nd);
  CK(hipDeviceSynchronize());
  std::vector<T> got(n), gin(n);
  T gtot;
  if (n) {
    CK(hipMemcpy(got.data(), alias ? d_in : d_out, n * sizeof(T), hipMemcpyDeviceToHost));
    CK(hipMemcpy(gin.data(), d_in, n * sizeof(T), hipMemcpyDeviceToHost));
  }
  CK(hipMemcpy(&gtot, d_tot, sizeof(T), hipMemcpyDeviceToHost));
  uint32_t gnd;
  CK(hipMemcpy(&gnd, d_nd, 4, hipMemcpyDeviceToHost));
  for (const Arena* a : {&B.in, &B.out, &B.total, &B.scr, &B.ndev})
    if (!a->check()) return fmt("\"what\": \"guard of %s overwritten\"", a->name);
  T fill;
  memset(&fill, OUT_FILL, sizeof fill);
  T run = 0;  // (wraps modulo 2^32 for uint32_t, as the device does)
  for (uint64_t i = 0; i < n; ++i) {
    const T want = i < cnt ? run : alias ? poison<T>() : fill;
    if (got[i] != want)
      return fmt("\"what\": \"%s\", \"pos\": %llu, \"expected\": %llu, \"actual\": %llu",
                 i < cnt ? "output" : "entry past the device count written", (unsigned long long)i,
                 (unsigned long long)want, (unsigned long long)got[i]);
    if (i < cnt) run += in[i];
  }
  if (!alias)
    for (uint64_t i = 0; i < n; ++i)
      if (gin[i] != in[i])
        return fmt("\"what\": \"input written\", \"pos\": %llu, \"expected\": %llu, \"actual\": %llu",
                   (unsigned long long)i, (unsigned long long)in[i], (unsigned long long)gin[i]);
  const T wtot = want_total ? run : fill;
  if (gtot != wtot)
    return fmt("\"what\": \"total\", \"expected\": %llu, \"actual\": %llu", (unsigned long long)wtot,
               (unsigned long long)gtot);
  if (gnd != c32) return fmt("\"what\": \"n_dev written\"");
  return "";
}

template <typename T>
static std::string scan_case(ScanBufs& B, const ScanCase& c, int* variants) {
  std::vector<T> in;
  gen_scan_input<T>(in, c.n, c.input, c.n * 2654435761ull + c.input + 16 * sizeof(T));
  // the device counts under the host bound n (none: no n_dev).  The large sizes take n - 1 only.
  std::vector<long long> counts = {-1};
  if (c.n > SCAN_SMALL_MAX + 1)
    counts.push_back((long long)c.n - 1);
  else
    for (long long k : {0ll, 1ll, (long long)(c.n / 2), (long long)c.n - 1, (long long)c.n})
      if (k >= 0 && k <= (long long)c.n) counts.push_back(k);
  for (long long cnt : counts)
    for (int tot = 1; tot >= 0; --tot)
      for (int alias = 0; alias < 2; ++alias) {
        ++*variants;
        std::string e = scan_once<T>(B, in, tot != 0, alias != 0, c.small_ok, cnt);
        if (!e.empty())
          return e + fmt(", \"variant\": {\"total\": %s, \"in_is_out\": %s, \"n_dev\": %lld}", tot ? "true" : "false",
                         alias ? "true" : "false", cnt);
      }
  return "";
}

// k_scan_small3: jobs a, b of uint32_t and c of uint64_t (as a commit launches it), `skip` null (-1: none)
static std::string small3_once(Arena* in3, Arena* out3, Arena* tot3, uint64_t n, int skip) {
  std::vector<uint32_t> a, b;
  std::vector<uint64_t> c;
  gen_scan_input<uint32_t>(a, n, 1, n + 1);
  gen_scan_input<uint32_t>(b, n, 2, n + 2);
  gen_scan_input<uint64_t>(c, n, 2, n + 3);
  const void* src[3] = {a.data(), b.data(), c.data()};
  const size_t eb[3] = {4, 4, 8};
  ScanJob job[3];
  for (int j = 0; j < 3; ++j) {
    void* di = in3[j].set(n * eb[j]);
    void* dout = out3[j].set(n * eb[j]);
    void* dt = tot3[j].set(eb[j]);
    CK(hipMemcpy(di, src[j], n * eb[j], hipMemcpyHostToDevice));
    CK(hipMemset(dout, OUT_FILL, n * eb[j]));
    CK(hipMemset(dt, OUT_FILL, eb[j]));
    job[j] = ScanJob{j == skip ? nullptr : di, dout, dt, eb[j] == 8};
  }
  hipLaunchKernelGGL(k_scan_small3, dim3(3), dim3(SCAN_SMALL_THREADS), 0, (hipStream_t)0, job[0], job[1], job[2], n);
  CK(hipDeviceSynchronize());
  for (int j = 0; j < 3; ++j) {
    std::vector<uint64_t> got(n);
    uint64_t gt = 0;
    if (eb[j] == 4) {
      std::vector<uint32_t> g4(n);
      uint32_t t4;
      CK(hipMemcpy(g4.data(), out3[j].ptr(), n * 4, hipMemcpyDeviceToHost));
      CK(hipMemcpy(&t4, tot3[j].ptr(), 4, hipMemcpyDeviceToHost));
      for (uint64_t i = 0; i < n; ++i) got[i] = g4[i];
      gt = t4;
    } else {
      CK(hipMemcpy(got.data(), out3[j].ptr(), n * 8, hipMemcpyDeviceToHost));
      CK(hipMemcpy(&gt, tot3[j].ptr(), 8, hipMemcpyDeviceToHost));
    }
    if (!in3[j].check() || !out3[j].check() || !tot3[j].check()) return fmt("\"what\": \"guard overwritten\", \"job\": %d", j);
    const uint64_t m = eb[j] == 4 ? 0xFFFFFFFFull : ~0ull;
    uint64_t fill;
    memset(&fill, OUT_FILL, 8);
    fill &= m;
    uint64_t run = 0;
    for (uint64_t i = 0; i < n; ++i) {
      const uint64_t want = j == skip ? fill : run;
      if (got[i] != want)
        return fmt("\"what\": \"output\", \"job\": %d, \"pos\": %llu, \"expected\": %llu, \"actual\": %llu", j,
                   (unsigned long long)i, (unsigned long long)want, (unsigned long long)got[i]);
      run = (run + (j == 0 ? a[i] : j == 1 ? b[i] : c[i])) & m;
    }
    const uint64_t wt = j == skip ? fill : run;
    if (gt != wt)
      return fmt("\"what\": \"total\", \"job\": %d, \"expected\": %llu, \"actual\": %llu", j, (unsigned long long)wt,
                 (unsigned long long)gt);
  }
  return "";
}

static int do_scan() {
  const double t0 = now_ms();
  ScanBufs B;
  B.init(SCAN_TWO_MAX + 1);
  int failed = 0, ncases = 0;
  for (const ScanCase& c : scan_cases()) {
    int variants = 0;
    std::string err = c.elem_bytes == 4 ? scan_case<uint32_t>(B, c, &variants) : scan_case<uint64_t>(B, c, &variants);
    ++ncases;
    failed += !err.empty();
    printf("{\"name\": \"%s\", \"n\": %llu, \"elem_bytes\": %d, \"input\": \"%s\", \"small_ok\": %s, \"variants\": %d, "
           "\"ok\": %s%s%s}\n",
           scan_name(c).c_str(), (unsigned long long)c.n, c.elem_bytes, SCAN_INPUTS[c.input],
           c.small_ok ? "true" : "false", variants, err.empty() ? "true" : "false", err.empty() ? "" : ", ",
           err.c_str());
  }
  Arena in3[3], out3[3], tot3[3];
  for (int j = 0; j < 3; ++j) {
    in3[j].init("in3", SCAN_SMALL_MAX * 8);
    out3[j].init("out3", SCAN_SMALL_MAX * 8);
    tot3[j].init("total3", 8);
  }
  for (uint64_t n : small3_sizes()) {
    std::string err;
    int variants = 0;
    for (int skip = -1; skip < 3 && err.empty(); ++skip) {
      ++variants;
      err = small3_once(in3, out3, tot3, n, skip);
      if (!err.empty()) err += fmt(", \"null_job\": %d", skip);
    }
    ++ncases;
    failed += !err.empty();
    printf("{\"name\": \"scan_small3/n%llu\", \"n\": %llu, \"variants\": %d, \"ok\": %s%s%s}\n", (unsigned long long)n,
           (unsigned long long)n, variants, err.empty() ? "true" : "false", err.empty() ? "" : ", ", err.c_str());
  }
  printf("{\"summary\": \"scan\", \"cases\": %d, \"failed\": %d, \"elapsed_ms\": %.0f, \"launches\": {", ncases, failed,
         now_ms() - t0);
  print_launches();
  printf("}}\n");
  return failed ? 1 : 0;
}

// ---------------------------------------------------------------------------
// wave helpers: one block of four waves
// ---------------------------------------------------------------------------
constexpr int WT = RS_THREADS;  // 256 threads

__global__ void __launch_bounds__(WT) k_w_reduce(const uint32_t* in32, const uint64_t* in64, uint32_t* omax,
                                                 uint32_t* osum32, uint64_t* osum64) {
  const int t = threadIdx.x;
  omax[t] = wave_max_u32(in32[t]);
  osum32[t] = wave_sum<uint32_t>(in32[t]);
  osum64[t] = wave_sum<uint64_t>(in64[t]);
}
// divergent: only the odd lanes call (they aggregate among themselves)
__global__ void __launch_bounds__(WT) k_w_claim(unsigned long long* ctr, const uint8_t* want, uint64_t* slot,
                                                int divergent) {
  const int t = threadIdx.x;
  uint64_t s = ~0ull;
  if (!divergent)
    s = wave_claim(ctr, want[t] != 0);
  else if (t & 1)
    s = wave_claim(ctr, want[t] != 0);
  slot[t] = s;
}
__global__ void __launch_bounds__(WT) k_w_atomic(unsigned long long* dst, const uint64_t* v) {
  wave_atomic_add(dst, v[threadIdx.x]);
}
// two scans in a row over one lds_waves array, as k_rs_pass runs them
__global__ void __launch_bounds__(WT) k_w_bscan(const uint32_t* a, const uint32_t* b, uint32_t* oa, uint32_t* ob,
                                                uint32_t* tots) {
  __shared__ uint32_t lw[SCAN_THREADS / 64];
  const int t = threadIdx.x;
  uint32_t ta, tb;
  oa[t] = block_exclusive_scan<uint32_t>(a[t], lw, &ta);
  ob[t] = block_exclusive_scan<uint32_t>(b[t], lw, &tb);
  tots[2 * t] = ta;
  tots[2 * t + 1] = tb;
}

struct WaveBufs {
  Arena a32, b32, a64, o32a, o32b, o64, o512, ctr, want;
  void init() {
    a32.init("a32", WT * 4);
    b32.init("b32", WT * 4);
    a64.init("a64", WT * 8);
    o32a.init("o32a", WT * 4);
    o32b.init("o32b", WT * 4);
    o64.init("o64", WT * 8);
    o512.init("o512", 2 * WT * 4);
    ctr.init("ctr", 8);
    want.init("want", WT);
    a32.set(WT * 4), b32.set(WT * 4), a64.set(WT * 8), o32a.set(WT * 4), o32b.set(WT * 4), o64.set(WT * 8);
    o512.set(2 * WT * 4), ctr.set(8), want.set(WT);
  }
  std::string guards() {
    for (const Arena* a : {&a32, &b32, &a64, &o32a, &o32b, &o64, &o512, &ctr, &want})
      if (!a->check()) return fmt("\"what\": \"guard of %s overwritten\"", a->name);
    return "";
  }
};

// the maximum (a value no sum of the others reaches) in lane `pos` of every wave
static std::string wave_reduce_case(WaveBufs& B, int which, int pos) {
  Rng r(pos + 100 * which);
  uint32_t a[WT];
  uint64_t b[WT];
  for (int t = 0; t < WT; ++t) {
    a[t] = (uint32_t)(r.next() % 1000);
    b[t] = (1ull << 33) + (r.next() & 0xFFFFFFFFFFull);
    if ((t & 63) == pos) {
      a[t] = 0xF0000000u + (uint32_t)(t >> 6);
      b[t] = (1ull << 60) + (uint64_t)(t >> 6);
    }
  }
  CK(hipMemcpy(B.a32.ptr(), a, sizeof a, hipMemcpyHostToDevice));
  CK(hipMemcpy(B.a64.ptr(), b, sizeof b, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_w_reduce, dim3(1), dim3(WT), 0, (hipStream_t)0, (const uint32_t*)B.a32.ptr(),
                     (const uint64_t*)B.a64.ptr(), (uint32_t*)B.o32a.ptr(), (uint32_t*)B.o32b.ptr(),
                     (uint64_t*)B.o64.ptr());
  CK(hipDeviceSynchronize());
  uint32_t omax[WT], os32[WT];
  uint64_t os64[WT];
  CK(hipMemcpy(omax, B.o32a.ptr(), sizeof omax, hipMemcpyDeviceToHost));
  CK(hipMemcpy(os32, B.o32b.ptr(), sizeof os32, hipMemcpyDeviceToHost));
  CK(hipMemcpy(os64, B.o64.ptr(), sizeof os64, hipMemcpyDeviceToHost));
  for (int t = 0; t < WT; ++t) {
    const int w0 = t & ~63;
    uint32_t m = 0, s32 = 0;
    uint64_t s64 = 0;
    for (int l = 0; l < 64; ++l) {
      m = std::max(m, a[w0 + l]);
      s32 += a[w0 + l];
      s64 += b[w0 + l];
    }
    const uint64_t want = which == 0 ? m : which == 1 ? s32 : s64;
    const uint64_t got = which == 0 ? omax[t] : which == 1 ? os32[t] : os64[t];
    if (got != want)
      return fmt("\"what\": \"lane result\", \"max_lane\": %d, \"pos\": %d, \"expected\": %llu, \"actual\": %llu", pos, t,
                 (unsigned long long)want, (unsigned long long)got);
  }
  return B.guards();
}

static std::string wave_claim_case(WaveBufs& B, int pattern, int divergent) {
  uint8_t want[WT];
  for (int t = 0; t < WT; ++t) {
    const int lane = t & 63, w = t >> 6;
    switch (pattern) {
      case 0: want[t] = 1; break;
      case 1: want[t] = 0; break;
      case 2: want[t] = (w == 0 && lane == 17) || (w == 1 && lane == 0) || (w == 2 && lane == 63); break;  // wave 3: none
      case 3: want[t] = lane & 1; break;
      default: want[t] = t % 3 == 0; break;
    }
  }
  const unsigned long long start = 0xFFFFFFF0ull;  // the claims cross 2^32: both halves of the base are passed on
  CK(hipMemcpy(B.want.ptr(), want, sizeof want, hipMemcpyHostToDevice));
  CK(hipMemcpy(B.ctr.ptr(), &start, 8, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_w_claim, dim3(1), dim3(WT), 0, (hipStream_t)0, (unsigned long long*)B.ctr.ptr(),
                     (const uint8_t*)B.want.ptr(), (uint64_t*)B.o64.ptr(), divergent);
  CK(hipDeviceSynchronize());
  uint64_t slot[WT];
  unsigned long long ctr;
  CK(hipMemcpy(slot, B.o64.ptr(), sizeof slot, hipMemcpyDeviceToHost));
  CK(hipMemcpy(&ctr, B.ctr.ptr(), 8, hipMemcpyDeviceToHost));
  // per wave consecutive in lane order; over the waves the ranges tile [start, start + claims)
  std::vector<std::pair<uint64_t, uint64_t>> ranges;
  uint64_t claims = 0;
  for (int w = 0; w < WT / 64; ++w) {
    uint64_t base = 0, cnt = 0;
    for (int l = 0; l < 64; ++l) {
      const int t = 64 * w + l;
      if (!want[t] || (divergent && !(t & 1))) continue;
      if (cnt == 0) base = slot[t];
      if (slot[t] != base + cnt)
        return fmt("\"what\": \"slot\", \"pos\": %d, \"expected\": %llu, \"actual\": %llu", t,
                   (unsigned long long)(base + cnt), (unsigned long long)slot[t]);
      ++cnt;
    }
    if (cnt) ranges.push_back({base, cnt});
    claims += cnt;
  }
  std::sort(ranges.begin(), ranges.end());
  uint64_t at = start;
  for (auto& rg : ranges) {
    if (rg.first != at)
      return fmt("\"what\": \"wave ranges not distinct and consecutive\", \"expected\": %llu, \"actual\": %llu",
                 (unsigned long long)at, (unsigned long long)rg.first);
    at += rg.second;
  }
  if (ctr != start + claims)
    return fmt("\"what\": \"counter\", \"expected\": %llu, \"actual\": %llu", (unsigned long long)(start + claims), ctr);
  return B.guards();
}

static std::string wave_atomic_case(WaveBufs& B, bool zero) {
  Rng r(77);
  uint64_t v[WT];
  const unsigned long long start = 0x123456789ull;
  unsigned long long want = start;
  for (int t = 0; t < WT; ++t) {
    v[t] = zero ? 0 : (t % 5 == 0 ? 0 : (1ull << 32) + (r.next() & 0xFFFFFFFFull));
    want += v[t];
  }
  CK(hipMemcpy(B.a64.ptr(), v, sizeof v, hipMemcpyHostToDevice));
  CK(hipMemcpy(B.ctr.ptr(), &start, 8, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_w_atomic, dim3(1), dim3(WT), 0, (hipStream_t)0, (unsigned long long*)B.ctr.ptr(),
                     (const uint64_t*)B.a64.ptr());
  CK(hipDeviceSynchronize());
  unsigned long long got;
  CK(hipMemcpy(&got, B.ctr.ptr(), 8, hipMemcpyDeviceToHost));
  if (got != want) return fmt("\"what\": \"sum\", \"expected\": %llu, \"actual\": %llu", want, got);
  return B.guards();
}

static std::string wave_bscan_case(WaveBufs& B) {
  Rng r(91);
  uint32_t a[WT], b[WT];
  for (int t = 0; t < WT; ++t) {
    a[t] = (uint32_t)(r.next() % 17);           // a tile's digit counts
    b[t] = (uint32_t)(r.next() & 0x3FFFFFFF);   // sums that wrap
  }
  CK(hipMemcpy(B.a32.ptr(), a, sizeof a, hipMemcpyHostToDevice));
  CK(hipMemcpy(B.b32.ptr(), b, sizeof b, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_w_bscan, dim3(1), dim3(WT), 0, (hipStream_t)0, (const uint32_t*)B.a32.ptr(),
                     (const uint32_t*)B.b32.ptr(), (uint32_t*)B.o32a.ptr(), (uint32_t*)B.o32b.ptr(),
                     (uint32_t*)B.o512.ptr());
  CK(hipDeviceSynchronize());
  uint32_t oa[WT], ob[WT], tots[2 * WT];
  CK(hipMemcpy(oa, B.o32a.ptr(), sizeof oa, hipMemcpyDeviceToHost));
  CK(hipMemcpy(ob, B.o32b.ptr(), sizeof ob, hipMemcpyDeviceToHost));
  CK(hipMemcpy(tots, B.o512.ptr(), sizeof tots, hipMemcpyDeviceToHost));
  uint32_t ta = 0, tb = 0;
  for (int t = 0; t < WT; ++t) ta += a[t], tb += b[t];
  uint32_t ra = 0, rb = 0;
  for (int t = 0; t < WT; ++t) {
    if (oa[t] != ra || ob[t] != rb)
      return fmt("\"what\": \"prefix\", \"pos\": %d, \"expected\": [%u, %u], \"actual\": [%u, %u]", t, ra, rb, oa[t], ob[t]);
    if (tots[2 * t] != ta || tots[2 * t + 1] != tb)
      return fmt("\"what\": \"total\", \"pos\": %d, \"expected\": [%u, %u], \"actual\": [%u, %u]", t, ta, tb, tots[2 * t],
                 tots[2 * t + 1]);
    ra += a[t];
    rb += b[t];
  }
  return B.guards();
}

static int do_wave() {
  const double t0 = now_ms();
  WaveBufs B;
  B.init();
  int failed = 0, ncases = 0;
  const size_t nw = sizeof WAVE_CASES / sizeof *WAVE_CASES;
  for (size_t i = 0; i < nw; ++i) {
    std::string err;
    if (i < 3) {
      for (int pos : MAX_LANES)
        if (err.empty()) err = wave_reduce_case(B, (int)i, pos);
    } else if (i < 9) {
      const int pat[] = {0, 1, 2, 3, 0, 4};
      err = wave_claim_case(B, pat[i - 3], i >= 7);
    } else if (i < 11) {
      err = wave_atomic_case(B, i == 10);
    } else {
      err = wave_bscan_case(B);
    }
    ++ncases;
    failed += !err.empty();
    printf("{\"name\": \"%s\", \"n\": %d, \"ok\": %s%s%s}\n", WAVE_CASES[i], WT, err.empty() ? "true" : "false",
           err.empty() ? "" : ", ", err.c_str());
  }
  printf("{\"summary\": \"wave\", \"cases\": %d, \"failed\": %d, \"elapsed_ms\": %.0f, \"launches\": {", ncases, failed,
         now_ms() - t0);
  print_launches();
  printf("}}\n");
  return failed ? 1 : 0;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "plan") return do_plan();
  if (mode == "sort32") return do_sort<uint32_t>();
  if (mode == "sort64") return do_sort<uint64_t>();
  if (mode == "scan") return do_scan();
  if (mode == "wave") return do_wave();
  fprintf(stderr, "usage: prims_check plan | sort32 | sort64 | scan | wave\n");
  return 2;
}
