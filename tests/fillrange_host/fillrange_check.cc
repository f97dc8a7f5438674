// Host replay of the range fill's span test (khipu_amd/csrc/fillrange.h) and of the order check it
// shares with range verification (rangeverify.h), stand-alone: built with
// g++ -fsanitize=address,undefined by tests/test_fillrange_host.py and run as a child process.
//
//   fillrange_check FILE
// FILE, one record a line:
//   S prefixhex md lohex hihex      a stub: its 32-byte key prefix (zero past nibble md) and a span
//   R originhex m key_1 val_1 .. key_m val_m      a range (val "-": empty)
// Answers, in input order:
//   I inside endhex      fill_inside, and the upper end of the stub's own span (fill_span_end)
//   O bad                1 iff any entry of the range breaks the order contract (k_rv_order's flag)
// Every array has exactly the size the replayed code may touch.
#include "../host_common/replay.h"

#include "../../khipu_amd/csrc/fillrange.h"
#include "../../khipu_amd/csrc/rangeverify.h"

static uint64_t* words32(const Bytes& b) {
  if (b.size() != 32) exit(2);
  uint64_t* w = new uint64_t[4];
  memcpy(w, b.data(), 32);
  return w;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream f(argv[1]);
  if (!f) return 2;
  std::string line;
  while (std::getline(f, line)) {
    std::istringstream ss(line);
    std::string tag, a, b, c;
    ss >> tag;
    if (tag == "S") {
      uint32_t md = 0;
      ss >> a >> md >> b >> c;
      uint64_t *k = words32(unhex(a)), *lo = words32(unhex(b)), *hi = words32(unhex(c));
      uint64_t* end = new uint64_t[4];
      if (md > 64) return 2;
      fill_span_end(k, md, end);
      printf("I %d ", fill_inside(k, md, lo, hi) ? 1 : 0);
      put_hex((const uint8_t*)end, 32);
      printf("\n");
      delete[] k;
      delete[] lo;
      delete[] hi;
      delete[] end;
    } else if (tag == "R") {
      size_t m = 0;
      ss >> a >> m;
      uint64_t* origin = words32(unhex(a));
      uint64_t* keys = new uint64_t[4 * m];
      uint64_t* voff = new uint64_t[m + 1];
      uint64_t ent_off[2] = {0, m};
      uint64_t vb = 0;
      for (size_t i = 0; i < m; ++i) {
        ss >> b >> c;
        const Bytes k = unhex(b);
        if (k.size() != 32) return 2;
        memcpy(keys + 4 * i, k.data(), 32);
        voff[i] = vb;
        vb += unhex(c).size();
      }
      voff[m] = vb;
      const RvIn I{nullptr, origin, nullptr, 1, keys, voff, ent_off, NStore{}};
      bool bad = false;
      for (size_t i = 0; i < m; ++i) {  // one thread an entry (k_rv_order)
        if (rv_range_of(ent_off, 1, i) != 0) return 3;
        bad = rv_order_bad(I, 0, i) || bad;
      }
      printf("O %d\n", bad ? 1 : 0);
      delete[] origin;
      delete[] keys;
      delete[] voff;
    }
  }
  return 0;
}
