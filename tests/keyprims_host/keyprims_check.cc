// The anchor key primitives of khipu_amd/csrc/forest.h on the host, stand-alone: built by
// tests/test_keyprims_host.py (once plain, once with -fsanitize=address,undefined) and run as a
// child process.
//
//   keyprims_check < FILE
// FILE, one record a line (keys as 64 hex digits):
//   K t keyhex        for every d in 0..64:  K idx d w0 w1 w2 w3 tag
//                     (w0..w3: prefix_word(key, d, q) as the word's 8 bytes in memory order;
//                      tag: anchor_tag(t, d, key), 16 hex digits)
//   P ahex bhex       P idx e0e1...e64      (e_d: prefix_eq(a, b, d) as 0 / 1)
//   S keyhex          for every i in 0..63 and v in 0..15:  S idx i v keyhex  (the key after set_nibble)
// idx counts the records of each kind from 0.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "../../khipu_amd/csrc/forest.h"

using namespace khst;

static bool key_of(const std::string& s, uint64_t k[4]) {
  if (s.size() != 64) return false;
  uint8_t b[32];
  for (int i = 0; i < 32; ++i) b[i] = (uint8_t)strtoul(s.substr(2 * i, 2).c_str(), nullptr, 16);
  memcpy(k, b, 32);
  return true;
}
static void put_bytes(const void* p, size_t n) {
  const uint8_t* b = (const uint8_t*)p;
  for (size_t i = 0; i < n; ++i) printf("%02x", b[i]);
}

int main() {
  std::string line;
  long nk = 0, np = 0, ns = 0;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string kind, a, b;
    in >> kind;
    if (kind == "K") {
      unsigned long t;
      uint64_t k[4];
      in >> t >> a;
      if (!key_of(a, k)) return 2;
      for (uint32_t d = 0; d <= 64; ++d) {
        printf("K %ld %u", nk, d);
        for (int q = 0; q < 4; ++q) {
          const uint64_t w = prefix_word(k, d, q);
          printf(" ");
          put_bytes(&w, 8);
        }
        printf(" %016llx\n", (unsigned long long)anchor_tag((uint32_t)t, d, k));
      }
      ++nk;
    } else if (kind == "P") {
      uint64_t x[4], y[4];
      in >> a >> b;
      if (!key_of(a, x) || !key_of(b, y)) return 2;
      printf("P %ld ", np++);
      for (uint32_t d = 0; d <= 64; ++d) printf("%d", prefix_eq(x, y, d) ? 1 : 0);
      printf("\n");
    } else if (kind == "S") {
      uint64_t k0[4];
      in >> a;
      if (!key_of(a, k0)) return 2;
      for (uint32_t i = 0; i < 64; ++i)
        for (uint32_t v = 0; v < 16; ++v) {
          uint64_t k[4] = {k0[0], k0[1], k0[2], k0[3]};
          set_nibble(k, i, v);
          printf("S %ld %u %u ", ns, i, v);
          put_bytes(k, 32);
          printf("\n");
        }
      ++ns;
    } else if (!kind.empty()) {
      return 2;
    }
  }
  return 0;
}
