// Host check of keccak.h's digest forms (tests/test_keccak_digest.py): a stand-alone program.
//
//   P <count> <seed>   -> "P <mismatches>": keccakf_digest's lanes 0..3 against the full keccakf's
//                         on <count> random states, at every loop shape the header builds
//   M <hex | ->        -> "M <len> <form> <digest hex>" per form that takes the length, the message
//                         placed at each of the 8 byte alignments (one line per form: every
//                         alignment must agree, else the form prints "MISALIGNED")
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <iostream>
#include <string>
#include <vector>

#include "../../khipu_amd/csrc/keccak.h"

using namespace khst;

static uint64_t rng_state;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ULL);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}

template <int U>
static bool digest_matches(const KState& in) {
  KState full = in, dig = in;
  keccakf(full);
  keccakf_digest<U>(dig);
  for (int i = 0; i < 4; ++i)
    if (lane(full, i) != lane(dig, i)) return false;
  return true;
}

static std::string hex32(const uint64_t h[4]) {
  char buf[65];
  for (int i = 0; i < 32; ++i) snprintf(buf + 2 * i, 3, "%02x", (unsigned)((h[i / 8] >> (8 * (i % 8))) & 0xFF));
  return buf;
}

// f(p, out) at every alignment of the message inside an 8-byte-aligned buffer that ends with the
// message's last aligned word (the forms read aligned words that hold message bytes, nothing else)
template <typename F>
static void run_form(const char* name, const std::vector<uint8_t>& msg, F f) {
  std::string first;
  bool same = true;
  for (size_t a = 0; a < 8; ++a) {
    std::vector<uint64_t> buf((a + msg.size() + 7) / 8 + (msg.empty() ? 1 : 0), 0xA5A5A5A5A5A5A5A5ULL);
    uint8_t* p = (uint8_t*)buf.data() + a;
    if (!msg.empty()) memcpy(p, msg.data(), msg.size());
    uint64_t h[4];
    f(p, h);
    const std::string s = hex32(h);
    if (a == 0)
      first = s;
    else
      same = same && s == first;
  }
  printf("M %zu %s %s\n", msg.size(), name, same ? first.c_str() : "MISALIGNED");
}

int main() {
  std::string cmd;
  while (std::cin >> cmd) {
    if (cmd == "P") {
      uint64_t count, seed, bad = 0;
      std::cin >> count >> seed;
      rng_state = seed;
      for (uint64_t k = 0; k < count; ++k) {
        KState s;
        for (int i = 0; i < 25; ++i) {
          const uint64_t w = k == 0 ? 0 : rnd();  // (the all-zero state first)
          s.lo[i] = (uint32_t)w;
          s.hi[i] = (uint32_t)(w >> 32);
        }
        bad += !(digest_matches<22>(s) && digest_matches<11>(s) && digest_matches<2>(s) && digest_matches<1>(s));
      }
      printf("P %llu\n", (unsigned long long)bad);
    } else if (cmd == "M") {
      std::string hx;
      std::cin >> hx;
      std::vector<uint8_t> msg;
      if (hx != "-")
        for (size_t i = 0; i + 1 < hx.size(); i += 2) msg.push_back((uint8_t)std::stoul(hx.substr(i, 2), nullptr, 16));
      const uint32_t len = (uint32_t)msg.size();
      run_form("msg", msg, [&](const uint8_t* p, uint64_t* h) { kec256_msg<false>(p, len, h); });
      run_form("msg_digest", msg, [&](const uint8_t* p, uint64_t* h) { kec256_msg_digest<false>(p, len, h); });
      if (len <= 135) {
        run_form("short", msg, [&](const uint8_t* p, uint64_t* h) { kec256_short(p, len, h); });
        run_form("short_digest", msg, [&](const uint8_t* p, uint64_t* h) { kec256_short_digest(p, len, h); });
      }
      if (len == 20) run_form("fixed", msg, [&](const uint8_t* p, uint64_t* h) { kec256_fixed<20>(p, h); });
      if (len == 32) run_form("fixed", msg, [&](const uint8_t* p, uint64_t* h) { kec256_fixed<32>(p, h); });
      if (len == 19) run_form("fixed", msg, [&](const uint8_t* p, uint64_t* h) { kec256_fixed<19>(p, h); });
      if (len == 135) run_form("fixed", msg, [&](const uint8_t* p, uint64_t* h) { kec256_fixed<135>(p, h); });
    } else {
      fprintf(stderr, "unknown command %s\n", cmd.c_str());
      return 2;
    }
  }
  return 0;
}
