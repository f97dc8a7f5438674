// Host replay of the record -> node encoder (khipu_amd/csrc/export.h), stand-alone: built with
// g++ -fsanitize=address,undefined by tests/test_export_host.py and run as a child process.
//
//   export_check FILE [flip]
// FILE: one "keyhex valuehex" line per put (32-byte keys; "-" = the empty value).  The program
// builds the canonical records of that trie bottom-up -- each node's encoding made by export.h's
// own write bodies and hashed by keccak.h's host path to fill ref / bref -- inserts the anchors
// (anchor_tag, linear probing), then runs the sizes and write bodies over all records the way
// the kernels do (16 lanes a record, replayed by loops; a prefix sum between the passes) into
// buffers of exactly the scanned size, verifies every node, and prints "hash enc" lines and a
// last line "verify_bad N".  With `flip`, one byte of one record's ref is flipped before the run.
#include "../host_common/replay.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const bool flip = argc > 2 && !strcmp(argv[2], "flip");
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  std::vector<Put> in;
  char kb[128], vb[8192];
  while (fscanf(f, "%127s %8191s", kb, vb) == 2) {
    const Bytes k = unhex(kb);
    if (k.size() != 32) return 2;
    Put p;
    memcpy(p.k.data(), k.data(), 32);
    p.v = unhex(vb);
    in.push_back(p);
  }
  fclose(f);
  Builder H(in);
  if (flip) {
    for (uint64_t r = 0; r < H.rn; ++r)
      if (H.R.rrl[r] == 32) {
        ((uint8_t*)&H.R.rref[4 * r])[7] ^= 0x10;
        break;
      }
  }
  // pass 1: sizes of every record (the kernels' selection), then the scans
  const uint64_t n = H.rn;
  std::vector<uint32_t> cnt(n + 1, 0), byt(n + 1, 0);
  uint32_t len[2];
  for (uint64_t r = 0; r < n; ++r) {
    const uint32_t sel = exp_select(H.R, r, EXP_ALL_TRIES);
    if (sel) H.encode(r, sel, len, &byt[r], &cnt[r]);
  }
  uint64_t tn = 0, tb = 0;
  std::vector<uint64_t> cpos(n), bpos(n);
  for (uint64_t r = 0; r < n; ++r) {
    cpos[r] = tn;
    bpos[r] = tb;
    tn += cnt[r];
    tb += byt[r];
  }
  // pass 2: write into buffers of exactly that size (the encodings padded to a whole word)
  std::vector<uint8_t> hashes(tn * 32);
  std::vector<uint64_t> off(tn + 1), rlpw((tb + 7) / 8 + 1, 0);
  uint8_t* rlp = (uint8_t*)rlpw.data();
  for (uint64_t r = 0; r < n; ++r) {
    const uint32_t sel = exp_select(H.R, r, EXP_ALL_TRIES);
    if (!sel) continue;
    const Bytes e = H.encode(r, sel, len);
    if (bpos[r] + e.size() > tb) return 5;
    memcpy(rlp + bpos[r], e.data(), e.size());
    uint64_t slot = cpos[r], at = bpos[r];
    for (uint32_t w = 0; w < 2; ++w) {
      if (!len[w]) continue;
      memcpy(&hashes[32 * slot], exp_hash_of(H.R, r, w ? EXP_LOWER : EXP_UPPER), 32);
      off[slot++] = at;
      at += len[w];
    }
  }
  off[tn] = tb;
  uint64_t bad = 0;
  for (uint64_t j = 0; j < tn; ++j) {
    bad += exp_verify(hashes.data(), rlp, off.data(), j) ? 1 : 0;
    put_hex(&hashes[32 * j], 32, "");
    printf(" ");
    put_hex(rlp + off[j], off[j + 1] - off[j], "");
    printf("\n");
  }
  printf("verify_bad %llu\n", (unsigned long long)bad);
  return 0;
}
