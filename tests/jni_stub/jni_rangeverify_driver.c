/* TEST INFRASTRUCTURE ONLY: jni/khst_jni.c's verifyRanges through the in-process JNIEnv of
 * fake_env.c (tests/test_gpu_rangeverify.py compiles and runs it).
 *
 *   jni_rangeverify_driver FILE   FILE: u64 nr, ne, vb, nn, nb; roots[32 nr], origins[32 nr],
 *                                 proved[nr], keys[32 ne], vals[vb], u64 voff[ne + 1],
 *                                 u64 ent_off[nr + 1], enc[nb], u64 off[nn + 1].
 * One verifyRanges call over all nr ranges:
 *   "R s status more missing" per range, "N bad" the call's return, "E pending exc";
 * then calls without ranges, "X case pending exc": entOff null (0) or empty (1), voff null (2) or
 * empty (3) -- each an IllegalArgumentException -- and one-offset arrays (4): no exception. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fake_env.h"
#include "khst.h"

jlong Java_khipu_trie_gpu_Khst_verifyRanges(JNIEnv*, jclass, jbyteArray, jbyteArray, jbyteArray, jbyteArray, jbyteArray,
                                            jlongArray, jlongArray, jbyteArray, jlongArray, jint, jbyteArray, jbyteArray,
                                            jbyteArray);

static void* slurp(FILE* f, size_t esz, uint64_t n) {
  void* p = malloc(esz * n + 1);
  if (!p || fread(p, esz, n, f) != n) exit(2);
  return p;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint64_t hd[5];
  if (fread(hd, 8, 5, f) != 5) return 2;
  const uint64_t nr = hd[0], ne = hd[1], vb = hd[2], nn = hd[3], nb = hd[4];
  uint8_t* roots = slurp(f, 32, nr);
  uint8_t* origins = slurp(f, 32, nr);
  uint8_t* proved = slurp(f, 1, nr);
  uint8_t* keys = slurp(f, 32, ne);
  uint8_t* vals = slurp(f, 1, vb);
  uint64_t* voff = slurp(f, 8, ne + 1);
  uint64_t* eoff = slurp(f, 8, nr + 1);
  uint8_t* enc = slurp(f, 1, nb);
  uint64_t* off = slurp(f, 8, nn + 1);
  fclose(f);
  JNIEnv* env = fake_env();
  FakeObj* status = fake_array((jsize)nr, 1, NULL);
  FakeObj* more = fake_array((jsize)nr, 1, NULL);
  FakeObj* missing = fake_array((jsize)(32 * nr), 1, NULL);
  const jlong bad = Java_khipu_trie_gpu_Khst_verifyRanges(
      env, NULL, (jbyteArray)fake_array((jsize)(32 * nr), 1, roots), (jbyteArray)fake_array((jsize)(32 * nr), 1, origins),
      (jbyteArray)fake_array((jsize)nr, 1, proved), (jbyteArray)fake_array((jsize)(32 * ne), 1, keys),
      (jbyteArray)fake_array((jsize)vb, 1, vals), (jlongArray)fake_array((jsize)(ne + 1), 8, voff),
      (jlongArray)fake_array((jsize)(nr + 1), 8, eoff), (jbyteArray)fake_array((jsize)nb, 1, enc),
      (jlongArray)fake_array((jsize)(nn + 1), 8, off), (jint)nn, (jbyteArray)status, (jbyteArray)more,
      (jbyteArray)missing);
  if (!fake.pending) {
    const uint8_t* st = (const uint8_t*)status->data;
    const uint8_t* mo = (const uint8_t*)more->data;
    const uint8_t* ms = (const uint8_t*)missing->data;
    for (uint64_t s = 0; s < nr; ++s) {
      printf("R %llu %u %u ", (unsigned long long)s, st[s], mo[s]);
      for (int i = 0; i < 32; ++i) printf("%02x", ms[32 * s + i]);
      printf("\n");
    }
    printf("N %lld\n", (long long)bad);
  }
  printf("E %d %s\n", fake.pending, fake.exc_class);
  /* offset arrays that are null or empty: an exception, nothing read ("X case pending class") */
  for (int c = 0; c < 4 && !fake.pending; ++c) {
    FakeObj* eo = c == 0 ? NULL : fake_array(c == 1 ? 0 : 1, 8, NULL); /* (one zero offset: no range) */
    FakeObj* vo = c == 2 ? NULL : fake_array(c == 3 ? 0 : 1, 8, NULL);
    Java_khipu_trie_gpu_Khst_verifyRanges(env, NULL, (jbyteArray)fake_array(0, 1, NULL), NULL,
                                          (jbyteArray)fake_array(0, 1, NULL), (jbyteArray)fake_array(0, 1, NULL),
                                          (jbyteArray)fake_array(0, 1, NULL), (jlongArray)vo, (jlongArray)eo,
                                          (jbyteArray)fake_array(0, 1, NULL), (jlongArray)fake_array(1, 8, NULL), 0,
                                          (jbyteArray)fake_array(0, 1, NULL), (jbyteArray)fake_array(0, 1, NULL), NULL);
    printf("X %d %d %s\n", c, fake.pending, fake.exc_class);
    fake.pending = 0;
    fake.exc_class[0] = 0;
  }
  /* zero ranges with well-formed offset arrays: no exception */
  Java_khipu_trie_gpu_Khst_verifyRanges(env, NULL, (jbyteArray)fake_array(0, 1, NULL), NULL,
                                        (jbyteArray)fake_array(0, 1, NULL), (jbyteArray)fake_array(0, 1, NULL),
                                        (jbyteArray)fake_array(0, 1, NULL), (jlongArray)fake_array(1, 8, NULL),
                                        (jlongArray)fake_array(1, 8, NULL), (jbyteArray)fake_array(0, 1, NULL),
                                        (jlongArray)fake_array(1, 8, NULL), 0, (jbyteArray)fake_array(0, 1, NULL),
                                        (jbyteArray)fake_array(0, 1, NULL), NULL);
  printf("X 4 %d %s\n", fake.pending, fake.exc_class);
  return 0;
}
