/* TEST INFRASTRUCTURE ONLY: jni/khst_jni.c's fillRanges through the in-process JNIEnv of fake_env.c
 * (tests/test_gpu_fillrange.py compiles and runs it).
 *
 *   jni_fillrange_driver FILE
 * FILE: 32-byte root, 32-byte origin; u64 n, u64 off[n+1], the n node encodings packed (the FIRST is
 * the witness the trie is opened from, the whole set the boundary proof given to fillNodes); then
 * two pages, each u64 ne, u64 vb, keys[32 ne], vals[vb], u64 voff[ne + 1]: a refused one, then the
 * honest one.
 * openPartial over the first node and fillNodes: "O handle_ok pending stubs"; per page one
 * fillRanges call: "F bad status stubs_left keys_gained stubs_replaced pending size stubs"; "E
 * pending exc" ends the output. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fake_env.h"
#include "khst.h"

jlong Java_khipu_trie_gpu_Khst_openPartial(JNIEnv*, jclass, jbyteArray, jbyteArray, jlongArray, jint, jbyteArray);
jlong Java_khipu_trie_gpu_Khst_fillNodes(JNIEnv*, jclass, jlong, jbyteArray, jlongArray);
jlong Java_khipu_trie_gpu_Khst_fillRanges(JNIEnv*, jclass, jlong, jintArray, jbyteArray, jbyteArray, jbyteArray, jbyteArray,
                                          jlongArray, jlongArray, jbyteArray, jlongArray, jlongArray);
jlong Java_khipu_trie_gpu_Khst_stubs(JNIEnv*, jclass, jlong);
jlong Java_khipu_trie_gpu_Khst_size(JNIEnv*, jclass, jlong);
void Java_khipu_trie_gpu_Khst_free(JNIEnv*, jclass, jlongArray);

static void* slurp(FILE* f, size_t esz, uint64_t n) {
  void* p = malloc(esz * n + 1);
  if (!p || fread(p, esz, n, f) != n) exit(2);
  return p;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint8_t* root = slurp(f, 32, 1);
  uint8_t* origin = slurp(f, 32, 1);
  uint64_t n = 0;
  if (fread(&n, 8, 1, f) != 1 || n < 1) return 2;
  uint64_t* off = slurp(f, 8, n + 1);
  uint8_t* enc = slurp(f, 1, off[n]);
  JNIEnv* env = fake_env();
  const jlong h = Java_khipu_trie_gpu_Khst_openPartial(env, NULL, (jbyteArray)fake_array(32, 1, root),
                                                       (jbyteArray)fake_array((jsize)off[1], 1, enc),
                                                       (jlongArray)fake_array(2, 8, off), 0, NULL);
  if (!h || fake.pending) return 3;
  Java_khipu_trie_gpu_Khst_fillNodes(env, NULL, h, (jbyteArray)fake_array((jsize)off[n], 1, enc),
                                     (jlongArray)fake_array((jsize)(n + 1), 8, off));
  printf("O %d %d %lld\n", h != 0, fake.pending, (long long)Java_khipu_trie_gpu_Khst_stubs(env, NULL, h));
  for (int page = 0; page < 2 && !fake.pending; ++page) {
    uint64_t hd[2];
    if (fread(hd, 8, 2, f) != 2) return 2;
    const uint64_t ne = hd[0], vb = hd[1];
    uint8_t* keys = slurp(f, 32, ne);
    uint8_t* vals = slurp(f, 1, vb);
    uint64_t* voff = slurp(f, 8, ne + 1);
    const uint64_t eoff[2] = {0, ne};
    FakeObj* status = fake_array(1, 1, NULL);
    FakeObj* left = fake_array(1, 8, NULL);
    FakeObj* gained = fake_array(2, 8, NULL);
    const jlong bad = Java_khipu_trie_gpu_Khst_fillRanges(
        env, NULL, h, NULL, (jbyteArray)fake_array(32, 1, root), (jbyteArray)fake_array(32, 1, origin),
        (jbyteArray)fake_array((jsize)(32 * ne), 1, keys), (jbyteArray)fake_array((jsize)vb, 1, vals),
        (jlongArray)fake_array((jsize)(ne + 1), 8, voff), (jlongArray)fake_array(2, 8, eoff), (jbyteArray)status,
        (jlongArray)left, (jlongArray)gained);
    const int pending = fake.pending;
    printf("F %lld %u %lld %lld %lld %d %lld %lld\n", (long long)bad, ((const uint8_t*)status->data)[0],
           (long long)((const jlong*)left->data)[0], (long long)((const jlong*)gained->data)[0],
           (long long)((const jlong*)gained->data)[1], pending, (long long)Java_khipu_trie_gpu_Khst_size(env, NULL, h),
           (long long)Java_khipu_trie_gpu_Khst_stubs(env, NULL, h));
  }
  fclose(f);
  jlong box[1] = {h};
  Java_khipu_trie_gpu_Khst_free(env, NULL, (jlongArray)fake_array(1, 8, box));
  printf("E %d %s\n", fake.pending, fake.exc_class);
  return 0;
}
