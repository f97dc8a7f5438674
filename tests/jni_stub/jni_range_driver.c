/* TEST INFRASTRUCTURE ONLY: jni/khst_jni.c's range through the in-process JNIEnv of fake_env.c
 * (tests/test_gpu_range.py compiles and runs it).
 *
 *   jni_range_driver FILE   FILE as jni_driver's (u32 klen, u64 n, keys[n*klen], u64 voff[n+1],
 *                           vals), then u64 nq and nq queries (origin[32], limit[32], u64 max_entries).
 * openHost (KH_HASH_KEYS unless klen is 32), then every query paged to its end by `next`, the
 * value array starting empty and grown when range returns -1:
 *   "K q key value" per entry, "Q q entries pages grows" per query; "E pending exc" ends the output. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fake_env.h"
#include "khst.h"

jlong Java_khipu_trie_gpu_Khst_openHost(JNIEnv*, jclass, jbyteArray, jint, jbyteArray, jlongArray, jint, jbyteArray);
jlong Java_khipu_trie_gpu_Khst_range(JNIEnv*, jclass, jlong, jint, jbyteArray, jbyteArray, jbyteArray, jbyteArray,
                                     jlongArray, jbyteArray, jlongArray);
void Java_khipu_trie_gpu_Khst_free(JNIEnv*, jclass, jlongArray);

static void put_hex(const uint8_t* p, uint64_t n) {
  if (!n) printf("-");
  for (uint64_t i = 0; i < n; ++i) printf("%02x", p[i]);
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t klen = 0;
  uint64_t n = 0, nq = 0;
  if (fread(&klen, 4, 1, f) != 1 || fread(&n, 8, 1, f) != 1) return 2;
  uint8_t* keys = malloc(n * klen + 1);
  uint64_t* voff = malloc(8 * (n + 1));
  if (fread(keys, klen, n, f) != n || fread(voff, 8, n + 1, f) != n + 1) return 2;
  uint8_t* vals = malloc(voff[n] + 1);
  if (fread(vals, 1, voff[n], f) != voff[n]) return 2;
  if (fread(&nq, 8, 1, f) != 1) return 2;
  uint8_t* q = malloc(nq * 72 + 1);
  if (fread(q, 72, nq, f) != nq) return 2;
  fclose(f);
  const uint32_t flags = klen == 32 ? 0 : KH_HASH_KEYS;
  JNIEnv* env = fake_env();
  FakeObj* rootOut = fake_array(32, 1, NULL);
  const jlong h = Java_khipu_trie_gpu_Khst_openHost(
      env, NULL, (jbyteArray)fake_array((jsize)(n * klen), 1, keys), (jint)klen, (jbyteArray)fake_array((jsize)voff[n], 1, vals),
      (jlongArray)fake_array((jsize)(n + 1), 8, voff), (jint)flags, (jbyteArray)rootOut);
  if (!h || fake.pending) return 3;
  for (uint64_t i = 0; i < nq && !fake.pending; ++i) {
    uint64_t mx = 0;
    memcpy(&mx, q + 72 * i + 64, 8);
    FakeObj* origin = fake_array(32, 1, q + 72 * i);
    FakeObj* limit = fake_array(32, 1, q + 72 * i + 32);
    FakeObj* ks = fake_array((jsize)(32 * mx), 1, NULL);
    FakeObj* vo = fake_array((jsize)(mx + 1), 8, NULL);
    FakeObj* next = fake_array(32, 1, NULL);
    FakeObj* sizes = fake_array(3, 8, NULL);
    uint64_t vcap = 0, entries = 0; /* (too small: the grow path runs) */
    int pages = 0, grows = 0;
    for (;;) {
      FakeObj* vs = fake_array((jsize)vcap, 1, NULL);
      const jlong got = Java_khipu_trie_gpu_Khst_range(env, NULL, h, 0, (jbyteArray)origin, (jbyteArray)limit, (jbyteArray)ks,
                                                       (jbyteArray)vs, (jlongArray)vo, (jbyteArray)next, (jlongArray)sizes);
      if (fake.pending || grows > 64) break;
      const jlong* sz = (const jlong*)sizes->data;
      if (got < 0) { /* not even the first value fits: grow to a few of it */
        vcap = 3 * (uint64_t)sz[1];
        ++grows;
        continue;
      }
      ++pages;
      const uint64_t* off = (const uint64_t*)vo->data;
      for (jlong e = 0; e < got; ++e) {
        printf("K %llu ", (unsigned long long)i);
        put_hex((const uint8_t*)ks->data + 32 * e, 32);
        printf(" ");
        put_hex((const uint8_t*)vs->data + off[e], off[e + 1] - off[e]);
        printf("\n");
      }
      entries += (uint64_t)got;
      if (!sz[2]) break;
      origin = fake_array(32, 1, next->data);
    }
    printf("Q %llu %llu %d %d\n", (unsigned long long)i, (unsigned long long)entries, pages, grows);
  }
  jlong box[1] = {h};
  Java_khipu_trie_gpu_Khst_free(env, NULL, (jlongArray)fake_array(1, 8, box));
  printf("E %d %s\n", fake.pending, fake.exc_class);
  return 0;
}
