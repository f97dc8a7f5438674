/* TEST INFRASTRUCTURE ONLY: jni/khst_jni.c's ranges through the in-process JNIEnv of fake_env.c
 * (tests/test_gpu_ranges.py compiles and runs it).
 *
 *   jni_ranges_driver FILE  FILE as jni_driver's (u32 klen, u64 n, keys[n*klen], u64 voff[n+1],
 *                           vals), then u64 nb and nb batches: u64 nq, u64 max_entries, then nq
 *                           requests (origin[32], limit[32]).
 * openHost (KH_HASH_KEYS unless klen is 32), then every batch asked of the one trie (tries = null)
 * until it is done: the requests answered completely are dropped, the cut one continues at `next`;
 * the value array starts empty and is grown when ranges returns -1:
 *   "K b q key value" per entry (q: the request's index in the batch), "Q b entries calls grows" per
 * batch; "E pending exc" ends the output. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fake_env.h"
#include "khst.h"

jlong Java_khipu_trie_gpu_Khst_openHost(JNIEnv*, jclass, jbyteArray, jint, jbyteArray, jlongArray, jint, jbyteArray);
jlong Java_khipu_trie_gpu_Khst_ranges(JNIEnv*, jclass, jlong, jintArray, jbyteArray, jbyteArray, jint, jbyteArray,
                                      jbyteArray, jlongArray, jlongArray, jbyteArray, jlongArray);
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
  uint64_t n = 0, nb = 0;
  if (fread(&klen, 4, 1, f) != 1 || fread(&n, 8, 1, f) != 1) return 2;
  uint8_t* keys = malloc(n * klen + 1);
  uint64_t* voff = malloc(8 * (n + 1));
  if (fread(keys, klen, n, f) != n || fread(voff, 8, n + 1, f) != n + 1) return 2;
  uint8_t* vals = malloc(voff[n] + 1);
  if (fread(vals, 1, voff[n], f) != voff[n]) return 2;
  if (fread(&nb, 8, 1, f) != 1) return 2;
  const uint32_t flags = klen == 32 ? 0 : KH_HASH_KEYS;
  JNIEnv* env = fake_env();
  FakeObj* rootOut = fake_array(32, 1, NULL);
  const jlong h = Java_khipu_trie_gpu_Khst_openHost(
      env, NULL, (jbyteArray)fake_array((jsize)(n * klen), 1, keys), (jint)klen, (jbyteArray)fake_array((jsize)voff[n], 1, vals),
      (jlongArray)fake_array((jsize)(n + 1), 8, voff), (jint)flags, (jbyteArray)rootOut);
  if (!h || fake.pending) return 3;
  for (uint64_t b = 0; b < nb && !fake.pending; ++b) {
    uint64_t nq = 0, mx = 0;
    if (fread(&nq, 8, 1, f) != 1 || fread(&mx, 8, 1, f) != 1 || !nq) return 2;
    uint8_t* og = malloc(32 * nq);
    uint8_t* lm = malloc(32 * nq);
    for (uint64_t q = 0; q < nq; ++q)
      if (fread(og + 32 * q, 32, 1, f) != 1 || fread(lm + 32 * q, 32, 1, f) != 1) return 2;
    FakeObj* ks = fake_array((jsize)(32 * mx), 1, NULL);
    FakeObj* vo = fake_array((jsize)(mx + 1), 8, NULL);
    FakeObj* next = fake_array(32, 1, NULL);
    FakeObj* sizes = fake_array(3, 8, NULL);
    uint64_t vcap = 0, entries = 0, first = 0; /* (vcap too small: the grow path runs); first: the request the call starts at */
    int calls = 0, grows = 0;
    while (first < nq) {
      const uint64_t m = nq - first;
      FakeObj* origins = fake_array((jsize)(32 * m), 1, og + 32 * first);
      FakeObj* limits = fake_array((jsize)(32 * m), 1, lm + 32 * first);
      FakeObj* eo = fake_array((jsize)(m + 1), 8, NULL);
      FakeObj* vs = fake_array((jsize)vcap, 1, NULL);
      const jlong got = Java_khipu_trie_gpu_Khst_ranges(env, NULL, h, NULL, (jbyteArray)origins, (jbyteArray)limits, (jint)m,
                                                        (jbyteArray)ks, (jbyteArray)vs, (jlongArray)vo, (jlongArray)eo,
                                                        (jbyteArray)next, (jlongArray)sizes);
      if (fake.pending || grows > 64 || calls > 100000) break;
      const jlong* sz = (const jlong*)sizes->data;
      if (got < 0) { /* not even the first value fits: grow to a few of it */
        vcap = 3 * (uint64_t)sz[1];
        ++grows;
        continue;
      }
      ++calls;
      const uint64_t* off = (const uint64_t*)vo->data;
      const uint64_t* span = (const uint64_t*)eo->data;
      if (span[m] != (uint64_t)got) return 4;
      for (uint64_t q = 0; q < m; ++q)
        for (uint64_t e = span[q]; e < span[q + 1]; ++e) {
          printf("K %llu %llu ", (unsigned long long)b, (unsigned long long)(first + q));
          put_hex((const uint8_t*)ks->data + 32 * e, 32);
          printf(" ");
          put_hex((const uint8_t*)vs->data + off[e], off[e + 1] - off[e]);
          printf("\n");
        }
      entries += (uint64_t)got;
      const uint64_t done = (uint64_t)sz[2];
      if (done < m) memcpy(og + 32 * (first + done), next->data, 32);
      first += done;
    }
    printf("Q %llu %llu %d %d\n", (unsigned long long)b, (unsigned long long)entries, calls, grows);
    free(og);
    free(lm);
  }
  fclose(f);
  jlong box[1] = {h};
  Java_khipu_trie_gpu_Khst_free(env, NULL, (jlongArray)fake_array(1, 8, box));
  printf("E %d %s\n", fake.pending, fake.exc_class);
  return 0;
}
