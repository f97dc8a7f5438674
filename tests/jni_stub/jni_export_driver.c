/* TEST INFRASTRUCTURE ONLY: jni/khst_jni.c's exportNodes and nodesByHash through the in-process
 * JNIEnv of fake_env.c (tests/test_gpu_export.py compiles and runs it).
 *
 *   jni_export_driver FILE   FILE as jni_driver's: u32 klen, u64 n, keys[n*klen], u64 voff[n+1], vals.
 * openHost, then the cursor loop of INTEGRATION.md over small arrays (grown when exportNodes
 * returns -1), one "N hash enc" line per node; then nodesByHash of the first 40 exported hashes
 * and one absent hash, one "B hash enc" line each ("-" for null); "E pending exc" ends the output. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fake_env.h"
#include "khst.h"

jlong Java_khipu_trie_gpu_Khst_openHost(JNIEnv*, jclass, jbyteArray, jint, jbyteArray, jlongArray, jint, jbyteArray);
jlong Java_khipu_trie_gpu_Khst_exportNodes(JNIEnv*, jclass, jlong, jint, jint, jlongArray, jbyteArray, jbyteArray,
                                           jlongArray, jlongArray);
jobjectArray Java_khipu_trie_gpu_Khst_nodesByHash(JNIEnv*, jclass, jlong, jbyteArray);
void Java_khipu_trie_gpu_Khst_free(JNIEnv*, jclass, jlongArray);

static void put_hex(const uint8_t* p, uint64_t n) {
  for (uint64_t i = 0; i < n; ++i) printf("%02x", p[i]);
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t klen = 0;
  uint64_t n = 0;
  if (fread(&klen, 4, 1, f) != 1 || fread(&n, 8, 1, f) != 1) return 2;
  uint8_t* keys = malloc(n * klen + 1);
  uint64_t* voff = malloc(8 * (n + 1));
  if (fread(keys, klen, n, f) != n || fread(voff, 8, n + 1, f) != n + 1) return 2;
  uint8_t* vals = malloc(voff[n] + 1);
  if (fread(vals, 1, voff[n], f) != voff[n]) return 2;
  fclose(f);
  const uint32_t flags = klen == 32 ? 0 : KH_HASH_KEYS;
  JNIEnv* env = fake_env();
  FakeObj* rootOut = fake_array(32, 1, NULL);
  const jlong h = Java_khipu_trie_gpu_Khst_openHost(
      env, NULL, (jbyteArray)fake_array((jsize)(n * klen), 1, keys), (jint)klen, (jbyteArray)fake_array((jsize)voff[n], 1, vals),
      (jlongArray)fake_array((jsize)(n + 1), 8, voff), (jint)flags, (jbyteArray)rootOut);
  if (!h || fake.pending) return 3;
  /* the cursor loop */
  const jlong zero2[2] = {0, 0};
  FakeObj* cursor = fake_array(2, 8, zero2);
  FakeObj* sizes = fake_array(3, 8, NULL);
  uint64_t node_cap = 8, rlp_cap = 64; /* (too small for a branch: the grow path runs) */
  uint8_t first[41 * 32];
  uint32_t nfirst = 0;
  int done = 0, calls = 0, grows = 0;
  while (!done && !fake.pending && calls < 100000) {
    FakeObj* hs = fake_array((jsize)(32 * node_cap), 1, NULL);
    FakeObj* rl = fake_array((jsize)rlp_cap, 1, NULL);
    FakeObj* of = fake_array((jsize)(node_cap + 1), 8, NULL);
    const jlong got = Java_khipu_trie_gpu_Khst_exportNodes(env, NULL, h, -1, (jint)KH_EXPORT_VERIFY, (jlongArray)cursor,
                                                           (jbyteArray)hs, (jbyteArray)rl, (jlongArray)of, (jlongArray)sizes);
    ++calls;
    const jlong* sz = (const jlong*)sizes->data;
    if (got < 0) { /* grow to what the next record needs */
      if ((uint64_t)sz[0] > node_cap) node_cap = (uint64_t)sz[0];
      if ((uint64_t)sz[1] > rlp_cap) rlp_cap = (uint64_t)sz[1];
      ++grows;
      continue;
    }
    const uint64_t* off = (const uint64_t*)of->data;
    for (jlong j = 0; j < got; ++j) {
      const uint8_t* hh = (const uint8_t*)hs->data + 32 * j;
      printf("N ");
      put_hex(hh, 32);
      printf(" ");
      put_hex((const uint8_t*)rl->data + off[j], off[j + 1] - off[j]);
      printf("\n");
      if (nfirst < 40) memcpy(first + 32 * nfirst++, hh, 32);
    }
    done = (int)sz[2];
  }
  printf("C %d %d\n", calls, grows);
  /* by hash: the first exported hashes and one absent */
  for (int i = 0; i < 32; ++i) first[32 * nfirst + i] = (uint8_t)(0x5A ^ i);
  if (!fake.pending) {
    jobjectArray got = Java_khipu_trie_gpu_Khst_nodesByHash(env, NULL, h, (jbyteArray)fake_array((jsize)(32 * (nfirst + 1)), 1, first));
    for (uint32_t i = 0; got && !fake.pending && i <= nfirst; ++i) {
      FakeObj* v = ((FakeObj**)((FakeObj*)got)->data)[i];
      printf("B ");
      put_hex(first + 32 * i, 32);
      printf(" ");
      if (v)
        put_hex(v->data, (uint64_t)v->len);
      else
        printf("-");
      printf("\n");
    }
  }
  jlong box[1] = {h};
  Java_khipu_trie_gpu_Khst_free(env, NULL, (jlongArray)fake_array(1, 8, box));
  printf("E %d %s\n", fake.pending, fake.exc_class);
  return 0;
}
