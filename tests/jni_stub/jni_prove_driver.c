/* TEST INFRASTRUCTURE ONLY: jni/khst_jni.c's prove and verifyProofs through the in-process JNIEnv
 * of fake_env.c (tests/test_gpu_prove.py compiles and runs it).
 *
 *   jni_prove_driver FILE   FILE as jni_driver's (u32 klen, u64 n, keys[n*klen], u64 voff[n+1],
 *                           vals), then u64 nq and the nq keys to prove.
 * openHost, then prove plain (s = 0) and with KH_PROVE_SHARED (s = 1) over arrays that start too
 * small (grown when prove returns -1), then verifyProofs of what prove returned:
 *   "P s found status count enc.." per key, "G s grows" per mode, "V key value" per key of the
 * shared run ("-" for no value); "E pending exc" ends the output. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fake_env.h"
#include "khst.h"

jlong Java_khipu_trie_gpu_Khst_openHost(JNIEnv*, jclass, jbyteArray, jint, jbyteArray, jlongArray, jint, jbyteArray);
jlong Java_khipu_trie_gpu_Khst_prove(JNIEnv*, jclass, jlong, jintArray, jbyteArray, jint, jint, jbyteArray, jbyteArray,
                                     jbyteArray, jlongArray, jintArray, jlongArray, jlongArray);
jlong Java_khipu_trie_gpu_Khst_verifyProofs(JNIEnv*, jclass, jbyteArray, jbyteArray, jint, jint, jbyteArray, jlongArray,
                                            jint, jintArray, jlongArray, jbyteArray, jbyteArray, jlongArray, jlongArray);
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
  uint8_t* q = malloc(nq * klen + 1);
  if (fread(q, klen, nq, f) != nq) return 2;
  fclose(f);
  const uint32_t flags = klen == 32 ? 0 : KH_HASH_KEYS;
  JNIEnv* env = fake_env();
  FakeObj* rootOut = fake_array(32, 1, NULL);
  const jlong h = Java_khipu_trie_gpu_Khst_openHost(
      env, NULL, (jbyteArray)fake_array((jsize)(n * klen), 1, keys), (jint)klen, (jbyteArray)fake_array((jsize)voff[n], 1, vals),
      (jlongArray)fake_array((jsize)(n + 1), 8, voff), (jint)flags, (jbyteArray)rootOut);
  if (!h || fake.pending) return 3;
  FakeObj* qk = fake_array((jsize)(nq * klen), 1, q);
  for (int shared = 0; shared < 2 && !fake.pending; ++shared) {
    FakeObj* sizes = fake_array(3, 8, NULL);
    FakeObj* found = fake_array((jsize)nq, 1, NULL);
    FakeObj* po = fake_array((jsize)(nq + 1), 8, NULL);
    uint64_t node_cap = 4, rlp_cap = 64, path_cap = 4; /* (too small: the grow path runs) */
    FakeObj *hs = NULL, *rl = NULL, *of = NULL, *pi = NULL;
    jlong got = -1;
    int grows = 0;
    while (got < 0 && !fake.pending && grows < 8) {
      hs = fake_array((jsize)(32 * node_cap), 1, NULL);
      rl = fake_array((jsize)rlp_cap, 1, NULL);
      of = fake_array((jsize)(node_cap + 1), 8, NULL);
      pi = fake_array((jsize)path_cap, 4, NULL);
      got = Java_khipu_trie_gpu_Khst_prove(env, NULL, h, NULL, (jbyteArray)qk, (jint)klen, shared ? (jint)KH_PROVE_SHARED : 0,
                                           (jbyteArray)found, (jbyteArray)hs, (jbyteArray)rl, (jlongArray)of, (jintArray)pi,
                                           (jlongArray)po, (jlongArray)sizes);
      if (got < 0) { /* grow to what the call needs */
        const jlong* sz = (const jlong*)sizes->data;
        if ((uint64_t)sz[0] > node_cap) node_cap = (uint64_t)sz[0];
        if ((uint64_t)sz[1] > rlp_cap) rlp_cap = (uint64_t)sz[1];
        if ((uint64_t)sz[2] > path_cap) path_cap = (uint64_t)sz[2];
        ++grows;
      }
    }
    if (got < 0 || fake.pending) break;
    /* verifyProofs over the same arrays; the values' size negotiated from an empty array */
    FakeObj* status = fake_array((jsize)nq, 1, NULL);
    FakeObj* vo = fake_array((jsize)(nq + 1), 8, NULL);
    FakeObj* vsz = fake_array(1, 8, NULL);
    FakeObj* vv = fake_array(0, 1, NULL);
    jlong vb = Java_khipu_trie_gpu_Khst_verifyProofs(env, NULL, (jbyteArray)rootOut, (jbyteArray)qk, (jint)klen, (jint)flags,
                                                     (jbyteArray)rl, (jlongArray)of, (jint)got, (jintArray)pi, (jlongArray)po,
                                                     (jbyteArray)status, (jbyteArray)vv, (jlongArray)vo, (jlongArray)vsz);
    if (vb < 0 && !fake.pending) {
      vv = fake_array((jsize)((const jlong*)vsz->data)[0], 1, NULL);
      vb = Java_khipu_trie_gpu_Khst_verifyProofs(env, NULL, (jbyteArray)rootOut, (jbyteArray)qk, (jint)klen, (jint)flags,
                                                 (jbyteArray)rl, (jlongArray)of, (jint)got, (jintArray)pi, (jlongArray)po,
                                                 (jbyteArray)status, (jbyteArray)vv, (jlongArray)vo, (jlongArray)vsz);
    }
    if (vb < 0 || fake.pending) break;
    const uint64_t* off = (const uint64_t*)of->data;
    const uint64_t* poff = (const uint64_t*)po->data;
    const uint32_t* pidx = (const uint32_t*)pi->data;
    const uint64_t* voff2 = (const uint64_t*)vo->data;
    for (uint64_t i = 0; i < nq; ++i) {
      printf("P %d %d %d %llu", shared, (int)((const uint8_t*)found->data)[i], (int)((const uint8_t*)status->data)[i],
             (unsigned long long)(poff[i + 1] - poff[i]));
      for (uint64_t k = poff[i]; k < poff[i + 1]; ++k) {
        printf(" ");
        put_hex((const uint8_t*)rl->data + off[pidx[k]], off[pidx[k] + 1] - off[pidx[k]]);
      }
      printf("\n");
      if (shared) {
        printf("V ");
        put_hex(q + i * klen, klen);
        printf(" ");
        put_hex((const uint8_t*)vv->data + voff2[i], voff2[i + 1] - voff2[i]);
        printf("\n");
      }
    }
    printf("G %d %d\n", shared, grows);
  }
  jlong box[1] = {h};
  Java_khipu_trie_gpu_Khst_free(env, NULL, (jlongArray)fake_array(1, 8, box));
  printf("E %d %s\n", fake.pending, fake.exc_class);
  return 0;
}
