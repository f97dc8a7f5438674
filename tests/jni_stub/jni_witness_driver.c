/* TEST INFRASTRUCTURE ONLY: jni/khst_jni.c's commitWitness on a trie opened by openHost, through the
 * in-process JNIEnv of fake_env.c (tests/test_gpu_witness.py compiles and runs it).
 *
 *   jni_witness_driver FILE
 * FILE: u64 n, nup, ndel; n 32-byte keys, u64 voff[n + 1], the values packed (the trie); nup 32-byte
 * upsert keys; ndel 32-byte delete keys.
 * commitWitness with empty arrays (the size query, -1), then with arrays of exactly the sizes it
 * reported: "W pending nodes rlp_bytes collapse", "N hash encoding" per table node in table order;
 * "E pending" ends the output. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fake_env.h"
#include "khst.h"

jlong Java_khipu_trie_gpu_Khst_openHost(JNIEnv*, jclass, jbyteArray, jint, jbyteArray, jlongArray, jint, jbyteArray);
jlong Java_khipu_trie_gpu_Khst_commitWitness(JNIEnv*, jclass, jlong, jintArray, jbyteArray, jintArray, jbyteArray, jint,
                                             jbyteArray, jbyteArray, jlongArray, jbyteArray, jlongArray);
void Java_khipu_trie_gpu_Khst_free(JNIEnv*, jclass, jlongArray);

static void put_hex(const uint8_t* p, uint64_t n) {
  if (!n) printf("-");
  for (uint64_t i = 0; i < n; ++i) printf("%02x", p[i]);
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint64_t hdr[3];
  if (fread(hdr, 8, 3, f) != 3 || hdr[0] < 1 || hdr[0] > (1u << 20) || hdr[1] > (1u << 20) || hdr[2] > (1u << 20)) return 2;
  const uint64_t n = hdr[0], nup = hdr[1], ndel = hdr[2];
  uint8_t* keys = malloc(32 * n);
  uint64_t* voff = malloc(8 * (n + 1));
  if (fread(keys, 32, n, f) != n || fread(voff, 8, n + 1, f) != n + 1) return 2;
  uint8_t* vals = malloc(voff[n] + 1);
  if (fread(vals, 1, voff[n], f) != voff[n]) return 2;
  uint8_t* uk = malloc(32 * nup + 1);
  uint8_t* dk = malloc(32 * ndel + 1);
  if (fread(uk, 32, nup, f) != nup || fread(dk, 32, ndel, f) != ndel) return 2;
  fclose(f);
  JNIEnv* env = fake_env();
  const jlong h = Java_khipu_trie_gpu_Khst_openHost(env, NULL, (jbyteArray)fake_array((jsize)(32 * n), 1, keys), 32,
                                                    (jbyteArray)fake_array((jsize)voff[n], 1, vals),
                                                    (jlongArray)fake_array((jsize)(n + 1), 8, voff), 0, NULL);
  if (!h || fake.pending) return 3;
  FakeObj* ju = fake_array((jsize)(32 * nup), 1, uk);
  FakeObj* jd = fake_array((jsize)(32 * ndel), 1, dk);
  const uint64_t zero[4] = {0, 0, 0, 0};
  FakeObj* jsz = fake_array(4, 8, zero);
  FakeObj* jo0 = fake_array(1, 8, zero);
  const jlong q = Java_khipu_trie_gpu_Khst_commitWitness(env, NULL, h, NULL, (jbyteArray)ju, NULL, (jbyteArray)jd, 32,
                                                         (jbyteArray)fake_array(0, 1, zero), (jbyteArray)fake_array(0, 1, zero),
                                                         (jlongArray)jo0, NULL, (jlongArray)jsz);
  if (q != -1 || fake.pending) return 4;
  const uint64_t nn = ((const uint64_t*)jsz->data)[0], nb = ((const uint64_t*)jsz->data)[1];
  uint8_t* zh = calloc(32 * nn + 1, 1);
  uint8_t* zr = calloc(nb + 1, 1);
  uint64_t* zo = calloc(nn + 1, 8);
  FakeObj* jh = fake_array((jsize)(32 * nn), 1, zh);
  FakeObj* jr = fake_array((jsize)nb, 1, zr);
  FakeObj* jo = fake_array((jsize)(nn + 1), 8, zo);
  const jlong got = Java_khipu_trie_gpu_Khst_commitWitness(env, NULL, h, NULL, (jbyteArray)ju, NULL, (jbyteArray)jd, 32,
                                                           (jbyteArray)jh, (jbyteArray)jr, (jlongArray)jo, NULL,
                                                           (jlongArray)jsz);
  const uint64_t* sz = (const uint64_t*)jsz->data;
  printf("W %d %lld %llu %llu\n", fake.pending, (long long)got, (unsigned long long)sz[1], (unsigned long long)sz[2]);
  const uint64_t* of = (const uint64_t*)jo->data;
  for (jlong j = 0; j < got; ++j) {
    printf("N ");
    put_hex((const uint8_t*)jh->data + 32 * j, 32);
    printf(" ");
    put_hex((const uint8_t*)jr->data + of[j], of[j + 1] - of[j]);
    printf("\n");
  }
  jlong box[1] = {h};
  Java_khipu_trie_gpu_Khst_free(env, NULL, (jlongArray)fake_array(1, 8, box));
  printf("E %d\n", fake.pending);
  return 0;
}
