/* TEST INFRASTRUCTURE ONLY: jni/khst_jni.c's forestLoadNodes, forestRoots and forestEvict through
 * the in-process JNIEnv of fake_env.c (tests/test_gpu_forest_load.py compiles and runs it).
 *
 *   jni_load_driver FILE   FILE: u64 k, then k x (u32 trie id, 32-byte root); u64 n, u64 off[n+1],
 *                          the n node encodings packed.
 * forestOpen; forestLoadNodes over the store without its LAST node (the test puts a node there
 * whose absence the walk meets): "X pending exc factory_calls hash n_missing idx0 hash0"; the same
 * over the whole store: "L pending"; forestRoots: "R id root" per trie; forestEvict of the first
 * listed id: "V dropped", then forestRoots again: "S id root" per trie; "E pending exc" ends the
 * output. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fake_env.h"
#include "khst.h"

jlong Java_khipu_trie_gpu_Khst_forestOpen(JNIEnv*, jclass, jint);
void Java_khipu_trie_gpu_Khst_forestLoadNodes(JNIEnv*, jclass, jlong, jintArray, jbyteArray, jbyteArray, jlongArray,
                                              jintArray, jbyteArray, jlongArray);
jbyteArray Java_khipu_trie_gpu_Khst_forestRoots(JNIEnv*, jclass, jlong);
jlong Java_khipu_trie_gpu_Khst_forestEvict(JNIEnv*, jclass, jlong, jintArray);
void Java_khipu_trie_gpu_Khst_free(JNIEnv*, jclass, jlongArray);

static void put_hex(const uint8_t* p, uint64_t n) {
  if (!n) printf("-");
  for (uint64_t i = 0; i < n; ++i) printf("%02x", p[i]);
}
static void print_roots(JNIEnv* env, jlong h, const char* tag) {
  const FakeObj* r = (const FakeObj*)Java_khipu_trie_gpu_Khst_forestRoots(env, NULL, h);
  if (!r || fake.pending) return;
  const uint8_t* p = (const uint8_t*)r->data;
  for (jsize i = 0; i + 36 <= r->len; i += 36) {
    uint32_t id;
    memcpy(&id, p + i, 4);
    printf("%s %u ", tag, id);
    put_hex(p + i + 4, 32);
    printf("\n");
  }
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint64_t k = 0, n = 0;
  if (fread(&k, 8, 1, f) != 1) return 2;
  uint32_t* ids = malloc(4 * k + 4);
  uint8_t* roots = malloc(32 * k + 1);
  for (uint64_t j = 0; j < k; ++j)
    if (fread(ids + j, 4, 1, f) != 1 || fread(roots + 32 * j, 32, 1, f) != 1) return 2;
  if (fread(&n, 8, 1, f) != 1 || n < 1) return 2;
  uint64_t* off = malloc(8 * (n + 1));
  if (fread(off, 8, n + 1, f) != n + 1) return 2;
  uint8_t* enc = malloc(off[n] + 1);
  if (fread(enc, 1, off[n], f) != off[n]) return 2;
  fclose(f);
  JNIEnv* env = fake_env();
  const jlong h = Java_khipu_trie_gpu_Khst_forestOpen(env, NULL, 0);
  if (!h || fake.pending) return 3;
  FakeObj* jt = fake_array((jsize)k, 4, ids);
  FakeObj* jr = fake_array((jsize)(32 * k), 1, roots);
  FakeObj* mi = fake_array(4, 4, NULL);
  FakeObj* mh = fake_array(4 * 32, 1, NULL);
  FakeObj* nm = fake_array(1, 8, NULL);
  /* the store without its last node: MPTNodeMissingException through Khst.nodeMissing */
  Java_khipu_trie_gpu_Khst_forestLoadNodes(env, NULL, h, (jintArray)jt, (jbyteArray)jr,
                                           (jbyteArray)fake_array((jsize)off[n - 1], 1, enc),
                                           (jlongArray)fake_array((jsize)n, 8, off), (jintArray)mi, (jbyteArray)mh,
                                           (jlongArray)nm);
  printf("X %d %s %d ", fake.pending, fake.exc_class, fake.node_missing_calls);
  put_hex(fake.node_missing_hash, 32);
  printf(" %lld %u ", (long long)((const jlong*)nm->data)[0], ((const uint32_t*)mi->data)[0]);
  put_hex((const uint8_t*)mh->data, 32);
  printf("\n");
  fake.pending = 0;
  fake.exc_class[0] = 0;
  print_roots(env, h, "Q"); /* (nothing resident after the refused load) */
  Java_khipu_trie_gpu_Khst_forestLoadNodes(env, NULL, h, (jintArray)jt, (jbyteArray)jr,
                                           (jbyteArray)fake_array((jsize)off[n], 1, enc),
                                           (jlongArray)fake_array((jsize)(n + 1), 8, off), (jintArray)mi, (jbyteArray)mh,
                                           (jlongArray)nm);
  printf("L %d\n", fake.pending);
  if (!fake.pending) {
    print_roots(env, h, "R");
    const jlong dropped = Java_khipu_trie_gpu_Khst_forestEvict(env, NULL, h, (jintArray)fake_array(1, 4, ids));
    printf("V %lld\n", (long long)dropped);
    print_roots(env, h, "S");
  }
  jlong box[1] = {h};
  Java_khipu_trie_gpu_Khst_free(env, NULL, (jlongArray)fake_array(1, 8, box));
  printf("E %d %s\n", fake.pending, fake.exc_class);
  return 0;
}
