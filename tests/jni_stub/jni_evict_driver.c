/* TEST INFRASTRUCTURE ONLY: jni/khst_jni.c's evictSubtrees, then apply (refused:
 * MPTNodeMissingException), fillNodes and apply again, through the in-process JNIEnv of fake_env.c
 * (tests/test_gpu_evict.py compiles and runs it).
 *
 *   jni_evict_driver FILE
 * FILE: 32-byte root; 32-byte key, u64 vlen, the value (one upsert); u64 np, np depth bytes, np
 * 32-byte paths (the prefixes to evict); u64 n, u64 off[n+1], the n node encodings packed (the whole
 * store: the trie is opened from it in full, and the fill is given it again).
 * openPartial over the store: "O handle_ok pending stubs"; evictSubtrees: "V keys pending stubs",
 * then "S status hash" per prefix; apply of the upsert: "A pending exc factory_calls hash";
 * fillNodes over the store: "F decoded pending stubs"; apply again: "C pending root"; "E pending exc"
 * ends the output. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fake_env.h"
#include "khst.h"

jlong Java_khipu_trie_gpu_Khst_openPartial(JNIEnv*, jclass, jbyteArray, jbyteArray, jlongArray, jint, jbyteArray);
jbyteArray Java_khipu_trie_gpu_Khst_apply(JNIEnv*, jclass, jlong, jbyteArray, jbyteArray, jlongArray, jbyteArray, jint,
                                          jint, jlongArray);
jlong Java_khipu_trie_gpu_Khst_evictSubtrees(JNIEnv*, jclass, jlong, jintArray, jbyteArray, jbyteArray, jbyteArray,
                                             jbyteArray);
jlong Java_khipu_trie_gpu_Khst_fillNodes(JNIEnv*, jclass, jlong, jbyteArray, jlongArray);
jlong Java_khipu_trie_gpu_Khst_stubs(JNIEnv*, jclass, jlong);
void Java_khipu_trie_gpu_Khst_free(JNIEnv*, jclass, jlongArray);

static void put_hex(const uint8_t* p, uint64_t n) {
  if (!n) printf("-");
  for (uint64_t i = 0; i < n; ++i) printf("%02x", p[i]);
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint8_t root[32], key[32];
  uint64_t vlen = 0, np = 0, n = 0;
  if (fread(root, 32, 1, f) != 1 || fread(key, 32, 1, f) != 1 || fread(&vlen, 8, 1, f) != 1) return 2;
  uint8_t* val = malloc(vlen + 1);
  if (vlen && fread(val, 1, vlen, f) != vlen) return 2;
  if (fread(&np, 8, 1, f) != 1 || np < 1 || np > 1024) return 2;
  uint8_t* depths = malloc(np);
  uint8_t* paths = malloc(32 * np);
  if (fread(depths, 1, np, f) != np || fread(paths, 32, np, f) != np) return 2;
  if (fread(&n, 8, 1, f) != 1 || n < 1) return 2;
  uint64_t* off = malloc(8 * (n + 1));
  if (fread(off, 8, n + 1, f) != n + 1) return 2;
  uint8_t* enc = malloc(off[n] + 1);
  if (fread(enc, 1, off[n], f) != off[n]) return 2;
  fclose(f);
  JNIEnv* env = fake_env();
  FakeObj* je = fake_array((jsize)off[n], 1, enc);
  FakeObj* jf = fake_array((jsize)(n + 1), 8, off);
  const jlong h = Java_khipu_trie_gpu_Khst_openPartial(env, NULL, (jbyteArray)fake_array(32, 1, root), (jbyteArray)je,
                                                       (jlongArray)jf, 0, NULL);
  printf("O %d %d %lld\n", h != 0, fake.pending, h ? (long long)Java_khipu_trie_gpu_Khst_stubs(env, NULL, h) : -1);
  if (!h || fake.pending) return 3;
  uint8_t* zero = calloc(32 * np, 1);
  FakeObj* js = fake_array((jsize)np, 1, zero);
  FakeObj* jh = fake_array((jsize)(32 * np), 1, zero);
  const jlong keys = Java_khipu_trie_gpu_Khst_evictSubtrees(env, NULL, h, NULL, (jbyteArray)fake_array((jsize)(32 * np), 1, paths),
                                                            (jbyteArray)fake_array((jsize)np, 1, depths), (jbyteArray)js,
                                                            (jbyteArray)jh);
  printf("V %lld %d %lld\n", (long long)keys, fake.pending, (long long)Java_khipu_trie_gpu_Khst_stubs(env, NULL, h));
  for (uint64_t i = 0; i < np; ++i) {
    printf("S %u ", ((const uint8_t*)js->data)[i]);
    put_hex((const uint8_t*)jh->data + 32 * i, 32);
    printf("\n");
  }
  const uint64_t voff[2] = {0, vlen};
  FakeObj* jk = fake_array(32, 1, key);
  FakeObj* jv = fake_array((jsize)vlen, 1, val);
  FakeObj* jo = fake_array(2, 8, voff);
  Java_khipu_trie_gpu_Khst_apply(env, NULL, h, (jbyteArray)jk, (jbyteArray)jv, (jlongArray)jo, NULL, 32, 0, NULL);
  printf("A %d %s %d ", fake.pending, fake.exc_class, fake.node_missing_calls);
  put_hex(fake.node_missing_hash, 32);
  printf("\n");
  fake.pending = 0;
  fake.exc_class[0] = 0;
  const jlong dec = Java_khipu_trie_gpu_Khst_fillNodes(env, NULL, h, (jbyteArray)je, (jlongArray)jf);
  printf("F %lld %d %lld\n", (long long)dec, fake.pending, (long long)Java_khipu_trie_gpu_Khst_stubs(env, NULL, h));
  const FakeObj* r2 = (const FakeObj*)Java_khipu_trie_gpu_Khst_apply(env, NULL, h, (jbyteArray)jk, (jbyteArray)jv,
                                                                     (jlongArray)jo, NULL, 32, 0, NULL);
  printf("C %d ", fake.pending);
  if (r2 && r2->len == 32) put_hex((const uint8_t*)r2->data, 32);
  printf("\n");
  jlong box[1] = {h};
  Java_khipu_trie_gpu_Khst_free(env, NULL, (jlongArray)fake_array(1, 8, box));
  printf("E %d %s\n", fake.pending, fake.exc_class);
  return 0;
}
