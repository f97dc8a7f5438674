/* TEST INFRASTRUCTURE ONLY: jni/khst_jni.c's diffs through the in-process JNIEnv of fake_env.c
 * (tests/test_gpu_diffs.py compiles and runs it).
 *
 *   jni_diffs_driver FILE  FILE: u64 n, keys[n*32], u64 voff[n+1], vals (the trie); the same again (a
 *                          block's upserts); u64 ndel, keys[ndel*32] (its deletes); then u64 nb and nb
 *                          batches: u64 nq, u64 max_entries, then nq requests (origin[32], limit[32]).
 * openHost, copy, apply of the block on the copy ("T root"), then every batch -- the original as side
 * a, the copy as side b, both single tries (triesA = triesB = null) -- asked until it is done: the
 * requests answered completely are dropped, the cut one continues at `next`; the value array starts
 * empty and is grown when diffs returns -1:
 *   "K b q key kind value" per difference (q: the request's index in the batch), "Q b differences
 * calls grows" per batch; "E pending exc" ends the output. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fake_env.h"
#include "khst.h"

jlong Java_khipu_trie_gpu_Khst_openHost(JNIEnv*, jclass, jbyteArray, jint, jbyteArray, jlongArray, jint, jbyteArray);
jlong Java_khipu_trie_gpu_Khst_copy(JNIEnv*, jclass, jlong);
jbyteArray Java_khipu_trie_gpu_Khst_apply(JNIEnv*, jclass, jlong, jbyteArray, jbyteArray, jlongArray, jbyteArray, jint, jint,
                                          jlongArray);
jlong Java_khipu_trie_gpu_Khst_diffs(JNIEnv*, jclass, jlong, jintArray, jlong, jintArray, jbyteArray, jbyteArray, jint,
                                     jbyteArray, jbyteArray, jbyteArray, jlongArray, jlongArray, jbyteArray, jlongArray);
void Java_khipu_trie_gpu_Khst_free(JNIEnv*, jclass, jlongArray);

static void put_hex(const uint8_t* p, uint64_t n) {
  if (!n) printf("-");
  for (uint64_t i = 0; i < n; ++i) printf("%02x", p[i]);
}

typedef struct {
  uint64_t n;
  uint8_t* keys;
  uint64_t* voff;
  uint8_t* vals;
} Packed;

static int read_packed(FILE* f, Packed* p) {
  if (fread(&p->n, 8, 1, f) != 1) return 0;
  p->keys = malloc(p->n * 32 + 1);
  p->voff = malloc(8 * (p->n + 1));
  if (fread(p->keys, 32, p->n, f) != p->n || fread(p->voff, 8, p->n + 1, f) != p->n + 1) return 0;
  p->vals = malloc(p->voff[p->n] + 1);
  return fread(p->vals, 1, p->voff[p->n], f) == p->voff[p->n];
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  Packed t, up;
  uint64_t ndel = 0, nb = 0;
  if (!read_packed(f, &t) || !read_packed(f, &up) || fread(&ndel, 8, 1, f) != 1) return 2;
  uint8_t* dels = malloc(ndel * 32 + 1);
  if (fread(dels, 32, ndel, f) != ndel || fread(&nb, 8, 1, f) != 1) return 2;
  JNIEnv* env = fake_env();
  FakeObj* rootOut = fake_array(32, 1, NULL);
  const jlong a = Java_khipu_trie_gpu_Khst_openHost(
      env, NULL, (jbyteArray)fake_array((jsize)(t.n * 32), 1, t.keys), 32, (jbyteArray)fake_array((jsize)t.voff[t.n], 1, t.vals),
      (jlongArray)fake_array((jsize)(t.n + 1), 8, t.voff), 0, (jbyteArray)rootOut);
  if (!a || fake.pending) return 3;
  const jlong b = Java_khipu_trie_gpu_Khst_copy(env, NULL, a);
  if (!b || fake.pending) return 3;
  FakeObj* root = (FakeObj*)Java_khipu_trie_gpu_Khst_apply(
      env, NULL, b, (jbyteArray)fake_array((jsize)(up.n * 32), 1, up.keys), (jbyteArray)fake_array((jsize)up.voff[up.n], 1, up.vals),
      (jlongArray)fake_array((jsize)(up.n + 1), 8, up.voff), (jbyteArray)fake_array((jsize)(ndel * 32), 1, dels), 32, 0, NULL);
  if (!root || fake.pending) return 3;
  printf("T ");
  put_hex((const uint8_t*)root->data, 32);
  printf("\n");
  for (uint64_t bi = 0; bi < nb && !fake.pending; ++bi) {
    uint64_t nq = 0, mx = 0;
    if (fread(&nq, 8, 1, f) != 1 || fread(&mx, 8, 1, f) != 1 || !nq) return 2;
    uint8_t* og = malloc(32 * nq);
    uint8_t* lm = malloc(32 * nq);
    for (uint64_t q = 0; q < nq; ++q)
      if (fread(og + 32 * q, 32, 1, f) != 1 || fread(lm + 32 * q, 32, 1, f) != 1) return 2;
    FakeObj* ks = fake_array((jsize)(32 * mx), 1, NULL);
    FakeObj* kd = fake_array((jsize)mx, 1, NULL);
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
      const jlong got = Java_khipu_trie_gpu_Khst_diffs(env, NULL, a, NULL, b, NULL, (jbyteArray)origins, (jbyteArray)limits,
                                                       (jint)m, (jbyteArray)ks, (jbyteArray)kd, (jbyteArray)vs, (jlongArray)vo,
                                                       (jlongArray)eo, (jbyteArray)next, (jlongArray)sizes);
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
          printf("K %llu %llu ", (unsigned long long)bi, (unsigned long long)(first + q));
          put_hex((const uint8_t*)ks->data + 32 * e, 32);
          printf(" %u ", (unsigned)((const uint8_t*)kd->data)[e]);
          put_hex((const uint8_t*)vs->data + off[e], off[e + 1] - off[e]);
          printf("\n");
        }
      entries += (uint64_t)got;
      const uint64_t done = (uint64_t)sz[2];
      if (done < m) memcpy(og + 32 * (first + done), next->data, 32);
      first += done;
    }
    printf("Q %llu %llu %d %d\n", (unsigned long long)bi, (unsigned long long)entries, calls, grows);
    free(og);
    free(lm);
  }
  fclose(f);
  jlong box[2] = {a, b};
  Java_khipu_trie_gpu_Khst_free(env, NULL, (jlongArray)fake_array(2, 8, box));
  printf("E %d %s\n", fake.pending, fake.exc_class);
  return 0;
}
