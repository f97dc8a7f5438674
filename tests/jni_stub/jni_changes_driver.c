/* TEST INFRASTRUCTURE ONLY: jni/khst_jni.c's changesSince through the in-process JNIEnv of fake_env.c
 * (tests/test_changes_jni.py compiles and runs it; no device is needed: every check here is refused
 * before the library touches one).
 *
 *   jni_changes_driver   one JSON line a check: {"check": name, "ret": returned, "pending": 0|1, "exc": class}
 *     next_short     next holds 31 bytes                      IllegalArgumentException, no library call
 *     sizes_short    sizes holds 4 longs                      IllegalArgumentException
 *     from_short     from holds 31 bytes                      IllegalArgumentException
 *     no_room        keys holds no whole key                  IllegalArgumentException
 *     tries_bound    tries shorter than keys: it bounds max_entries; with no entry left, refused
 *     null_handle    handle 0: the library's KH_EINVAL        MerklePatriciaTrie$MPTException */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "fake_env.h"
#include "khst.h"

jlong Java_khipu_trie_gpu_Khst_changesSince(JNIEnv*, jclass, jlong, jint, jboolean, jint, jbyteArray, jintArray, jbyteArray,
                                            jbyteArray, jbyteArray, jlongArray, jbyteArray, jlongArray);

static void check(JNIEnv* env, const char* name, jsize n_from, jsize n_tries, jsize n_keys, jsize n_next, jsize n_sizes) {
  memset(&fake, 0, sizeof(fake));
  FakeObj* sizes = fake_array(n_sizes, 8, NULL);
  const jlong ret = Java_khipu_trie_gpu_Khst_changesSince(
      env, NULL, 0, 0, 0, 0, n_from ? (jbyteArray)fake_array(n_from, 1, NULL) : NULL,
      n_tries >= 0 ? (jintArray)fake_array(n_tries, 4, NULL) : NULL, (jbyteArray)fake_array(n_keys, 1, NULL),
      (jbyteArray)fake_array(4, 1, NULL), (jbyteArray)fake_array(64, 1, NULL), (jlongArray)fake_array(5, 8, NULL),
      (jbyteArray)fake_array(n_next, 1, NULL), (jlongArray)sizes);
  printf("{\"check\": \"%s\", \"ret\": %lld, \"pending\": %d, \"exc\": \"%s\"}\n", name, (long long)ret, fake.pending,
         fake.exc_class);
}

int main(void) {
  JNIEnv* env = fake_env();
  check(env, "next_short", 0, -1, 128, 31, 5);
  check(env, "sizes_short", 0, -1, 128, 32, 4);
  check(env, "from_short", 31, -1, 128, 32, 5);
  check(env, "no_room", 32, -1, 31, 32, 5);
  check(env, "tries_bound", 32, 0, 128, 32, 5);
  check(env, "null_handle", 32, 4, 128, 32, 5);
  return 0;
}
