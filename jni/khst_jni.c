/*
 * khst_jni.c — the JNI binding of libkhst.so's host-buffer entry points (include/khst.h) for
 * khipu's JVM side, class khipu.trie.gpu.Khst (INTEGRATION.md §3 has the Scala declarations).
 *
 *   cc -std=c99 -shared -fPIC -I$JAVA_HOME/include -I$JAVA_HOME/include/linux -Iinclude \
 *      jni/khst_jni.c -Lkhipu_amd -lkhst -o libkhst_jni.so
 *
 * tests/test_jni_shim.py compiles it against include/khst.h (with a declaration-only jni.h,
 * the image has no JDK) and links it against libkhst.so with --no-undefined, and checks that
 * every host entry point of khst.h has a wrapper here.
 *
 * Conventions:
 *   - no JNI critical region is ever held: a library call may wait for the context's mutex
 *     while another thread's commit runs and then run milliseconds to seconds of GPU work,
 *     and a JVM thread inside GetPrimitiveArrayCritical must not block (HotSpot's GC locker
 *     would stall every allocating thread for that time).  byte[] / int[] / long[] inputs are
 *     copied out with Get<Type>ArrayRegion into malloc'd buffers (one memcpy: ~0.3 ms for a
 *     configs[2] block's ~3 MB) and outputs copied back with Set<Type>ArrayRegion — only the
 *     part the call wrote;
 *   - the large fresh builds (a state root over 100M accounts: ~10 GB of inputs) also take
 *     direct ByteBuffers (the *Direct wrappers): GetDirectBufferAddress, no copy, no pinning by
 *     the JVM; the library stages them over PCIe in pinned chunks, keys first, while the build
 *     runs (khst.h "host inputs");
 *   - a failing call throws: KH_EINVAL -> MerklePatriciaTrie.MPTException; KH_ENODE ->
 *     MerklePatriciaTrie.MPTNodeMissingException(message, hash, storage)
 *     (MerklePatriciaTrie.scala:46-47), built by the Scala factory Khst.nodeMissing(String,
 *     byte[]) that knows the handle's node storage (the case class has no (String)
 *     constructor, and Ledger.scala:511/542 match on its hash and storage); anything else ->
 *     khipu.trie.gpu.DeviceException; the message is kh_last_error();
 *   - KH_ENOSPC (an output array too small) does not throw: the wrapper returns a negative
 *     count or fills the `sizes` array, and the Scala side grows its arrays and calls again;
 *   - resident handles (kh_trie*) are jlongs; free() takes the long[1] the handle lives in and
 *     zeroes it, so a second free (or a finalizer after close) is a no-op, never a double free.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <jni.h>

#include "khst.h"

#define CLS "khipu/trie/gpu/Khst"

/* the class to throw; a missing class leaves its NoClassDefFoundError pending */
static void throw_cls(JNIEnv* env, const char* name, const char* msg) {
  jclass c = (*env)->FindClass(env, name);
  if (c) (*env)->ThrowNew(env, c, msg);
}

/* MPTNodeMissingException for the missing node's hash (32 bytes; zeros if unknown) */
static void throw_node_missing(JNIEnv* env, const uint8_t* hash32) {
  static const uint8_t zero[32] = {0};
  const char* msg = kh_last_error();
  jclass k = (*env)->FindClass(env, CLS);
  if (!k) return;
  jmethodID f = (*env)->GetStaticMethodID(env, k, "nodeMissing", "(Ljava/lang/String;[B)Ljava/lang/Throwable;");
  if (!f) return; /* NoSuchMethodError pending */
  jstring s = (*env)->NewStringUTF(env, msg);
  jbyteArray h = (*env)->NewByteArray(env, 32);
  if (!s || !h) return; /* OutOfMemoryError pending */
  (*env)->SetByteArrayRegion(env, h, 0, 32, (const jbyte*)(hash32 ? hash32 : zero));
  jthrowable t = (jthrowable)(*env)->CallStaticObjectMethod(env, k, f, s, h);
  if ((*env)->ExceptionCheck(env)) return; /* the factory threw: that exception stands */
  if (t) {
    (*env)->Throw(env, t);
    return;
  }
  throw_cls(env, "khipu/trie/gpu/DeviceException", msg);
}

static void throw_kh_hash(JNIEnv* env, int rc, const uint8_t* missing32) {
  if (rc == KH_ENODE) {
    throw_node_missing(env, missing32);
    return;
  }
  if (rc == KH_ENOMEM) {
    throw_cls(env, "java/lang/OutOfMemoryError", kh_last_error());
    return;
  }
  throw_cls(env, rc == KH_EINVAL ? "khipu/trie/MerklePatriciaTrie$MPTException" : "khipu/trie/gpu/DeviceException",
            kh_last_error());
}
static void throw_kh(JNIEnv* env, int rc) { throw_kh_hash(env, rc, NULL); }
/* a refused commit: KH_ENODE carries the first hash of a's missing list, or of b's (kh_trie_missing:
 * a partial handle whose commit walked into a stub; missing() lists them all) */
static void throw_kh_commit(JNIEnv* env, int rc, kh_trie* a, kh_trie* b) {
  if (rc == KH_ENODE) {
    kh_trie* hs[2] = {a, b};
    for (int i = 0; i < 2; ++i) {
      uint64_t n = 0;
      if (!hs[i] || kh_trie_missing(hs[i], NULL, NULL, 0, &n) != KH_ENOSPC || !n) continue;
      uint32_t* t = malloc(4 * (size_t)n);
      uint8_t* h = malloc(32 * (size_t)n);
      const int got = t && h && kh_trie_missing(hs[i], t, h, n, &n) == KH_OK && n;
      uint8_t first[32];
      if (got) memcpy(first, h, 32);
      free(t);
      free(h);
      if (got) { /* (the size query leaves kh_last_error alone: the commit's message is thrown) */
        throw_node_missing(env, first);
        return;
      }
    }
  }
  throw_kh(env, rc);
}

/* ---- host copies of Java arrays (no critical regions) ----
 * A Bufs holds every buffer one wrapper call allocates; bufs_free releases them all.  An input
 * copy of a NULL array is NULL; of an empty one a valid 1-byte allocation.  On allocation
 * failure `oom` is set and the wrapper throws OutOfMemoryError without calling the library. */
typedef struct {
  void* p[24];
  int n;
  int oom;
} Bufs;
static void* bufs_alloc(Bufs* b, size_t bytes) {
  if (b->oom || b->n == 24) {
    b->oom = 1;
    return NULL;
  }
  void* p = malloc(bytes ? bytes : 1);
  if (!p) {
    b->oom = 1;
    return NULL;
  }
  b->p[b->n++] = p;
  return p;
}
static void bufs_free(Bufs* b) {
  for (int i = 0; i < b->n; ++i) free(b->p[i]);
  b->n = 0;
}
/* true (and OutOfMemoryError thrown) when an allocation failed */
static int bufs_failed(JNIEnv* env, Bufs* b) {
  if (!b->oom) return 0;
  bufs_free(b);
  throw_cls(env, "java/lang/OutOfMemoryError", "khst_jni: host copy of the arguments");
  return 1;
}
static jsize len_of(JNIEnv* env, jarray a) { return a ? (*env)->GetArrayLength(env, a) : 0; }
static const uint8_t* in_b(JNIEnv* env, Bufs* b, jbyteArray a) {
  if (!a) return NULL;
  const jsize n = len_of(env, a);
  jbyte* p = bufs_alloc(b, (size_t)n);
  if (p && n) (*env)->GetByteArrayRegion(env, a, 0, n, p);
  return (const uint8_t*)p;
}
static const uint32_t* in_i(JNIEnv* env, Bufs* b, jintArray a) {
  if (!a) return NULL;
  const jsize n = len_of(env, a);
  jint* p = bufs_alloc(b, 4 * (size_t)n);
  if (p && n) (*env)->GetIntArrayRegion(env, a, 0, n, p);
  return (const uint32_t*)p;
}
static const uint64_t* in_l(JNIEnv* env, Bufs* b, jlongArray a) {
  if (!a) return NULL;
  const jsize n = len_of(env, a);
  jlong* p = bufs_alloc(b, 8 * (size_t)n);
  if (p && n) (*env)->GetLongArrayRegion(env, a, 0, n, p);
  return (const uint64_t*)p;
}
/* an output buffer the size of array a (NULL array: NULL) */
static void* out_buf(JNIEnv* env, Bufs* b, jarray a, size_t esz) {
  return a ? bufs_alloc(b, esz * (size_t)len_of(env, a)) : NULL;
}
/* copy the first n elements of an output buffer back (clamped to the array) */
static void put_b(JNIEnv* env, jbyteArray a, const void* p, uint64_t n) {
  const jsize L = len_of(env, a);
  if (a && p && n) (*env)->SetByteArrayRegion(env, a, 0, n < (uint64_t)L ? (jsize)n : L, (const jbyte*)p);
}
static void put_i(JNIEnv* env, jintArray a, const void* p, uint64_t n) {
  const jsize L = len_of(env, a);
  if (a && p && n) (*env)->SetIntArrayRegion(env, a, 0, n < (uint64_t)L ? (jsize)n : L, (const jint*)p);
}
static void put_l(JNIEnv* env, jlongArray a, const void* p, uint64_t n) {
  const jsize L = len_of(env, a);
  if (a && p && n) (*env)->SetLongArrayRegion(env, a, 0, n < (uint64_t)L ? (jsize)n : L, (const jlong*)p);
}

/* entries of an offsets array (n + 1 offsets -> n items; NULL or empty -> 0) */
static uint64_t count_of(JNIEnv* env, jlongArray off) {
  const jsize n = len_of(env, off);
  return n > 0 ? (uint64_t)(n - 1) : 0;
}
static jbyteArray bytes_of(JNIEnv* env, const uint8_t* p, jsize n) {
  jbyteArray out = (*env)->NewByteArray(env, n);
  if (out) (*env)->SetByteArrayRegion(env, out, 0, n, (const jbyte*)p);
  return out;
}
static kh_trie* H(jlong h) { return (kh_trie*)(intptr_t)h; }
/* kh_stats -> long[] statsOut (nullable): n_inputs, n_leaves, n_branches, n_extensions, n_inline,
 * n_node_hashes, n_node_perms, n_key_perms, arena_bytes, n_levels, full_sort */
static void put_stats(JNIEnv* env, jlongArray out, const kh_stats* s) {
  if (!out) return;
  const jlong v[11] = {(jlong)s->n_inputs,      (jlong)s->n_leaves,     (jlong)s->n_branches, (jlong)s->n_extensions,
                       (jlong)s->n_inline,      (jlong)s->n_node_hashes, (jlong)s->n_node_perms,
                       (jlong)s->n_key_perms,   (jlong)s->arena_bytes,  (jlong)s->n_levels,   (jlong)s->full_sort};
  put_l(env, out, v, 11);
}

/* ---- direct ByteBuffers (the *Direct wrappers): the address, or NULL with an
 * IllegalArgumentException pending when the buffer is not direct or holds fewer than `need`
 * bytes (a NULL buffer is allowed when need == 0) */
static void* direct(JNIEnv* env, jobject buf, uint64_t need, const char* what) {
  if (!buf) {
    if (need) throw_cls(env, "java/lang/IllegalArgumentException", what);
    return NULL;
  }
  void* p = (*env)->GetDirectBufferAddress(env, buf);
  const jlong cap = (*env)->GetDirectBufferCapacity(env, buf);
  if (!p || cap < 0 || (uint64_t)cap < need) {
    throw_cls(env, "java/lang/IllegalArgumentException", what);
    return NULL;
  }
  return p;
}
/* the keys / value offsets / values of n inputs in direct buffers, capacities checked */
typedef struct {
  const uint8_t* keys;
  const uint64_t* voff;
  const uint8_t* vals;
} DirectIn;
static int direct_inputs(JNIEnv* env, jobject keys, jint klen, jobject vals, jobject voff, jlong n, DirectIn* in) {
  if (n < 0 || klen < 0) {
    throw_cls(env, "java/lang/IllegalArgumentException", "negative count or key length");
    return 0;
  }
  in->keys = direct(env, keys, (uint64_t)n * (uint64_t)klen, "keys: not a direct buffer of n * klen bytes");
  if ((*env)->ExceptionCheck(env)) return 0;
  in->voff = direct(env, voff, 8 * ((uint64_t)n + 1), "voff: not a direct buffer of n + 1 longs (native order)");
  if ((*env)->ExceptionCheck(env)) return 0;
  const uint64_t vend = n ? in->voff[n] : 0;
  if (n && in->voff[n] < in->voff[0]) {
    throw_cls(env, "java/lang/IllegalArgumentException", "voff: not monotone");
    return 0;
  }
  in->vals = direct(env, vals, vend, "vals: not a direct buffer of voff[n] bytes");
  return !(*env)->ExceptionCheck(env);
}

/* ---- library ---- */
JNIEXPORT jbyteArray JNICALL Java_khipu_trie_gpu_Khst_version(JNIEnv* env, jclass cls) {
  (void)cls;
  const char* v = kh_version();
  return bytes_of(env, (const uint8_t*)v, (jsize)strlen(v));
}
JNIEXPORT jint JNICALL Java_khipu_trie_gpu_Khst_deviceCount(JNIEnv* env, jclass cls) {
  (void)env, (void)cls;
  return kh_device_count();
}

/* ---- crypto.kec256 over a batch (crypto/package.scala:37-47): messages data[off[i]..off[i+1]) */
JNIEXPORT jbyteArray JNICALL Java_khipu_trie_gpu_Khst_kec256Batch(JNIEnv* env, jclass cls, jbyteArray data,
                                                                 jlongArray off) {
  (void)cls;
  const uint64_t n = count_of(env, off);
  Bufs b = {0};
  const uint8_t* d = in_b(env, &b, data);
  const uint64_t* o = in_l(env, &b, off);
  uint8_t* r = bufs_alloc(&b, 32 * (size_t)n);
  if (bufs_failed(env, &b)) return NULL;
  const int rc = kh_kec256_batch(d, o, n, r);
  jbyteArray out = rc == KH_OK ? bytes_of(env, r, (jsize)(32 * n)) : NULL;
  bufs_free(&b);
  if (rc != KH_OK) throw_kh(env, rc);
  return out;
}

/* ---- fresh tries (TrieAccounts.flush / TrieStorage.flush / GenesisDataLoader) ---- */
/* keys: n*klen bytes, vals packed with voff (n+1 offsets); returns the root */
JNIEXPORT jbyteArray JNICALL Java_khipu_trie_gpu_Khst_trieRoot(JNIEnv* env, jclass cls, jbyteArray keys, jint klen,
                                                              jbyteArray vals, jlongArray voff, jint flags,
                                                              jlongArray statsOut) {
  (void)cls;
  const uint64_t n = count_of(env, voff);
  uint8_t root[32];
  kh_stats st;
  Bufs b = {0};
  const uint8_t* k = in_b(env, &b, keys);
  const uint8_t* v = in_b(env, &b, vals);
  const uint64_t* o = in_l(env, &b, voff);
  if (bufs_failed(env, &b)) return NULL;
  const int rc = kh_trie_root(k, (uint32_t)klen, v, o, n, (uint32_t)flags, root, &st);
  bufs_free(&b);
  if (rc != KH_OK) {
    throw_kh(env, rc);
    return NULL;
  }
  put_stats(env, statsOut, &st);
  return bytes_of(env, root, 32);
}

/* the same over direct buffers (keys: n*klen bytes, voff: n+1 native-order longs, vals:
 * voff[n] bytes): no copy on the JVM side; the library stages the inputs over PCIe while the
 * build runs */
JNIEXPORT jbyteArray JNICALL Java_khipu_trie_gpu_Khst_trieRootDirect(JNIEnv* env, jclass cls, jobject keys, jint klen,
                                                                    jobject vals, jobject voff, jlong n, jint flags,
                                                                    jlongArray statsOut) {
  (void)cls;
  DirectIn in;
  if (!direct_inputs(env, keys, klen, vals, voff, n, &in)) return NULL;
  uint8_t root[32];
  kh_stats st;
  const int rc = kh_trie_root(in.keys, (uint32_t)klen, in.vals, in.voff, (uint64_t)n, (uint32_t)flags, root, &st);
  if (rc != KH_OK) {
    throw_kh(env, rc);
    return NULL;
  }
  put_stats(env, statsOut, &st);
  return bytes_of(env, root, 32);
}

/* nseg tries (segOff: nseg+1 input offsets); returns nseg*32 bytes of roots */
JNIEXPORT jbyteArray JNICALL Java_khipu_trie_gpu_Khst_trieRootsSegmented(JNIEnv* env, jclass cls, jbyteArray keys,
                                                                        jint klen, jbyteArray vals, jlongArray voff,
                                                                        jlongArray segOff, jint flags) {
  (void)cls;
  const uint64_t nseg = count_of(env, segOff);
  Bufs b = {0};
  const uint8_t* k = in_b(env, &b, keys);
  const uint8_t* v = in_b(env, &b, vals);
  const uint64_t* o = in_l(env, &b, voff);
  const uint64_t* so = in_l(env, &b, segOff);
  uint8_t* r = bufs_alloc(&b, 32 * (size_t)nseg);
  if (bufs_failed(env, &b)) return NULL;
  const int rc = kh_trie_roots_segmented(k, (uint32_t)klen, v, o, so, nseg, (uint32_t)flags, r, NULL);
  jbyteArray out = rc == KH_OK ? bytes_of(env, r, (jsize)(32 * nseg)) : NULL;
  bufs_free(&b);
  if (rc != KH_OK) throw_kh(env, rc);
  return out;
}

/* the same over the listed devices of this JVM (contiguous trie ranges, no exchange) */
JNIEXPORT jbyteArray JNICALL Java_khipu_trie_gpu_Khst_trieRootsSegmentedSharded(
    JNIEnv* env, jclass cls, jintArray devices, jbyteArray keys, jint klen, jbyteArray vals, jlongArray voff,
    jlongArray segOff, jint flags) {
  (void)cls;
  const uint64_t nseg = count_of(env, segOff);
  const jsize ng = len_of(env, devices);
  Bufs b = {0};
  const uint32_t* d = in_i(env, &b, devices);
  const uint8_t* k = in_b(env, &b, keys);
  const uint8_t* v = in_b(env, &b, vals);
  const uint64_t* o = in_l(env, &b, voff);
  const uint64_t* so = in_l(env, &b, segOff);
  uint8_t* r = bufs_alloc(&b, 32 * (size_t)nseg);
  if (bufs_failed(env, &b)) return NULL;
  const int rc =
      kh_trie_roots_segmented_sharded((const int*)d, (int)ng, k, (uint32_t)klen, v, o, so, nseg, (uint32_t)flags, r, NULL);
  jbyteArray out = rc == KH_OK ? bytes_of(env, r, (jsize)(32 * nseg)) : NULL;
  bufs_free(&b);
  if (rc != KH_OK) throw_kh(env, rc);
  return out;
}

/* variable-length unhashed keys (keys[koff[i]..koff[i+1]), 0..32 bytes); nseg tries */
JNIEXPORT jbyteArray JNICALL Java_khipu_trie_gpu_Khst_trieRootsVarkeys(JNIEnv* env, jclass cls, jbyteArray keys,
                                                                      jlongArray koff, jbyteArray vals,
                                                                      jlongArray voff, jlongArray segOff) {
  (void)cls;
  const uint64_t nseg = count_of(env, segOff);
  Bufs b = {0};
  const uint8_t* k = in_b(env, &b, keys);
  const uint64_t* ko = in_l(env, &b, koff);
  const uint8_t* v = in_b(env, &b, vals);
  const uint64_t* o = in_l(env, &b, voff);
  const uint64_t* so = in_l(env, &b, segOff);
  uint8_t* r = bufs_alloc(&b, 32 * (size_t)nseg);
  if (bufs_failed(env, &b)) return NULL;
  const int rc = kh_trie_roots_varkeys(k, ko, v, o, so, nseg, r, NULL);
  jbyteArray out = rc == KH_OK ? bytes_of(env, r, (jsize)(32 * nseg)) : NULL;
  bufs_free(&b);
  if (rc != KH_OK) throw_kh(env, rc);
  return out;
}

/* every block's transactions (or receipts) root in one call (MptListValidator.scala:15-46) */
JNIEXPORT jbyteArray JNICALL Java_khipu_trie_gpu_Khst_listRoots(JNIEnv* env, jclass cls, jbyteArray items,
                                                               jlongArray off, jlongArray segOff) {
  (void)cls;
  const uint64_t nseg = count_of(env, segOff);
  Bufs b = {0};
  const uint8_t* it = in_b(env, &b, items);
  const uint64_t* o = in_l(env, &b, off);
  const uint64_t* so = in_l(env, &b, segOff);
  uint8_t* r = bufs_alloc(&b, 32 * (size_t)nseg);
  if (bufs_failed(env, &b)) return NULL;
  const int rc = kh_list_roots(it, o, so, nseg, r, NULL);
  jbyteArray out = rc == KH_OK ? bytes_of(env, r, (jsize)(32 * nseg)) : NULL;
  bufs_free(&b);
  if (rc != KH_OK) throw_kh(env, rc);
  return out;
}

/* the root on several GPUs of this JVM (nibble shards, RCCL point-to-point exchange) */
JNIEXPORT jbyteArray JNICALL Java_khipu_trie_gpu_Khst_trieRootSharded(JNIEnv* env, jclass cls, jintArray devices,
                                                                     jbyteArray keys, jint klen, jbyteArray vals,
                                                                     jlongArray voff, jint flags) {
  (void)cls;
  const uint64_t n = count_of(env, voff);
  const jsize ng = len_of(env, devices);
  uint8_t root[32];
  Bufs b = {0};
  const uint32_t* d = in_i(env, &b, devices);
  const uint8_t* k = in_b(env, &b, keys);
  const uint8_t* v = in_b(env, &b, vals);
  const uint64_t* o = in_l(env, &b, voff);
  if (bufs_failed(env, &b)) return NULL;
  const int rc = kh_trie_root_sharded((const int*)d, (int)ng, k, (uint32_t)klen, v, o, n, (uint32_t)flags, root, NULL);
  bufs_free(&b);
  if (rc != KH_OK) {
    throw_kh(env, rc);
    return NULL;
  }
  return bytes_of(env, root, 32);
}

/* the same over direct buffers (as trieRootDirect) */
JNIEXPORT jbyteArray JNICALL Java_khipu_trie_gpu_Khst_trieRootShardedDirect(JNIEnv* env, jclass cls, jintArray devices,
                                                                           jobject keys, jint klen, jobject vals,
                                                                           jobject voff, jlong n, jint flags) {
  (void)cls;
  DirectIn in;
  if (!direct_inputs(env, keys, klen, vals, voff, n, &in)) return NULL;
  const jsize ng = len_of(env, devices);
  uint8_t root[32];
  Bufs b = {0};
  const uint32_t* d = in_i(env, &b, devices);
  if (bufs_failed(env, &b)) return NULL;
  const int rc = kh_trie_root_sharded((const int*)d, (int)ng, in.keys, (uint32_t)klen, in.vals, in.voff, (uint64_t)n,
                                      (uint32_t)flags, root, NULL);
  bufs_free(&b);
  if (rc != KH_OK) {
    throw_kh(env, rc);
    return NULL;
  }
  return bytes_of(env, root, 32);
}

/* Root + the node set a fresh store needs (GenesisDataLoader.scala:139-147, persist of a fresh
 * trie): the caller's hashes (32 per node), rlp and off (n_nodes + 1) arrays receive the nodes;
 * sizes[0] / sizes[1] = nodes / RLP bytes.  Returns the root, or NULL when an output array is
 * too small (sizes then hold what is needed: grow and call again). */
JNIEXPORT jbyteArray JNICALL Java_khipu_trie_gpu_Khst_trieRootNodes(JNIEnv* env, jclass cls, jbyteArray keys,
                                                                   jint klen, jbyteArray vals, jlongArray voff,
                                                                   jint flags, jbyteArray hashes, jbyteArray rlp,
                                                                   jlongArray off, jlongArray sizes) {
  (void)cls;
  const uint64_t n = count_of(env, voff);
  const uint64_t node_cap = (uint64_t)len_of(env, hashes) / 32, rlp_cap = (uint64_t)len_of(env, rlp);
  const jsize noff = len_of(env, off);
  const uint64_t cap = node_cap < (uint64_t)(noff > 0 ? noff - 1 : 0) ? node_cap : (uint64_t)(noff > 0 ? noff - 1 : 0);
  uint8_t root[32];
  uint64_t nn = 0, nb = 0;
  Bufs b = {0};
  const uint8_t* k = in_b(env, &b, keys);
  const uint8_t* v = in_b(env, &b, vals);
  const uint64_t* o = in_l(env, &b, voff);
  uint8_t* hs = out_buf(env, &b, hashes, 1);
  uint8_t* rl = out_buf(env, &b, rlp, 1);
  uint64_t* of = out_buf(env, &b, off, 8);
  if (bufs_failed(env, &b)) return NULL;
  const int rc = kh_trie_root_nodes(k, (uint32_t)klen, v, o, n, (uint32_t)flags, root, hs, cap, rl, rlp_cap, of, &nn,
                                    &nb, NULL);
  if (rc == KH_OK) {
    put_b(env, hashes, hs, 32 * nn);
    put_b(env, rlp, rl, nb);
    put_l(env, off, of, nn + 1);
  }
  bufs_free(&b);
  const jlong sz[2] = {(jlong)nn, (jlong)nb};
  put_l(env, sizes, sz, 2);
  if (rc == KH_ENOSPC) return NULL;
  if (rc != KH_OK) {
    throw_kh(env, rc);
    return NULL;
  }
  return bytes_of(env, root, 32);
}

/* the same over direct buffers: inputs as trieRootDirect; outputs hashes (32 per node), rlp and
 * off (n_nodes + 1 native-order longs) are direct buffers too, written in place (a 100M-account
 * state's node set is ~20 GB: no Java array holds it) */
JNIEXPORT jbyteArray JNICALL Java_khipu_trie_gpu_Khst_trieRootNodesDirect(JNIEnv* env, jclass cls, jobject keys,
                                                                         jint klen, jobject vals, jobject voff, jlong n,
                                                                         jint flags, jobject hashes, jobject rlp,
                                                                         jobject off, jlongArray sizes) {
  (void)cls;
  DirectIn in;
  if (!direct_inputs(env, keys, klen, vals, voff, n, &in)) return NULL;
  uint8_t* hs = direct(env, hashes, 0, "hashes: not a direct buffer");
  uint8_t* rl = (*env)->ExceptionCheck(env) ? NULL : direct(env, rlp, 0, "rlp: not a direct buffer");
  uint64_t* of = (*env)->ExceptionCheck(env) ? NULL : direct(env, off, 0, "off: not a direct buffer");
  if ((*env)->ExceptionCheck(env)) return NULL;
  const jlong hcap = hashes ? (*env)->GetDirectBufferCapacity(env, hashes) : 0;
  const jlong rcap = rlp ? (*env)->GetDirectBufferCapacity(env, rlp) : 0;
  const jlong ocap = off ? (*env)->GetDirectBufferCapacity(env, off) : 0;
  const uint64_t node_cap = (uint64_t)hcap / 32, ocount = ocap >= 8 ? (uint64_t)ocap / 8 - 1 : 0;
  const uint64_t cap = node_cap < ocount ? node_cap : ocount;
  uint8_t root[32];
  uint64_t nn = 0, nb = 0;
  const int rc = kh_trie_root_nodes(in.keys, (uint32_t)klen, in.vals, in.voff, (uint64_t)n, (uint32_t)flags, root, hs,
                                    cap, rl, (uint64_t)rcap, of, &nn, &nb, NULL);
  const jlong sz[2] = {(jlong)nn, (jlong)nb};
  put_l(env, sizes, sz, 2);
  if (rc == KH_ENOSPC) return NULL;
  if (rc != KH_OK) {
    throw_kh(env, rc);
    return NULL;
  }
  return bytes_of(env, root, 32);
}

/* ---- fast sync: NodeDatasRequest.processResponse (sync/package.scala:81-165) ---- */
/* per value: hash32 (32 each), match (-1: none), status; nchild (per value) and the children
 * 16 slots per value (child32: 512 bytes, childKind: 16 per value) */
JNIEXPORT void JNICALL Java_khipu_trie_gpu_Khst_verifyNodes(JNIEnv* env, jclass cls, jbyteArray data, jlongArray off,
                                                           jbyteArray req32, jbyteArray reqKind, jbyteArray hash32,
                                                           jlongArray match, jbyteArray status, jbyteArray nchild,
                                                           jbyteArray child32, jbyteArray childKind) {
  (void)cls;
  const uint64_t n = count_of(env, off), nreq = (uint64_t)len_of(env, reqKind);
  Bufs b = {0};
  const uint8_t* dt = in_b(env, &b, data);
  const uint64_t* o = in_l(env, &b, off);
  const uint8_t* rq = in_b(env, &b, req32);
  const uint8_t* rk = in_b(env, &b, reqKind);
  uint8_t* hs = out_buf(env, &b, hash32, 1);
  int64_t* mt = out_buf(env, &b, match, 8);
  uint8_t* stt = out_buf(env, &b, status, 1);
  uint8_t* nc = out_buf(env, &b, nchild, 1);
  uint8_t* c32 = out_buf(env, &b, child32, 1);
  uint8_t* ck = out_buf(env, &b, childKind, 1);
  if (bufs_failed(env, &b)) return;
  const int rc = kh_verify_nodes(dt, o, n, rq, rk, nreq, hs, mt, stt, nc, c32, ck);
  if (rc == KH_OK) {
    put_b(env, hash32, hs, 32 * n);
    put_l(env, match, mt, n);
    put_b(env, status, stt, n);
    put_b(env, nchild, nc, n);
    put_b(env, child32, c32, 512 * n);
    put_b(env, childKind, ck, 16 * n);
  }
  bufs_free(&b);
  if (rc != KH_OK) throw_kh(env, rc);
}

/* the same with the children packed as processResponse concatenates them (childOff: n+1);
 * returns the number of children, or its negation when child32 / childKind are too small
 * (every other output is written: grow and call again) */
JNIEXPORT jlong JNICALL Java_khipu_trie_gpu_Khst_verifyNodesPacked(JNIEnv* env, jclass cls, jbyteArray data,
                                                                  jlongArray off, jbyteArray req32, jbyteArray reqKind,
                                                                  jlongArray match, jbyteArray status,
                                                                  jlongArray childOff, jbyteArray child32,
                                                                  jbyteArray childKind) {
  (void)cls;
  const uint64_t n = count_of(env, off), nreq = (uint64_t)len_of(env, reqKind);
  const uint64_t cap = (uint64_t)len_of(env, childKind);
  uint64_t nch = 0;
  Bufs b = {0};
  const uint8_t* dt = in_b(env, &b, data);
  const uint64_t* o = in_l(env, &b, off);
  const uint8_t* rq = in_b(env, &b, req32);
  const uint8_t* rk = in_b(env, &b, reqKind);
  uint8_t* hashes = bufs_alloc(&b, 32 * (size_t)n);
  int64_t* mt = out_buf(env, &b, match, 8);
  uint8_t* stt = out_buf(env, &b, status, 1);
  uint64_t* co = out_buf(env, &b, childOff, 8);
  uint8_t* c32 = out_buf(env, &b, child32, 1);
  uint8_t* ck = out_buf(env, &b, childKind, 1);
  if (bufs_failed(env, &b)) return 0;
  const int rc = kh_verify_nodes_packed(dt, o, n, rq, rk, nreq, hashes, mt, stt, co, c32, ck, cap, &nch);
  if (rc == KH_OK || rc == KH_ENOSPC) {
    put_l(env, match, mt, n);
    put_b(env, status, stt, n);
    put_l(env, childOff, co, n + 1);
  }
  if (rc == KH_OK) {
    put_b(env, child32, c32, 32 * nch);
    put_b(env, childKind, ck, nch);
  }
  bufs_free(&b);
  if (rc == KH_ENOSPC) return -(jlong)nch;
  if (rc != KH_OK) {
    throw_kh(env, rc);
    return 0;
  }
  return (jlong)nch;
}

/* ---- resident tries (BlockWorldState / TrieAccounts / TrieStorage over a live state) ---- */
/* open from records (flags: HASH_KEYS, EMIT_NODES); rootOut (byte[32], nullable) gets the root */
JNIEXPORT jlong JNICALL Java_khipu_trie_gpu_Khst_openHost(JNIEnv* env, jclass cls, jbyteArray keys, jint klen,
                                                         jbyteArray vals, jlongArray voff, jint flags,
                                                         jbyteArray rootOut) {
  (void)cls;
  const uint64_t n = count_of(env, voff);
  uint8_t root[32];
  kh_trie* h = NULL;
  Bufs b = {0};
  const uint8_t* k = in_b(env, &b, keys);
  const uint8_t* v = in_b(env, &b, vals);
  const uint64_t* o = in_l(env, &b, voff);
  if (bufs_failed(env, &b)) return 0;
  const int rc = kh_trie_open_host(k, (uint32_t)klen, v, o, n, (uint32_t)flags, root, &h);
  bufs_free(&b);
  if (rc != KH_OK) {
    throw_kh(env, rc);
    return 0;
  }
  put_b(env, rootOut, root, 32);
  return (jlong)(intptr_t)h;
}

/* the same over direct buffers (as trieRootDirect): a 50M-account state opened without a copy */
JNIEXPORT jlong JNICALL Java_khipu_trie_gpu_Khst_openHostDirect(JNIEnv* env, jclass cls, jobject keys, jint klen,
                                                               jobject vals, jobject voff, jlong n, jint flags,
                                                               jbyteArray rootOut) {
  (void)cls;
  DirectIn in;
  if (!direct_inputs(env, keys, klen, vals, voff, n, &in)) return 0;
  uint8_t root[32];
  kh_trie* h = NULL;
  const int rc = kh_trie_open_host(in.keys, (uint32_t)klen, in.vals, in.voff, (uint64_t)n, (uint32_t)flags, root, &h);
  if (rc != KH_OK) {
    throw_kh(env, rc);
    return 0;
  }
  put_b(env, rootOut, root, 32);
  return (jlong)(intptr_t)h;
}

/* MerklePatriciaTrie.apply(rootHash, source) (MerklePatriciaTrie.scala:60-66): open from a node
 * store (encodings enc[off[i]..off[i+1]), content addressed); a missing node throws
 * MPTNodeMissingException (with its hash) after writing the hash into missingOut (byte[32],
 * nullable) */
JNIEXPORT jlong JNICALL Java_khipu_trie_gpu_Khst_openNodes(JNIEnv* env, jclass cls, jbyteArray root32,
                                                          jbyteArray enc, jlongArray off, jint flags,
                                                          jbyteArray missingOut) {
  (void)cls;
  const uint64_t n = count_of(env, off);
  uint8_t missing[32] = {0};
  kh_trie* h = NULL;
  Bufs b = {0};
  const uint8_t* r = in_b(env, &b, root32);
  const uint8_t* e = in_b(env, &b, enc);
  const uint64_t* o = in_l(env, &b, off);
  if (bufs_failed(env, &b)) return 0;
  if (!r || len_of(env, root32) < 32) {
    bufs_free(&b);
    throw_cls(env, "java/lang/IllegalArgumentException", "root32: 32 bytes");
    return 0;
  }
  const int rc = kh_trie_open_nodes_host(r, e, o, n, (uint32_t)flags, missing, &h);
  bufs_free(&b);
  if (rc == KH_ENODE) put_b(env, missingOut, missing, 32);
  if (rc != KH_OK) {
    throw_kh_hash(env, rc, missing);
    return 0;
  }
  return (jlong)(intptr_t)h;
}

/* one commit (upserts then deletes) on a single trie; returns the new root */
JNIEXPORT jbyteArray JNICALL Java_khipu_trie_gpu_Khst_apply(JNIEnv* env, jclass cls, jlong handle, jbyteArray upKeys,
                                                           jbyteArray upVals, jlongArray upVoff, jbyteArray delKeys,
                                                           jint klen, jint flags, jlongArray statsOut) {
  (void)cls;
  const uint64_t nup = count_of(env, upVoff), ndel = klen > 0 ? (uint64_t)(len_of(env, delKeys) / klen) : 0;
  uint8_t root[32];
  kh_stats st;
  Bufs b = {0};
  const uint8_t* k = in_b(env, &b, upKeys);
  const uint8_t* v = in_b(env, &b, upVals);
  const uint64_t* o = in_l(env, &b, upVoff);
  const uint8_t* d = in_b(env, &b, delKeys);
  if (bufs_failed(env, &b)) return NULL;
  const int rc = kh_trie_apply_host(H(handle), k, v, o, nup, d, ndel, (uint32_t)klen, (uint32_t)flags, root, &st);
  bufs_free(&b);
  if (rc != KH_OK) {
    throw_kh_commit(env, rc, H(handle), NULL);
    return NULL;
  }
  put_stats(env, statsOut, &st);
  return bytes_of(env, root, 32);
}

/* a forest of tries (contract storage) on the host entry points' context */
JNIEXPORT jlong JNICALL Java_khipu_trie_gpu_Khst_forestOpen(JNIEnv* env, jclass cls, jint flags) {
  (void)cls;
  kh_trie* h = NULL;
  const int rc = kh_forest_open(NULL, (uint32_t)flags, &h);
  if (rc != KH_OK) {
    throw_kh(env, rc);
    return 0;
  }
  return (jlong)(intptr_t)h;
}

/* one commit of many tries' ops (each op names its trie); triesOut / rootsOut receive the
 * touched tries and their new roots; returns their number (negated: the outputs were short) */
JNIEXPORT jlong JNICALL Java_khipu_trie_gpu_Khst_forestApply(JNIEnv* env, jclass cls, jlong handle, jintArray upTrie,
                                                            jbyteArray upKeys, jbyteArray upVals, jlongArray upVoff,
                                                            jintArray delTrie, jbyteArray delKeys, jint klen,
                                                            jintArray triesOut, jbyteArray rootsOut) {
  (void)cls;
  const uint64_t nup = count_of(env, upVoff), ndel = (uint64_t)len_of(env, delTrie);
  const jsize tcap = len_of(env, triesOut), rcap = len_of(env, rootsOut) / 32;
  const uint64_t cap = (uint64_t)(tcap < rcap ? tcap : rcap);
  uint64_t nt = 0;
  Bufs b = {0};
  const uint32_t* ut = in_i(env, &b, upTrie);
  const uint8_t* k = in_b(env, &b, upKeys);
  const uint8_t* v = in_b(env, &b, upVals);
  const uint64_t* o = in_l(env, &b, upVoff);
  const uint32_t* dt = in_i(env, &b, delTrie);
  const uint8_t* d = in_b(env, &b, delKeys);
  uint32_t* to = out_buf(env, &b, triesOut, 4);
  uint8_t* ro = out_buf(env, &b, rootsOut, 1);
  if (bufs_failed(env, &b)) return 0;
  const int rc = kh_forest_apply_host(H(handle), ut, k, v, o, nup, dt, d, ndel, (uint32_t)klen, to, ro, cap, &nt, NULL);
  if (rc == KH_OK) {
    put_i(env, triesOut, to, nt);
    put_b(env, rootsOut, ro, 32 * nt);
  }
  bufs_free(&b);
  if (rc == KH_ENOSPC) return -(jlong)nt; /* committed; kh_forest_last_roots reads them again */
  if (rc != KH_OK) {
    throw_kh_commit(env, rc, H(handle), NULL);
    return 0;
  }
  return (jlong)nt;
}

/* the last commit's touched tries and roots (after a short forestApply, or a rollback) */
JNIEXPORT jlong JNICALL Java_khipu_trie_gpu_Khst_forestLastRoots(JNIEnv* env, jclass cls, jlong handle,
                                                                jintArray triesOut, jbyteArray rootsOut) {
  (void)cls;
  const jsize tcap = len_of(env, triesOut), rcap = len_of(env, rootsOut) / 32;
  const uint64_t cap = (uint64_t)(tcap < rcap ? tcap : rcap);
  uint64_t nt = 0;
  Bufs b = {0};
  uint32_t* to = out_buf(env, &b, triesOut, 4);
  uint8_t* ro = out_buf(env, &b, rootsOut, 1);
  if (bufs_failed(env, &b)) return 0;
  const int rc = kh_forest_last_roots(H(handle), to, ro, cap, &nt);
  if (rc == KH_OK) {
    put_i(env, triesOut, to, nt);
    put_b(env, rootsOut, ro, 32 * nt);
  }
  bufs_free(&b);
  if (rc == KH_ENOSPC) return -(jlong)nt;
  if (rc != KH_OK) {
    throw_kh(env, rc);
    return 0;
  }
  return (jlong)nt;
}

/* Page storage tries into a forest (MerklePatriciaTrie(account.stateRoot, storageSource) per
 * contract, batched): tries[j] with root roots[32j..) decoded from the node store enc / off (as
 * openNodes).  All or nothing.  Nodes missing from the store: missIdxOut / missOut (nullable)
 * receive the list index and hash of every missing reference of the round that stopped the walk
 * (as many as fit), nMissingOut[0] (long[1], nullable) their number, and
 * MPTNodeMissingException is thrown with the first listed hash.  dEnc != 0: the store is in HBM
 * (device addresses of the encodings and the n + 1 offsets, on the forest's context). */
static void forest_load(JNIEnv* env, jlong handle, jintArray tries, jbyteArray roots, jbyteArray enc, jlongArray off,
                        jlong dEnc, jlong dOff, jlong dN, jintArray missIdxOut, jbyteArray missOut,
                        jlongArray nMissingOut, int partial) {
  const uint64_t k = (uint64_t)len_of(env, tries);
  const jsize icap = len_of(env, missIdxOut), hcap = len_of(env, missOut) / 32;
  const uint64_t cap = (uint64_t)(icap < hcap ? icap : hcap);
  uint64_t nm = 0;
  Bufs b = {0};
  const uint32_t* t = in_i(env, &b, tries);
  const uint8_t* r = in_b(env, &b, roots);
  const uint8_t* e = dEnc ? NULL : in_b(env, &b, enc);
  const uint64_t* o = dEnc ? NULL : in_l(env, &b, off);
  uint32_t* mi = bufs_alloc(&b, 4 * (size_t)(cap ? cap : 1));
  uint8_t* mh = bufs_alloc(&b, 32 * (size_t)(cap ? cap : 1));
  if (bufs_failed(env, &b)) return;
  if ((uint64_t)len_of(env, roots) < 32 * k) {
    bufs_free(&b);
    throw_cls(env, "java/lang/IllegalArgumentException", "roots: 32 bytes per listed trie");
    return;
  }
  if (cap) memset(mh, 0, 32);
  int rc;
  if (partial)
    rc = dEnc ? kh_forest_load_partial(H(handle), t, r, k, (const uint8_t*)(intptr_t)dEnc,
                                       (const uint64_t*)(intptr_t)dOff, (uint64_t)dN, mi, mh, cap, &nm, NULL)
              : kh_forest_load_partial_host(H(handle), t, r, k, e, o, count_of(env, off), mi, mh, cap, &nm, NULL);
  else
    rc = dEnc ? kh_forest_load_nodes(H(handle), t, r, k, (const uint8_t*)(intptr_t)dEnc,
                                     (const uint64_t*)(intptr_t)dOff, (uint64_t)dN, mi, mh, cap, &nm, NULL)
              : kh_forest_load_nodes_host(H(handle), t, r, k, e, o, count_of(env, off), mi, mh, cap, &nm, NULL);
  if (rc == KH_ENODE) {
    const uint64_t w = nm < cap ? nm : cap;
    const jlong n64 = (jlong)nm;
    put_i(env, missIdxOut, mi, w);
    put_b(env, missOut, mh, 32 * w);
    put_l(env, nMissingOut, &n64, 1);
  }
  if (rc != KH_OK) throw_kh_hash(env, rc, cap && nm ? mh : NULL);
  bufs_free(&b);
}
JNIEXPORT void JNICALL Java_khipu_trie_gpu_Khst_forestLoadNodes(JNIEnv* env, jclass cls, jlong handle, jintArray tries,
                                                               jbyteArray roots, jbyteArray enc, jlongArray off,
                                                               jintArray missIdxOut, jbyteArray missOut,
                                                               jlongArray nMissingOut) {
  (void)cls;
  forest_load(env, handle, tries, roots, enc, off, 0, 0, 0, missIdxOut, missOut, nMissingOut, 0);
}
JNIEXPORT void JNICALL Java_khipu_trie_gpu_Khst_forestLoadNodesDevice(JNIEnv* env, jclass cls, jlong handle,
                                                                     jintArray tries, jbyteArray roots, jlong dEnc,
                                                                     jlong dOff, jlong n, jintArray missIdxOut,
                                                                     jbyteArray missOut, jlongArray nMissingOut) {
  (void)cls;
  if (!dEnc || !dOff) {
    throw_cls(env, "java/lang/IllegalArgumentException", "dEnc / dOff: device addresses");
    return;
  }
  forest_load(env, handle, tries, roots, NULL, NULL, dEnc, dOff, n, missIdxOut, missOut, nMissingOut, 0);
}

/* ---- partial handles: open from a witness, fill what a commit misses ----
 * The lazy getNode of MerklePatriciaTrie(rootHash, source) (MerklePatriciaTrie.scala:60-66,
 * 520-542): the subtrees whose node the store lacks stay stubs; only a missing ROOT throws
 * MPTNodeMissingException here.  A commit that walks into a stub throws it too (apply /
 * blockCommit / rootOf, KH_ENODE); missing(handle) then lists what to fetch and fillNodes takes
 * the fetched nodes (the fetch-and-retry loop). */
JNIEXPORT void JNICALL Java_khipu_trie_gpu_Khst_forestLoadPartial(JNIEnv* env, jclass cls, jlong handle,
                                                                 jintArray tries, jbyteArray roots, jbyteArray enc,
                                                                 jlongArray off, jintArray missIdxOut,
                                                                 jbyteArray missOut, jlongArray nMissingOut) {
  (void)cls;
  forest_load(env, handle, tries, roots, enc, off, 0, 0, 0, missIdxOut, missOut, nMissingOut, 1);
}
JNIEXPORT void JNICALL Java_khipu_trie_gpu_Khst_forestLoadPartialDevice(JNIEnv* env, jclass cls, jlong handle,
                                                                       jintArray tries, jbyteArray roots, jlong dEnc,
                                                                       jlong dOff, jlong n, jintArray missIdxOut,
                                                                       jbyteArray missOut, jlongArray nMissingOut) {
  (void)cls;
  if (!dEnc || !dOff) {
    throw_cls(env, "java/lang/IllegalArgumentException", "dEnc / dOff: device addresses");
    return;
  }
  forest_load(env, handle, tries, roots, NULL, NULL, dEnc, dOff, n, missIdxOut, missOut, nMissingOut, 1);
}
/* open a single trie from the nodes at hand (as openNodes; dEnc != 0: the store is in HBM, device
 * addresses on the shared context of the current device) */
static jlong open_partial(JNIEnv* env, jbyteArray root32, jbyteArray enc, jlongArray off, jlong dEnc, jlong dOff,
                          jlong dN, jint flags, jbyteArray missingOut) {
  uint8_t missing[32] = {0};
  kh_trie* h = NULL;
  Bufs b = {0};
  const uint8_t* r = in_b(env, &b, root32);
  const uint8_t* e = dEnc ? NULL : in_b(env, &b, enc);
  const uint64_t* o = dEnc ? NULL : in_l(env, &b, off);
  if (bufs_failed(env, &b)) return 0;
  if (!r || len_of(env, root32) < 32) {
    bufs_free(&b);
    throw_cls(env, "java/lang/IllegalArgumentException", "root32: 32 bytes");
    return 0;
  }
  const int rc = dEnc ? kh_trie_open_partial(NULL, r, (const uint8_t*)(intptr_t)dEnc, (const uint64_t*)(intptr_t)dOff,
                                             (uint64_t)dN, (uint32_t)flags, missing, &h)
                      : kh_trie_open_partial_host(r, e, o, count_of(env, off), (uint32_t)flags, missing, &h);
  bufs_free(&b);
  if (rc == KH_ENODE) put_b(env, missingOut, missing, 32);
  if (rc != KH_OK) {
    throw_kh_hash(env, rc, missing);
    return 0;
  }
  return (jlong)(intptr_t)h;
}
JNIEXPORT jlong JNICALL Java_khipu_trie_gpu_Khst_openPartial(JNIEnv* env, jclass cls, jbyteArray root32,
                                                            jbyteArray enc, jlongArray off, jint flags,
                                                            jbyteArray missingOut) {
  (void)cls;
  return open_partial(env, root32, enc, off, 0, 0, 0, flags, missingOut);
}
JNIEXPORT jlong JNICALL Java_khipu_trie_gpu_Khst_openPartialDevice(JNIEnv* env, jclass cls, jbyteArray root32,
                                                                  jlong dEnc, jlong dOff, jlong n, jint flags,
                                                                  jbyteArray missingOut) {
  (void)cls;
  if (!dEnc || !dOff) {
    throw_cls(env, "java/lang/IllegalArgumentException", "dEnc / dOff: device addresses");
    return 0;
  }
  return open_partial(env, root32, NULL, NULL, dEnc, dOff, n, flags, missingOut);
}
/* resolve the stubs whose node is in the store (between commits: no savepoint open); returns the
 * number of store nodes decoded into the handle */
JNIEXPORT jlong JNICALL Java_khipu_trie_gpu_Khst_fillNodes(JNIEnv* env, jclass cls, jlong handle, jbyteArray enc,
                                                          jlongArray off) {
  (void)cls;
  uint64_t nd = 0;
  Bufs b = {0};
  const uint8_t* e = in_b(env, &b, enc);
  const uint64_t* o = in_l(env, &b, off);
  if (bufs_failed(env, &b)) return 0;
  const int rc = kh_trie_fill_nodes_host(H(handle), e, o, count_of(env, off), &nd, NULL);
  bufs_free(&b);
  if (rc != KH_OK) {
    throw_kh(env, rc);
    return 0;
  }
  return (jlong)nd;
}
JNIEXPORT jlong JNICALL Java_khipu_trie_gpu_Khst_fillNodesDevice(JNIEnv* env, jclass cls, jlong handle, jlong dEnc,
                                                                jlong dOff, jlong n) {
  (void)cls;
  uint64_t nd = 0;
  if (!dEnc || !dOff) {
    throw_cls(env, "java/lang/IllegalArgumentException", "dEnc / dOff: device addresses");
    return 0;
  }
  const int rc = kh_trie_fill_nodes(H(handle), (const uint8_t*)(intptr_t)dEnc, (const uint64_t*)(intptr_t)dOff,
                                    (uint64_t)n, &nd, NULL);
  if (rc != KH_OK) {
    throw_kh(env, rc);
    return 0;
  }
  return (jlong)nd;
}
JNIEXPORT jlong JNICALL Java_khipu_trie_gpu_Khst_stubs(JNIEnv* env, jclass cls, jlong handle) {
  (void)cls;
  uint64_t n = 0;
  const int rc = kh_trie_stubs(H(handle), &n);
  if (rc != KH_OK) throw_kh(env, rc);
  return (jlong)n;
}
/* what the last commit, block commit or rootOf on the handle needed and the handle lacks: 36
 * bytes an entry, the trie id (4 bytes, little endian; 0 on a single trie) then the hash to
 * fetch -- the hash MPTNodeMissingException carries in the reference.  Empty unless that call
 * threw it.  The count is negotiated as forestRoots does. */
JNIEXPORT jbyteArray JNICALL Java_khipu_trie_gpu_Khst_missing(JNIEnv* env, jclass cls, jlong handle) {
  (void)cls;
  uint64_t nm = 0, cap = 0;
  uint32_t* t = NULL;
  uint8_t* r = NULL;
  int rc = KH_ENOSPC;
  for (int tries = 0; rc == KH_ENOSPC && tries < 16; ++tries) { /* the first call reports the count */
    rc = kh_trie_missing(H(handle), t, r, cap, &nm);
    if (rc == KH_ENOSPC) {
      free(t);
      free(r);
      cap = nm + nm / 8;
      t = malloc(4 * (size_t)(cap ? cap : 1));
      r = malloc(32 * (size_t)(cap ? cap : 1));
      if (!t || !r) rc = KH_ENOMEM;
    }
  }
  jbyteArray out = NULL;
  uint8_t* packed = rc == KH_OK ? malloc(36 * (size_t)(nm ? nm : 1)) : NULL;
  if (rc == KH_OK && !packed) rc = KH_ENOMEM;
  if (rc == KH_OK) {
    for (uint64_t i = 0; i < nm; ++i) {
      for (int q = 0; q < 4; ++q) packed[36 * i + q] = (uint8_t)(t[i] >> (8 * q));
      memcpy(packed + 36 * i + 4, r + 32 * i, 32);
    }
    out = bytes_of(env, packed, (jsize)(36 * nm));
  }
  free(packed);
  free(t);
  free(r);
  if (rc != KH_OK) throw_kh(env, rc);
  return out;
}
/* per key (klen bytes each; tries nullable on a single trie) 33 bytes: 1 and the hash of the node
 * to fetch when the key's walk reaches a stub, else 33 zero bytes */
JNIEXPORT jbyteArray JNICALL Java_khipu_trie_gpu_Khst_need(JNIEnv* env, jclass cls, jlong handle, jintArray tries,
                                                          jbyteArray keys, jint klen) {
  (void)cls;
  const uint64_t n = klen > 0 ? (uint64_t)(len_of(env, keys) / klen) : 0;
  Bufs b = {0};
  const uint32_t* t = in_i(env, &b, tries);
  const uint8_t* k = in_b(env, &b, keys);
  uint8_t* fl = bufs_alloc(&b, (size_t)(n ? n : 1));
  uint8_t* hs = bufs_alloc(&b, 32 * (size_t)(n ? n : 1));
  uint8_t* packed = bufs_alloc(&b, 33 * (size_t)(n ? n : 1));
  if (bufs_failed(env, &b)) return NULL;
  if (tries && (uint64_t)len_of(env, tries) < n) {
    bufs_free(&b);
    throw_cls(env, "java/lang/IllegalArgumentException", "tries: one id per key");
    return NULL;
  }
  const int rc = kh_trie_need_host(H(handle), t, k, (uint32_t)klen, n, fl, hs);
  jbyteArray out = NULL;
  if (rc == KH_OK) {
    for (uint64_t i = 0; i < n; ++i) {
      packed[33 * i] = fl[i];
      memcpy(packed + 33 * i + 1, hs + 32 * i, 32);
    }
    out = bytes_of(env, packed, (jsize)(33 * n));
  }
  bufs_free(&b);
  if (rc != KH_OK) throw_kh(env, rc);
  return out;
}

/* The commit witness of a batch (kh_trie_commit_witness_host): every node a handle opened by
 * openPartial / forestLoadPartial at the current root(s) needs to apply the upserts (upKeys) and
 * deletes (delKeys; klen bytes a key, upTrie / delTrie a forest's trie ids or null) at the first
 * attempt, into the caller's arrays as prove fills them (hashes / rlp / off).  sizes[0..3] = nodes /
 * RLP bytes / collapse children / missing nodes.  Returns the node count, or -1 when an array is
 * too small (sizes hold what the call needs: grow and call again).  A partial handle that lacks
 * nodes of the witness throws MPTNodeMissingException with the first hash, after writing the
 * entries that fit into missing (nullable; 36 bytes an entry, as missing() packs them). */
JNIEXPORT jlong JNICALL Java_khipu_trie_gpu_Khst_commitWitness(JNIEnv* env, jclass cls, jlong handle, jintArray upTrie,
                                                              jbyteArray upKeys, jintArray delTrie, jbyteArray delKeys,
                                                              jint klen, jbyteArray hashes, jbyteArray rlp,
                                                              jlongArray off, jbyteArray missing, jlongArray sizes) {
  (void)cls;
  if (klen <= 0) {
    throw_cls(env, "java/lang/IllegalArgumentException", "commitWitness: klen must be positive");
    return 0;
  }
  const uint64_t nup = (uint64_t)len_of(env, upKeys) / (uint64_t)klen;
  const uint64_t ndel = (uint64_t)len_of(env, delKeys) / (uint64_t)klen;
  if ((upTrie && (uint64_t)len_of(env, upTrie) < nup) || (delTrie && (uint64_t)len_of(env, delTrie) < ndel) ||
      len_of(env, off) < 1) {
    throw_cls(env, "java/lang/IllegalArgumentException", "commitWitness: trie ids / off shorter than the keys need");
    return 0;
  }
  uint64_t node_cap = (uint64_t)len_of(env, hashes) / 32;
  if ((uint64_t)len_of(env, off) - 1 < node_cap) node_cap = (uint64_t)len_of(env, off) - 1;
  const uint64_t rlp_cap = (uint64_t)len_of(env, rlp), miss_cap = (uint64_t)len_of(env, missing) / 36;
  Bufs b = {0};
  const uint32_t* ut = in_i(env, &b, upTrie);
  const uint8_t* uk = in_b(env, &b, upKeys);
  const uint32_t* dt = in_i(env, &b, delTrie);
  const uint8_t* dk = in_b(env, &b, delKeys);
  uint8_t* hs = out_buf(env, &b, hashes, 1);
  uint8_t* rl = out_buf(env, &b, rlp, 1);
  uint64_t* of = out_buf(env, &b, off, 8);
  uint32_t* mt = bufs_alloc(&b, 4 * (size_t)(miss_cap ? miss_cap : 1));
  uint8_t* mh = bufs_alloc(&b, 32 * (size_t)(miss_cap ? miss_cap : 1));
  uint8_t* packed = bufs_alloc(&b, 36 * (size_t)(miss_cap ? miss_cap : 1));
  if (bufs_failed(env, &b)) return 0;
  uint64_t nn = 0, nb = 0, nc = 0, nm = 0;
  const int rc = kh_trie_commit_witness_host(H(handle), ut, uk, nup, dt, dk, ndel, (uint32_t)klen, 0, hs, node_cap, rl,
                                             rlp_cap, of, &nn, &nb, &nc, mt, mh, miss_cap, &nm);
  uint8_t first[32] = {0};
  if (rc == KH_OK) {
    put_b(env, hashes, hs, 32 * nn);
    put_b(env, rlp, rl, nb);
    put_l(env, off, of, nn + 1);
  } else if (rc == KH_ENODE) {
    const uint64_t w = nm < miss_cap ? nm : miss_cap;
    for (uint64_t i = 0; i < w; ++i) {
      for (int q = 0; q < 4; ++q) packed[36 * i + q] = (uint8_t)(mt[i] >> (8 * q));
      memcpy(packed + 36 * i + 4, mh + 32 * i, 32);
    }
    put_b(env, missing, packed, 36 * w);
    if (w) memcpy(first, mh, 32);
  }
  bufs_free(&b);
  const jlong sz[4] = {(jlong)nn, (jlong)nb, (jlong)nc, (jlong)nm};
  put_l(env, sizes, sz, 4);
  if (rc == KH_ENOSPC) return -1;
  if (rc != KH_OK) {
    throw_kh_hash(env, rc, first);
    return 0;
  }
  return (jlong)nn;
}

/* every trie the forest holds, ascending ids: 36 bytes a trie, the id (4 bytes, little endian)
 * then its root.  The count is negotiated: KH_ENOSPC reports it, another thread's commit or load
 * can change it again, so the loop grows and retries (bounded), as get does. */
JNIEXPORT jbyteArray JNICALL Java_khipu_trie_gpu_Khst_forestRoots(JNIEnv* env, jclass cls, jlong handle) {
  (void)cls;
  uint64_t nt = 0, cap = 0;
  uint32_t* t = NULL;
  uint8_t* r = NULL;
  int rc = KH_ENOSPC;
  for (int tries = 0; rc == KH_ENOSPC && tries < 16; ++tries) { /* the first call reports the count */
    rc = kh_forest_roots(H(handle), t, r, cap, &nt);
    if (rc == KH_ENOSPC) {
      free(t);
      free(r);
      cap = nt + nt / 8;
      t = malloc(4 * (size_t)(cap ? cap : 1));
      r = malloc(32 * (size_t)(cap ? cap : 1));
      if (!t || !r) rc = KH_ENOMEM;
    }
  }
  jbyteArray out = NULL;
  uint8_t* packed = rc == KH_OK ? malloc(36 * (size_t)(nt ? nt : 1)) : NULL;
  if (rc == KH_OK && !packed) rc = KH_ENOMEM;
  if (rc == KH_OK) {
    for (uint64_t i = 0; i < nt; ++i) {
      for (int q = 0; q < 4; ++q) packed[36 * i + q] = (uint8_t)(t[i] >> (8 * q));
      memcpy(packed + 36 * i + 4, r + 32 * i, 32);
    }
    out = bytes_of(env, packed, (jsize)(36 * nt));
  }
  free(packed);
  free(t);
  free(r);
  if (rc != KH_OK) throw_kh(env, rc);
  return out;
}

/* drop whole tries from HBM (the caller owns residency: an evicted id reads as an empty trie
 * until forestLoadNodes brings it back); returns the number dropped */
JNIEXPORT jlong JNICALL Java_khipu_trie_gpu_Khst_forestEvict(JNIEnv* env, jclass cls, jlong handle, jintArray tries) {
  (void)cls;
  uint64_t dropped = 0;
  Bufs b = {0};
  const uint32_t* t = in_i(env, &b, tries);
  if (bufs_failed(env, &b)) return 0;
  const int rc = kh_forest_evict(H(handle), t, (uint64_t)len_of(env, tries), &dropped);
  bufs_free(&b);
  if (rc != KH_OK) {
    throw_kh(env, rc);
    return 0;
  }
  return (jlong)dropped;
}

/* subtrees of a resident trie back to stubs (kh_trie_evict_subtrees): one prefix per byte of depths,
 * the first depths[i] nibbles of paths32[32i..) in trie tries[i] (nullable on a single trie); status
 * (one byte a prefix, KH_EVICT_*) and hashes32 (32 bytes a prefix: the hash to fetch to bring the
 * subtree back) are filled; returns the keys evicted.  Region copies: the call runs kernels. */
JNIEXPORT jlong JNICALL Java_khipu_trie_gpu_Khst_evictSubtrees(JNIEnv* env, jclass cls, jlong handle, jintArray tries,
                                                              jbyteArray paths32, jbyteArray depths, jbyteArray status,
                                                              jbyteArray hashes32) {
  (void)cls;
  const uint64_t n = (uint64_t)len_of(env, depths);
  if ((uint64_t)len_of(env, paths32) < 32 * n || (tries && (uint64_t)len_of(env, tries) < n) ||
      (uint64_t)len_of(env, status) < n || (uint64_t)len_of(env, hashes32) < 32 * n) {
    throw_cls(env, "java/lang/IllegalArgumentException",
              "paths32 / hashes32: 32 bytes a prefix; tries / status: one entry a prefix");
    return 0;
  }
  uint64_t keys = 0;
  Bufs b = {0};
  const uint32_t* t = in_i(env, &b, tries);
  const uint8_t* p = in_b(env, &b, paths32);
  const uint8_t* d = in_b(env, &b, depths);
  uint8_t* st = bufs_alloc(&b, (size_t)(n ? n : 1));
  uint8_t* hs = bufs_alloc(&b, 32 * (size_t)(n ? n : 1));
  if (bufs_failed(env, &b)) return 0;
  const int rc = kh_trie_evict_subtrees(H(handle), t, p, d, n, st, hs, NULL, &keys, NULL);
  if (rc == KH_OK) {
    put_b(env, status, st, n);
    put_b(env, hashes32, hs, 32 * n);
  }
  bufs_free(&b);
  if (rc != KH_OK) {
    throw_kh(env, rc);
    return 0;
  }
  return (jlong)keys;
}

/* One block (BlockWorldState.scala:243-252 then TrieAccounts.flush): storage ops into the
 * forest, the new storage roots written into the named account bodies (accTrie[i], -1 =
 * KH_NO_TRIE: none), the account ops into the state trie.  All or nothing.  Returns the state
 * root. */
JNIEXPORT jbyteArray JNICALL Java_khipu_trie_gpu_Khst_blockCommit(
    JNIEnv* env, jclass cls, jlong state, jlong storage, jintArray slotTrie, jbyteArray slotKeys, jbyteArray slotVals,
    jlongArray slotVoff, jintArray delSlotTrie, jbyteArray delSlotKeys, jint slotKlen, jbyteArray accKeys,
    jbyteArray accBodies, jlongArray accVoff, jintArray accTrie, jbyteArray delAccKeys, jint accKlen,
    jlongArray statsOut) {
  (void)cls;
  const uint64_t ns_up = count_of(env, slotVoff), ns_del = (uint64_t)len_of(env, delSlotTrie);
  const uint64_t na_up = count_of(env, accVoff);
  const uint64_t na_del = accKlen > 0 ? (uint64_t)(len_of(env, delAccKeys) / accKlen) : 0;
  uint8_t root[32];
  kh_stats st;
  Bufs b = {0};
  const uint32_t* st_ = in_i(env, &b, slotTrie);
  const uint8_t* sk = in_b(env, &b, slotKeys);
  const uint8_t* sv = in_b(env, &b, slotVals);
  const uint64_t* so = in_l(env, &b, slotVoff);
  const uint32_t* sdt = in_i(env, &b, delSlotTrie);
  const uint8_t* sdk = in_b(env, &b, delSlotKeys);
  const uint8_t* ak = in_b(env, &b, accKeys);
  const uint8_t* av = in_b(env, &b, accBodies);
  const uint64_t* ao = in_l(env, &b, accVoff);
  const uint32_t* at = in_i(env, &b, accTrie);
  const uint8_t* adk = in_b(env, &b, delAccKeys);
  if (bufs_failed(env, &b)) return NULL;
  const int rc = kh_block_commit_host(H(state), H(storage), st_, sk, sv, so, ns_up, sdt, sdk, ns_del,
                                      (uint32_t)slotKlen, ak, av, ao, at, na_up, adk, na_del, (uint32_t)accKlen, root,
                                      &st);
  bufs_free(&b);
  if (rc != KH_OK) {
    throw_kh_commit(env, rc, H(storage), H(state));
    return NULL;
  }
  put_stats(env, statsOut, &st);
  return bytes_of(env, root, 32);
}

/* BlockWorldState.persist (BlockWorldState.scala:312-330): the nodes the last commit created
 * (opened with EMIT_NODES) into hashes / rlp / off; sizes[0] / sizes[1] = nodes / RLP bytes.
 * Returns the node count, or -1 when an output array is too small (sizes hold what is
 * needed: grow and call again; nothing is re-encoded). */
JNIEXPORT jlong JNICALL Java_khipu_trie_gpu_Khst_emitNodes(JNIEnv* env, jclass cls, jlong handle, jbyteArray hashes,
                                                          jbyteArray rlp, jlongArray off, jlongArray sizes) {
  (void)cls;
  const uint64_t node_cap = (uint64_t)len_of(env, hashes) / 32, rlp_cap = (uint64_t)len_of(env, rlp);
  const jsize noff = len_of(env, off);
  const uint64_t cap = node_cap < (uint64_t)(noff > 0 ? noff - 1 : 0) ? node_cap : (uint64_t)(noff > 0 ? noff - 1 : 0);
  uint64_t nn = 0, nb = 0;
  Bufs b = {0};
  uint8_t* hs = out_buf(env, &b, hashes, 1);
  uint8_t* rl = out_buf(env, &b, rlp, 1);
  uint64_t* of = out_buf(env, &b, off, 8);
  if (bufs_failed(env, &b)) return 0;
  const int rc = kh_trie_emit_nodes(H(handle), hs, cap, rl, rlp_cap, of, &nn, &nb);
  if (rc == KH_OK) {
    put_b(env, hashes, hs, 32 * nn);
    put_b(env, rlp, rl, nb);
    put_l(env, off, of, nn + 1);
  }
  bufs_free(&b);
  const jlong sz[2] = {(jlong)nn, (jlong)nb};
  put_l(env, sizes, sz, 2);
  if (rc == KH_ENOSPC) return -1;
  if (rc != KH_OK) {
    throw_kh(env, rc);
    return 0;
  }
  return (jlong)nn;
}

/* MerklePatriciaTrie.get for a batch (MerklePatriciaTrie.scala:90-147): byte[][] with null for
 * an absent key (None); trieIds (int[], nullable) for a forest.  The value bytes' size is
 * negotiated: a call that finds them larger than the buffer returns KH_ENOSPC with the size;
 * another thread's commit on the handle between two calls can change it again, so the loop
 * grows and retries (bounded) as khipu_amd/device.py does. */
#define GET_TRIES 16
JNIEXPORT jobjectArray JNICALL Java_khipu_trie_gpu_Khst_get(JNIEnv* env, jclass cls, jlong handle, jintArray trieIds,
                                                           jbyteArray keys, jint klen) {
  (void)cls;
  const jsize n = klen > 0 ? len_of(env, keys) / klen : 0;
  Bufs b = {0};
  const uint32_t* t = in_i(env, &b, trieIds);
  const uint8_t* k = in_b(env, &b, keys);
  uint8_t* found = bufs_alloc(&b, (size_t)n);
  uint64_t* voff = bufs_alloc(&b, 8 * ((size_t)n + 1));
  if (bufs_failed(env, &b)) return NULL;
  uint64_t need = 0, cap = 0;
  uint8_t* vals = NULL;
  int rc = KH_ENOSPC;
  for (int tries = 0; rc == KH_ENOSPC && tries < GET_TRIES; ++tries) { /* the first call reports the bytes needed */
    rc = kh_trie_get_host(H(handle), t, k, (uint32_t)klen, (uint64_t)n, vals, cap, voff, found, &need);
    if (rc == KH_ENOSPC) {
      free(vals);
      cap = need + need / 8; /* headroom for a concurrent commit that grows the values again */
      vals = malloc((size_t)(cap ? cap : 1));
      if (!vals) rc = KH_ENOMEM;
    }
  }
  jobjectArray out = NULL;
  if (rc == KH_OK) {
    jclass ba = (*env)->FindClass(env, "[B");
    out = ba ? (*env)->NewObjectArray(env, n, ba, NULL) : NULL;
    for (jsize i = 0; out && i < n; ++i) {
      if (!found[i]) continue; /* None */
      jbyteArray v = bytes_of(env, vals + voff[i], (jsize)(voff[i + 1] - voff[i]));
      if (!v) break; /* OutOfMemoryError pending */
      (*env)->SetObjectArrayElement(env, out, i, v);
      (*env)->DeleteLocalRef(env, v);
    }
  }
  free(vals);
  bufs_free(&b);
  if (rc != KH_OK) throw_kh(env, rc);
  return out;
}

/* Checkpoint: the next chunk of the current version's node store
 * into hashes / rlp / off, the nodes NodeStorage.update(Nil, pairs) takes.  cursor: long[2], zeroed
 * to start, advanced by the call; trieFilter: a forest's trie id or -1 (KH_NO_TRIE); flags:
 * KH_EXPORT_VERIFY.  sizes[0] / sizes[1] = nodes / RLP bytes written, sizes[2] = 1 when the
 * records are exhausted.  Returns the node count, or -1 when not even the next record's nodes
 * fit the arrays (sizes[0] / sizes[1] hold what it needs: grow and call again, the cursor is
 * unchanged).  A cursor from before a commit, rollback or compaction throws. */
JNIEXPORT jlong JNICALL Java_khipu_trie_gpu_Khst_exportNodes(JNIEnv* env, jclass cls, jlong handle, jint trieFilter,
                                                            jint flags, jlongArray cursor, jbyteArray hashes,
                                                            jbyteArray rlp, jlongArray off, jlongArray sizes) {
  (void)cls;
  if (len_of(env, cursor) < 2) {
    throw_cls(env, "java/lang/IllegalArgumentException", "exportNodes: cursor must be a long[2]");
    return 0;
  }
  const uint64_t node_cap = (uint64_t)len_of(env, hashes) / 32, rlp_cap = (uint64_t)len_of(env, rlp);
  const jsize noff = len_of(env, off);
  const uint64_t cap = node_cap < (uint64_t)(noff > 0 ? noff - 1 : 0) ? node_cap : (uint64_t)(noff > 0 ? noff - 1 : 0);
  jlong cw[2];
  (*env)->GetLongArrayRegion(env, cursor, 0, 2, cw);
  kh_export_cursor cur = {(uint64_t)cw[0], (uint64_t)cw[1]};
  uint64_t nn = 0, nb = 0;
  int done = 0;
  Bufs b = {0};
  uint8_t* hs = out_buf(env, &b, hashes, 1);
  uint8_t* rl = out_buf(env, &b, rlp, 1);
  uint64_t* of = out_buf(env, &b, off, 8);
  if (bufs_failed(env, &b)) return 0;
  const int rc = kh_trie_export_nodes(H(handle), (uint32_t)trieFilter, (uint32_t)flags, &cur, hs, cap, rl,
                                      cap ? rlp_cap : 0, of, &nn, &nb, &done);
  if (rc == KH_OK) {
    put_b(env, hashes, hs, 32 * nn);
    put_b(env, rlp, rl, nb);
    put_l(env, off, of, nn + 1);
    cw[0] = (jlong)cur.next;
    cw[1] = (jlong)cur.epoch;
    (*env)->SetLongArrayRegion(env, cursor, 0, 2, cw);
  }
  bufs_free(&b);
  const jlong sz[3] = {(jlong)nn, (jlong)nb, (jlong)done};
  put_l(env, sizes, sz, 3);
  if (rc == KH_ENOSPC) return -1;
  if (rc != KH_OK) {
    throw_kh(env, rc);
    return 0;
  }
  return (jlong)nn;
}

/* HostService's GetNodeData (HostService.scala:103-112 -> Blockchain.getMptNodeByHash,
 * Blockchain.scala:356-357) for a batch of 32-byte hashes (at most 4096): byte[][] with null for a
 * hash no node of the current version has.  The encodings' size is negotiated like get's. */
JNIEXPORT jobjectArray JNICALL Java_khipu_trie_gpu_Khst_nodesByHash(JNIEnv* env, jclass cls, jlong handle,
                                                                   jbyteArray hashes) {
  (void)cls;
  const jsize n = len_of(env, hashes) / 32;
  Bufs b = {0};
  const uint8_t* hs = in_b(env, &b, hashes);
  uint8_t* found = bufs_alloc(&b, (size_t)n);
  uint64_t* off = bufs_alloc(&b, 8 * ((size_t)n + 1));
  if (bufs_failed(env, &b)) return NULL;
  uint64_t need = 0, cap = 0;
  uint8_t* rl = NULL;
  int rc = KH_ENOSPC;
  for (int tries = 0; rc == KH_ENOSPC && tries < GET_TRIES; ++tries) { /* the first call reports the bytes needed */
    rc = kh_trie_nodes_by_hash(H(handle), hs, (uint64_t)n, found, rl, cap, off, &need);
    if (rc == KH_ENOSPC) {
      free(rl);
      cap = need + need / 8; /* headroom for a concurrent commit that grows the nodes again */
      rl = malloc((size_t)(cap ? cap : 1));
      if (!rl) rc = KH_ENOMEM;
    }
  }
  jobjectArray out = NULL;
  if (rc == KH_OK) {
    jclass ba = (*env)->FindClass(env, "[B");
    out = ba ? (*env)->NewObjectArray(env, n, ba, NULL) : NULL;
    for (jsize i = 0; out && i < n; ++i) {
      if (!found[i]) continue; /* None */
      jbyteArray v = bytes_of(env, rl + off[i], (jsize)(off[i + 1] - off[i]));
      if (!v) break; /* OutOfMemoryError pending */
      (*env)->SetObjectArrayElement(env, out, i, v);
      (*env)->DeleteLocalRef(env, v);
    }
  }
  free(rl);
  bufs_free(&b);
  if (rc != KH_OK) throw_kh(env, rc);
  return out;
}

/* Merkle proofs of keys.length / klen keys (trie: a forest's trie ids, or null) into the caller's
 * arrays: found[n], the node table (hashes / rlp / off as exportNodes fills them), pathIdx and
 * pathOff[n + 1] -- the proof of key i is the table nodes pathIdx[k], k in [pathOff[i],
 * pathOff[i + 1]), root first.  flags: KH_PROVE_SHARED (a block witness: every node once).
 * sizes[0..2] = nodes / RLP bytes / path entries.  Returns the node count, or -1 when an array is
 * too small (sizes hold what the call needs: grow and call again). */
JNIEXPORT jlong JNICALL Java_khipu_trie_gpu_Khst_prove(JNIEnv* env, jclass cls, jlong handle, jintArray trie,
                                                      jbyteArray keys, jint klen, jint flags, jbyteArray found,
                                                      jbyteArray hashes, jbyteArray rlp, jlongArray off,
                                                      jintArray pathIdx, jlongArray pathOff, jlongArray sizes) {
  (void)cls;
  if (klen <= 0) {
    throw_cls(env, "java/lang/IllegalArgumentException", "prove: klen must be positive");
    return 0;
  }
  const uint64_t n = (uint64_t)len_of(env, keys) / (uint64_t)klen;
  if ((uint64_t)len_of(env, found) < n || (uint64_t)len_of(env, pathOff) < n + 1 ||
      (trie && (uint64_t)len_of(env, trie) < n) || len_of(env, off) < 1) {
    throw_cls(env, "java/lang/IllegalArgumentException", "prove: found / pathOff / trie / off shorter than the keys need");
    return 0;
  }
  uint64_t node_cap = (uint64_t)len_of(env, hashes) / 32;
  if ((uint64_t)len_of(env, off) - 1 < node_cap) node_cap = (uint64_t)len_of(env, off) - 1;
  const uint64_t rlp_cap = (uint64_t)len_of(env, rlp), path_cap = (uint64_t)len_of(env, pathIdx);
  Bufs b = {0};
  const uint32_t* tr = in_i(env, &b, trie);
  const uint8_t* ks = in_b(env, &b, keys);
  uint8_t* fd = out_buf(env, &b, found, 1);
  uint8_t* hs = out_buf(env, &b, hashes, 1);
  uint8_t* rl = out_buf(env, &b, rlp, 1);
  uint64_t* of = out_buf(env, &b, off, 8);
  uint32_t* pi = out_buf(env, &b, pathIdx, 4);
  uint64_t* po = out_buf(env, &b, pathOff, 8);
  if (bufs_failed(env, &b)) return 0;
  uint64_t nn = 0, nb = 0, np = 0;
  const int rc = kh_trie_prove(H(handle), tr, ks, (uint32_t)klen, n, (uint32_t)flags, fd, hs, node_cap, rl, rlp_cap, of,
                               pi, path_cap, po, &nn, &nb, &np);
  if (rc == KH_OK) {
    put_b(env, found, fd, n);
    put_b(env, hashes, hs, 32 * nn);
    put_b(env, rlp, rl, nb);
    put_l(env, off, of, nn + 1);
    put_i(env, pathIdx, pi, np);
    put_l(env, pathOff, po, n + 1);
  }
  bufs_free(&b);
  const jlong sz[3] = {(jlong)nn, (jlong)nb, (jlong)np};
  put_l(env, sizes, sz, 3);
  if (rc == KH_ENOSPC) return -1;
  if (rc != KH_OK) {
    throw_kh(env, rc);
    return 0;
  }
  return (jlong)nn;
}

/* A page of a resident trie in key order (kh_trie_range_host): the first entries of [origin, limit]
 * (byte[32] each, or null: the lowest / the highest key) of trie `trie` (forests; ignored on a
 * single trie) into the caller's arrays: keys (32 bytes an entry), the values packed into vals with
 * voff; at most min(keys.length / 32, voff.length - 1) entries, with values fitting vals.  Keys
 * are trie keys (the kec256 values on a KH_HASH_KEYS handle).  sizes[0] = entries, sizes[1] =
 * value bytes, sizes[2] = 1 when an entry in range was not returned: next (byte[32]) is its key,
 * the origin of the next call.  Returns the entry count, or -1 when vals cannot hold even the first
 * value (sizes[1] is its size: grow and call again).  A partial handle whose page meets a missing
 * subtree throws MPTNodeMissingException with the hash to fetch. */
JNIEXPORT jlong JNICALL Java_khipu_trie_gpu_Khst_range(JNIEnv* env, jclass cls, jlong handle, jint trie,
                                                      jbyteArray origin, jbyteArray limit, jbyteArray keys,
                                                      jbyteArray vals, jlongArray voff, jbyteArray next,
                                                      jlongArray sizes) {
  (void)cls;
  if ((origin && len_of(env, origin) != 32) || (limit && len_of(env, limit) != 32) || len_of(env, next) < 32) {
    throw_cls(env, "java/lang/IllegalArgumentException", "range: origin / limit / next must hold 32 bytes");
    return 0;
  }
  uint64_t max_entries = (uint64_t)len_of(env, keys) / 32;
  const jsize nvo = len_of(env, voff);
  if ((uint64_t)(nvo > 0 ? nvo - 1 : 0) < max_entries) max_entries = (uint64_t)(nvo > 0 ? nvo - 1 : 0);
  if (max_entries == 0) {
    throw_cls(env, "java/lang/IllegalArgumentException", "range: keys / voff hold no entry");
    return 0;
  }
  Bufs b = {0};
  const uint8_t* og = in_b(env, &b, origin);
  const uint8_t* lm = in_b(env, &b, limit);
  uint8_t* ks = out_buf(env, &b, keys, 1);
  uint8_t* vs = out_buf(env, &b, vals, 1);
  uint64_t* vo = out_buf(env, &b, voff, 8);
  if (bufs_failed(env, &b)) return 0;
  uint64_t ne = 0, nb = 0;
  int more = 0;
  uint8_t nx[32] = {0}, miss[32] = {0};
  const int rc = kh_trie_range_host(H(handle), (uint32_t)trie, og, lm, max_entries, ks, vs, (uint64_t)len_of(env, vals),
                                    vo, &ne, &nb, &more, nx, miss);
  if (rc == KH_OK) {
    put_b(env, keys, ks, 32 * ne);
    put_b(env, vals, vs, nb);
    put_l(env, voff, vo, ne + 1);
    if (more) put_b(env, next, nx, 32);
  }
  bufs_free(&b);
  const jlong sz[3] = {(jlong)ne, (jlong)nb, (jlong)more};
  put_l(env, sizes, sz, 3);
  if (rc == KH_ENOSPC) return -1;
  if (rc != KH_OK) {
    throw_kh_hash(env, rc, miss);
    return 0;
  }
  return (jlong)ne;
}

/* Many ranges in one call (kh_trie_ranges_host): nq requests -- trie tries[q] (forests; null on a
 * single trie), range [origins[32q..), limits[32q..)] (either array null: the lowest / the highest
 * key for every request) -- answered in request order under ONE budget: at most
 * min(keys.length / 32, voff.length - 1) entries in total, with values fitting vals in total.  The
 * entries go into keys / vals / voff as in range; request q's entries are entOff[q] .. entOff[q+1]
 * (entOff holds nq + 1).  sizes[0] = entries, sizes[1] = value bytes, sizes[2] = the number of
 * leading requests answered completely: when it is less than nq, that request is the cut one, next
 * (byte[32]) its first key not returned, and the requests after it are to be asked again.  Returns
 * the entry count, or -1 when vals cannot hold even the first value (sizes[1] is its size).  A
 * partial handle whose answer meets a missing subtree throws MPTNodeMissingException with the hash
 * to fetch, sizes[2] the request it belongs to. */
JNIEXPORT jlong JNICALL Java_khipu_trie_gpu_Khst_ranges(JNIEnv* env, jclass cls, jlong handle, jintArray tries,
                                                       jbyteArray origins, jbyteArray limits, jint nq,
                                                       jbyteArray keys, jbyteArray vals, jlongArray voff,
                                                       jlongArray entOff, jbyteArray next, jlongArray sizes) {
  (void)cls;
  if (nq <= 0 || (tries && len_of(env, tries) < nq) || (origins && (uint64_t)len_of(env, origins) < 32ull * (uint64_t)nq) ||
      (limits && (uint64_t)len_of(env, limits) < 32ull * (uint64_t)nq) || len_of(env, entOff) < nq + 1 ||
      len_of(env, next) < 32) {
    throw_cls(env, "java/lang/IllegalArgumentException",
              "ranges: nq must be positive; tries / origins / limits / entOff must hold nq requests, next 32 bytes");
    return 0;
  }
  uint64_t max_entries = (uint64_t)len_of(env, keys) / 32;
  const jsize nvo = len_of(env, voff);
  if ((uint64_t)(nvo > 0 ? nvo - 1 : 0) < max_entries) max_entries = (uint64_t)(nvo > 0 ? nvo - 1 : 0);
  if (max_entries == 0) {
    throw_cls(env, "java/lang/IllegalArgumentException", "ranges: keys / voff hold no entry");
    return 0;
  }
  Bufs b = {0};
  const uint32_t* tr = in_i(env, &b, tries);
  const uint8_t* og = in_b(env, &b, origins);
  const uint8_t* lm = in_b(env, &b, limits);
  uint8_t* ks = out_buf(env, &b, keys, 1);
  uint8_t* vs = out_buf(env, &b, vals, 1);
  uint64_t* vo = out_buf(env, &b, voff, 8);
  uint64_t* eo = out_buf(env, &b, entOff, 8);
  if (bufs_failed(env, &b)) return 0;
  uint64_t ne = 0, nb = 0, nd = 0;
  uint8_t nx[32] = {0}, miss[32] = {0};
  const int rc = kh_trie_ranges_host(H(handle), tr, og, lm, (uint64_t)nq, max_entries, ks, vs,
                                     (uint64_t)len_of(env, vals), vo, eo, &ne, &nb, &nd, nx, miss);
  if (rc == KH_OK) {
    put_b(env, keys, ks, 32 * ne);
    put_b(env, vals, vs, nb);
    put_l(env, voff, vo, ne + 1);
    put_l(env, entOff, eo, (uint64_t)nq + 1);
    if (nd < (uint64_t)nq) put_b(env, next, nx, 32);
  }
  bufs_free(&b);
  const jlong sz[3] = {(jlong)ne, (jlong)nb, (jlong)nd};
  put_l(env, sizes, sz, 3);
  if (rc == KH_ENOSPC) return -1;
  if (rc != KH_OK) {
    throw_kh_hash(env, rc, miss);
    return 0;
  }
  return (jlong)ne;
}

/* What differs between two resident tries, in key order (kh_trie_diff_host): side a is trie trieA of
 * handleA, side b trie trieB of handleB (the ids are read on forests only; the two handles may be
 * one forest).  The first differences of [origin, limit] (byte[32] each, or null: the lowest / the
 * highest key) go into the caller's arrays: keys (32 bytes a difference), kinds (1: in a only, a
 * delete on the way from a to b; 2: in b only; 3: in both and changed), b's values packed into vals
 * with voff (an empty span for kind 1); at most min(keys.length / 32, kinds.length, voff.length - 1)
 * differences, with values fitting vals.  sizes[0] = differences, sizes[1] = value bytes, sizes[2]
 * = 1 when a difference in range was not returned: next (byte[32]) is its key, the origin of the
 * next call.  Returns the count, or -1 when vals cannot hold even the first value (sizes[1] is its
 * size: grow and call again).  A partial handle whose changed paths meet a missing subtree throws
 * MPTNodeMissingException with the hash to fetch. */
JNIEXPORT jlong JNICALL Java_khipu_trie_gpu_Khst_diff(JNIEnv* env, jclass cls, jlong handleA, jint trieA,
                                                     jlong handleB, jint trieB, jbyteArray origin, jbyteArray limit,
                                                     jbyteArray keys, jbyteArray kinds, jbyteArray vals,
                                                     jlongArray voff, jbyteArray next, jlongArray sizes) {
  (void)cls;
  if ((origin && len_of(env, origin) != 32) || (limit && len_of(env, limit) != 32) || len_of(env, next) < 32) {
    throw_cls(env, "java/lang/IllegalArgumentException", "diff: origin / limit / next must hold 32 bytes");
    return 0;
  }
  uint64_t max_entries = (uint64_t)len_of(env, keys) / 32;
  const jsize nvo = len_of(env, voff);
  if ((uint64_t)(nvo > 0 ? nvo - 1 : 0) < max_entries) max_entries = (uint64_t)(nvo > 0 ? nvo - 1 : 0);
  if ((uint64_t)len_of(env, kinds) < max_entries) max_entries = (uint64_t)len_of(env, kinds);
  if (max_entries == 0) {
    throw_cls(env, "java/lang/IllegalArgumentException", "diff: keys / kinds / voff hold no difference");
    return 0;
  }
  Bufs b = {0};
  const uint8_t* og = in_b(env, &b, origin);
  const uint8_t* lm = in_b(env, &b, limit);
  uint8_t* ks = out_buf(env, &b, keys, 1);
  uint8_t* kd = out_buf(env, &b, kinds, 1);
  uint8_t* vs = out_buf(env, &b, vals, 1);
  uint64_t* vo = out_buf(env, &b, voff, 8);
  if (bufs_failed(env, &b)) return 0;
  uint64_t ne = 0, nb = 0;
  int more = 0;
  uint8_t nx[32] = {0}, miss[32] = {0};
  const int rc = kh_trie_diff_host(H(handleA), (uint32_t)trieA, H(handleB), (uint32_t)trieB, og, lm, max_entries,
                                   (uint64_t)len_of(env, vals), ks, kd, vs, vo, &ne, &nb, &more, nx, miss);
  if (rc == KH_OK) {
    put_b(env, keys, ks, 32 * ne);
    put_b(env, kinds, kd, ne);
    put_b(env, vals, vs, nb);
    put_l(env, voff, vo, ne + 1);
    if (more) put_b(env, next, nx, 32);
  }
  bufs_free(&b);
  const jlong sz[3] = {(jlong)ne, (jlong)nb, (jlong)more};
  put_l(env, sizes, sz, 3);
  if (rc == KH_ENOSPC) return -1;
  if (rc != KH_OK) {
    throw_kh_hash(env, rc, miss);
    return 0;
  }
  return (jlong)ne;
}

/* The keys changed since an open savepoint of a resident trie or forest, read from its undo journal
 * without a copy (kh_trie_changes_since_host): level 0 is the innermost savepoint, 1 .. depth that
 * savepoint counted from the outermost.  The differences from (fromTrie, from) on (from byte[32] or
 * null: from the beginning; fromTrie is read on forests only) go into the caller's arrays as diff's
 * do -- side a the savepoint's version, side b the current one, and with reverse the other way
 * round (the ops that undo the commits: a reorg) -- with tries (int per difference; may be null on a
 * single trie) naming each difference's trie: at most min(keys.length / 32, kinds.length,
 * voff.length - 1, tries.length) differences, with values fitting vals.  sizes[0] = differences,
 * sizes[1] = value bytes, sizes[2] = 1 when a difference was not returned: next (byte[32]) is its
 * key and sizes[4] its trie, the (fromTrie, from) of the next call; sizes[3] = the differences from
 * (fromTrie, from) on, returned or not: one call sized from it takes them all.  Returns the count,
 * or -1 when vals cannot hold even the first value (sizes[1] is its size, sizes[3] is set: grow and
 * call again).  Exact on partial handles: never MPTNodeMissingException.  Region copies only, no
 * critical region. */
JNIEXPORT jlong JNICALL Java_khipu_trie_gpu_Khst_changesSince(JNIEnv* env, jclass cls, jlong handle, jint level,
                                                             jboolean reverse, jint fromTrie, jbyteArray from,
                                                             jintArray tries, jbyteArray keys, jbyteArray kinds,
                                                             jbyteArray vals, jlongArray voff, jbyteArray next,
                                                             jlongArray sizes) {
  (void)cls;
  if ((from && len_of(env, from) != 32) || len_of(env, next) < 32 || level < 0 || len_of(env, sizes) < 5) {
    throw_cls(env, "java/lang/IllegalArgumentException",
              "changesSince: from / next must hold 32 bytes, sizes 5 longs, level must not be negative");
    return 0;
  }
  uint64_t max_entries = (uint64_t)len_of(env, keys) / 32;
  const jsize nvo = len_of(env, voff);
  if ((uint64_t)(nvo > 0 ? nvo - 1 : 0) < max_entries) max_entries = (uint64_t)(nvo > 0 ? nvo - 1 : 0);
  if ((uint64_t)len_of(env, kinds) < max_entries) max_entries = (uint64_t)len_of(env, kinds);
  if (tries && (uint64_t)len_of(env, tries) < max_entries) max_entries = (uint64_t)len_of(env, tries);
  if (max_entries == 0) {
    throw_cls(env, "java/lang/IllegalArgumentException", "changesSince: keys / kinds / voff / tries hold no difference");
    return 0;
  }
  Bufs b = {0};
  const uint8_t* fr = in_b(env, &b, from);
  uint32_t* ts = out_buf(env, &b, tries, 4);
  uint8_t* ks = out_buf(env, &b, keys, 1);
  uint8_t* kd = out_buf(env, &b, kinds, 1);
  uint8_t* vs = out_buf(env, &b, vals, 1);
  uint64_t* vo = out_buf(env, &b, voff, 8);
  if (bufs_failed(env, &b)) return 0;
  uint64_t ne = 0, nb = 0, total = 0;
  int more = 0;
  uint32_t nt = 0;
  uint8_t nx[32] = {0};
  const int rc = kh_trie_changes_since_host(H(handle), (uint32_t)level, reverse ? KH_CHANGES_REVERSE : 0u,
                                            (uint32_t)fromTrie, fr, max_entries, (uint64_t)len_of(env, vals), ts, ks, kd,
                                            vs, vo, &ne, &nb, &total, &more, &nt, nx);
  if (rc == KH_OK) {
    put_i(env, tries, ts, ne);
    put_b(env, keys, ks, 32 * ne);
    put_b(env, kinds, kd, ne);
    put_b(env, vals, vs, nb);
    put_l(env, voff, vo, ne + 1);
    if (more) put_b(env, next, nx, 32);
  }
  bufs_free(&b);
  const jlong sz[5] = {(jlong)ne, (jlong)nb, (jlong)more, (jlong)total, (jlong)nt};
  put_l(env, sizes, sz, 5);
  if (rc == KH_ENOSPC) return -1;
  if (rc != KH_OK) {
    throw_kh(env, rc);
    return 0;
  }
  return (jlong)ne;
}

/* Many trie pairs in one call (kh_trie_diffs_host): nq requests -- trie triesA[q] of handleA against
 * trie triesB[q] of handleB (the ids are read on forests only and may be null on a single trie;
 * triesB null: triesA, two versions of one forest), range [origins[32q..), limits[32q..)] (either
 * array null: the lowest / the highest key for every request) -- answered in request order under
 * ONE budget: at most min(keys.length / 32, kinds.length, voff.length - 1) differences in total,
 * with values fitting vals in total.  The differences go into keys / kinds / vals / voff as in diff;
 * request q's differences are entOff[q] .. entOff[q+1] (entOff holds nq + 1).  sizes[0] =
 * differences, sizes[1] = value bytes, sizes[2] = the number of leading requests answered
 * completely: when it is less than nq, that request is the cut one, next (byte[32]) its first
 * differing key not returned, and the requests after it are to be asked again.  Returns the count,
 * or -1 when vals cannot hold even the first value (sizes[1] is its size).  A partial handle whose
 * changed paths meet a missing subtree throws MPTNodeMissingException with the hash to fetch,
 * sizes[2] the request it belongs to.  Region copies only, no critical region, as ranges. */
JNIEXPORT jlong JNICALL Java_khipu_trie_gpu_Khst_diffs(JNIEnv* env, jclass cls, jlong handleA, jintArray triesA,
                                                      jlong handleB, jintArray triesB, jbyteArray origins,
                                                      jbyteArray limits, jint nq, jbyteArray keys, jbyteArray kinds,
                                                      jbyteArray vals, jlongArray voff, jlongArray entOff,
                                                      jbyteArray next, jlongArray sizes) {
  (void)cls;
  if (nq <= 0 || (triesA && len_of(env, triesA) < nq) || (triesB && len_of(env, triesB) < nq) ||
      (origins && (uint64_t)len_of(env, origins) < 32ull * (uint64_t)nq) ||
      (limits && (uint64_t)len_of(env, limits) < 32ull * (uint64_t)nq) || len_of(env, entOff) < nq + 1 ||
      len_of(env, next) < 32) {
    throw_cls(env, "java/lang/IllegalArgumentException",
              "diffs: nq must be positive; triesA / triesB / origins / limits / entOff must hold nq requests, next 32 bytes");
    return 0;
  }
  uint64_t max_entries = (uint64_t)len_of(env, keys) / 32;
  const jsize nvo = len_of(env, voff);
  if ((uint64_t)(nvo > 0 ? nvo - 1 : 0) < max_entries) max_entries = (uint64_t)(nvo > 0 ? nvo - 1 : 0);
  if ((uint64_t)len_of(env, kinds) < max_entries) max_entries = (uint64_t)len_of(env, kinds);
  if (max_entries == 0) {
    throw_cls(env, "java/lang/IllegalArgumentException", "diffs: keys / kinds / voff hold no difference");
    return 0;
  }
  Bufs b = {0};
  const uint32_t* ta = in_i(env, &b, triesA);
  const uint32_t* tb = in_i(env, &b, triesB);
  const uint8_t* og = in_b(env, &b, origins);
  const uint8_t* lm = in_b(env, &b, limits);
  uint8_t* ks = out_buf(env, &b, keys, 1);
  uint8_t* kd = out_buf(env, &b, kinds, 1);
  uint8_t* vs = out_buf(env, &b, vals, 1);
  uint64_t* vo = out_buf(env, &b, voff, 8);
  uint64_t* eo = out_buf(env, &b, entOff, 8);
  if (bufs_failed(env, &b)) return 0;
  uint64_t ne = 0, nb = 0, nd = 0;
  uint8_t nx[32] = {0}, miss[32] = {0};
  const int rc = kh_trie_diffs_host(H(handleA), ta, H(handleB), tb, og, lm, (uint64_t)nq, max_entries,
                                    (uint64_t)len_of(env, vals), ks, kd, vs, vo, eo, &ne, &nb, &nd, nx, miss);
  if (rc == KH_OK) {
    put_b(env, keys, ks, 32 * ne);
    put_b(env, kinds, kd, ne);
    put_b(env, vals, vs, nb);
    put_l(env, voff, vo, ne + 1);
    put_l(env, entOff, eo, (uint64_t)nq + 1);
    if (nd < (uint64_t)nq) put_b(env, next, nx, 32);
  }
  bufs_free(&b);
  const jlong sz[3] = {(jlong)ne, (jlong)nb, (jlong)nd};
  put_l(env, sizes, sz, 3);
  if (rc == KH_ENOSPC) return -1;
  if (rc != KH_OK) {
    throw_kh_hash(env, rc, miss);
    return 0;
  }
  return (jlong)ne;
}

/* The proofs prove returned (or a peer sent) checked against roots (32 bytes: one root for every
 * key; or 32 per key): status[i] one of KH_PROOF_*, the values of the KH_PROOF_VALUE keys packed
 * into vals with voff[n + 1].  nNodes table nodes in rlp / off.  flags: KH_HASH_KEYS.  Returns the
 * value bytes written, or -1 when vals is too small (sizes[0] holds the bytes needed). */
JNIEXPORT jlong JNICALL Java_khipu_trie_gpu_Khst_verifyProofs(JNIEnv* env, jclass cls, jbyteArray roots,
                                                             jbyteArray keys, jint klen, jint flags, jbyteArray rlp,
                                                             jlongArray off, jint nNodes, jintArray pathIdx,
                                                             jlongArray pathOff, jbyteArray status, jbyteArray vals,
                                                             jlongArray voff, jlongArray sizes) {
  (void)cls;
  if (klen <= 0 || nNodes < 0) {
    throw_cls(env, "java/lang/IllegalArgumentException", "verifyProofs: klen must be positive, nNodes not negative");
    return 0;
  }
  const uint64_t n = (uint64_t)len_of(env, keys) / (uint64_t)klen, nroots = (uint64_t)len_of(env, roots) / 32;
  if ((uint64_t)len_of(env, status) < n || (uint64_t)len_of(env, voff) < n + 1 ||
      (uint64_t)len_of(env, pathOff) < n + 1 || (uint64_t)len_of(env, off) < (uint64_t)nNodes + 1) {
    throw_cls(env, "java/lang/IllegalArgumentException", "verifyProofs: status / voff / pathOff / off too short");
    return 0;
  }
  Bufs b = {0};
  const uint8_t* rt = in_b(env, &b, roots);
  const uint8_t* ks = in_b(env, &b, keys);
  const uint8_t* rl = in_b(env, &b, rlp);
  const uint64_t* of = in_l(env, &b, off);
  const uint32_t* pi = in_i(env, &b, pathIdx);
  const uint64_t* po = in_l(env, &b, pathOff);
  uint8_t* st = out_buf(env, &b, status, 1);
  uint8_t* vl = out_buf(env, &b, vals, 1);
  uint64_t* vo = out_buf(env, &b, voff, 8);
  if (bufs_failed(env, &b)) return 0;
  /* the library reads rlp up to off[nNodes] and pathIdx up to pathOff[n] */
  if (of[nNodes] > (uint64_t)len_of(env, rlp) || po[n] > (uint64_t)len_of(env, pathIdx)) {
    bufs_free(&b);
    throw_cls(env, "java/lang/IllegalArgumentException", "verifyProofs: off / pathOff point past rlp / pathIdx");
    return 0;
  }
  uint64_t need = 0;
  const int rc = kh_verify_proofs(rt, nroots, ks, (uint32_t)klen, n, (uint32_t)flags, rl, of, (uint64_t)nNodes, pi, po,
                                  st, vl, (uint64_t)len_of(env, vals), vo, &need);
  if (rc == KH_OK) {
    put_b(env, status, st, n);
    put_b(env, vals, vl, need);
    put_l(env, voff, vo, n + 1);
  }
  bufs_free(&b);
  const jlong sz[1] = {(jlong)need};
  put_l(env, sizes, sz, 1);
  if (rc == KH_ENOSPC) return -1;
  if (rc != KH_OK) {
    throw_kh(env, rc);
    return 0;
  }
  return (jlong)need;
}

/* Range responses checked against their roots without a handle (kh_verify_ranges): the receiving
 * half of range + prove(KH_PROVE_TRIE_KEYS).  nr = entOff.length - 1 ranges over ONE node set
 * (nNodes encodings in enc / off): roots (32 bytes a range), origins (32 bytes a range, or null:
 * all zero), proved (a byte a range: 0 the entries claim to be the whole trie, 1 a boundary proof is
 * used), the entries' 32-byte trie keys with their values packed in vals / voff, range s holding
 * entries entOff[s] .. entOff[s + 1].  Out: status (KH_RANGE_*) and more, a byte a range, and
 * missing (32 bytes a range, or null: the absent hash of a KH_RANGE_MISSING range).  Returns the
 * number of ranges whose status is not KH_RANGE_OK. */
JNIEXPORT jlong JNICALL Java_khipu_trie_gpu_Khst_verifyRanges(JNIEnv* env, jclass cls, jbyteArray roots,
                                                             jbyteArray origins, jbyteArray proved, jbyteArray keys,
                                                             jbyteArray vals, jlongArray voff, jlongArray entOff,
                                                             jbyteArray enc, jlongArray off, jint nNodes,
                                                             jbyteArray status, jbyteArray more, jbyteArray missing) {
  (void)cls;
  /* offset arrays hold one element more than they count: never null or empty (entOff[nr] and voff[ne] are read) */
  if (len_of(env, entOff) < 1 || len_of(env, voff) < 1) {
    throw_cls(env, "java/lang/IllegalArgumentException", "verifyRanges: entOff and voff must hold at least one offset");
    return 0;
  }
  const uint64_t nr = count_of(env, entOff), ne = count_of(env, voff);
  if (nNodes < 0 || (uint64_t)len_of(env, roots) < 32 * nr || (origins && (uint64_t)len_of(env, origins) < 32 * nr) ||
      (uint64_t)len_of(env, proved) < nr || (uint64_t)len_of(env, status) < nr || (uint64_t)len_of(env, more) < nr ||
      (missing && (uint64_t)len_of(env, missing) < 32 * nr) || (uint64_t)len_of(env, off) < (uint64_t)nNodes + 1 ||
      (uint64_t)len_of(env, keys) < 32 * ne) {
    throw_cls(env, "java/lang/IllegalArgumentException", "verifyRanges: an array is too short for its ranges / entries");
    return 0;
  }
  Bufs b = {0};
  const uint8_t* rt = in_b(env, &b, roots);
  const uint8_t* og = in_b(env, &b, origins);
  const uint8_t* pv = in_b(env, &b, proved);
  const uint8_t* ks = in_b(env, &b, keys);
  const uint8_t* vs = in_b(env, &b, vals);
  const uint64_t* vo = in_l(env, &b, voff);
  const uint64_t* eo = in_l(env, &b, entOff);
  const uint8_t* en = in_b(env, &b, enc);
  const uint64_t* of = in_l(env, &b, off);
  uint8_t* st = out_buf(env, &b, status, 1);
  uint8_t* mo = out_buf(env, &b, more, 1);
  uint8_t* ms = out_buf(env, &b, missing, 1);
  if (bufs_failed(env, &b)) return 0;
  /* the library reads keys / voff up to entOff[nr], vals up to voff[ne] and enc up to off[nNodes] */
  if (eo[nr] > ne || vo[ne] > (uint64_t)len_of(env, vals) || of[nNodes] > (uint64_t)len_of(env, enc)) {
    bufs_free(&b);
    throw_cls(env, "java/lang/IllegalArgumentException", "verifyRanges: entOff / voff / off point past keys / vals / enc");
    return 0;
  }
  const int rc = kh_verify_ranges(rt, og, pv, nr, ks, vs, vo, eo, en, of, (uint64_t)nNodes, st, mo, ms);
  jlong bad = 0;
  if (rc == KH_OK) {
    for (uint64_t s = 0; s < nr; ++s) bad += st[s] != KH_RANGE_OK;
    put_b(env, status, st, nr);
    put_b(env, more, mo, nr);
    if (missing) put_b(env, missing, ms, 32 * nr);
  }
  bufs_free(&b);
  if (rc != KH_OK) {
    throw_kh(env, rc);
    return 0;
  }
  return bad;
}

/* Range responses into a partial handle (kh_trie_fill_ranges_host): the stubs inside each delivered
 * span are replaced by the subtrees built from the entries, all or nothing, kept only if no root
 * moves.  nr = entOff.length - 1 ranges: tries (an int a range; null on a single trie), roots (32
 * bytes a range, or null: no claim), origins (32 bytes a range, or null: all zero), the entries'
 * 32-byte TRIE keys (never hashed) with their values packed in vals / voff, range s holding entries
 * entOff[s] .. entOff[s + 1].  The boundary-proof nodes go to fillNodes first.  Out: status
 * (KH_RANGE_*, a byte a range), stubsLeft (a long a range, or null), gained (or null): {keys
 * gained, stubs replaced}.  Returns the number of ranges whose status is not KH_RANGE_OK: anything
 * but 0 and the handle is as it was (a KH_RANGE_MISSING range's hashes: missing). */
JNIEXPORT jlong JNICALL Java_khipu_trie_gpu_Khst_fillRanges(JNIEnv* env, jclass cls, jlong handle, jintArray tries,
                                                           jbyteArray roots, jbyteArray origins, jbyteArray keys,
                                                           jbyteArray vals, jlongArray voff, jlongArray entOff,
                                                           jbyteArray status, jlongArray stubsLeft, jlongArray gained) {
  (void)cls;
  if (len_of(env, entOff) < 1 || len_of(env, voff) < 1) {
    throw_cls(env, "java/lang/IllegalArgumentException", "fillRanges: entOff and voff must hold at least one offset");
    return 0;
  }
  const uint64_t nr = count_of(env, entOff), ne = count_of(env, voff);
  if ((tries && (uint64_t)len_of(env, tries) < nr) || (roots && (uint64_t)len_of(env, roots) < 32 * nr) ||
      (origins && (uint64_t)len_of(env, origins) < 32 * nr) || (uint64_t)len_of(env, status) < nr ||
      (stubsLeft && (uint64_t)len_of(env, stubsLeft) < nr) || (gained && len_of(env, gained) < 2) ||
      (uint64_t)len_of(env, keys) < 32 * ne) {
    throw_cls(env, "java/lang/IllegalArgumentException", "fillRanges: an array is too short for its ranges / entries");
    return 0;
  }
  Bufs b = {0};
  const uint32_t* ts = in_i(env, &b, tries);
  const uint8_t* rt = in_b(env, &b, roots);
  const uint8_t* og = in_b(env, &b, origins);
  const uint8_t* ks = in_b(env, &b, keys);
  const uint8_t* vs = in_b(env, &b, vals);
  const uint64_t* vo = in_l(env, &b, voff);
  const uint64_t* eo = in_l(env, &b, entOff);
  uint8_t* st = out_buf(env, &b, status, 1);
  uint64_t* sl = out_buf(env, &b, stubsLeft, 8);
  if (bufs_failed(env, &b)) return 0;
  /* the library reads keys / voff up to entOff[nr] and vals up to voff[ne] */
  if (eo[nr] > ne || vo[ne] > (uint64_t)len_of(env, vals)) {
    bufs_free(&b);
    throw_cls(env, "java/lang/IllegalArgumentException", "fillRanges: entOff / voff point past keys / vals");
    return 0;
  }
  uint64_t g[2] = {0, 0};
  const int rc = kh_trie_fill_ranges_host(H(handle), ts, rt, og, nr, ks, vs, vo, eo, st, sl, &g[0], &g[1]);
  jlong bad = 0;
  if (rc == KH_OK) {
    for (uint64_t s = 0; s < nr; ++s) bad += st[s] != KH_RANGE_OK;
    put_b(env, status, st, nr);
    if (stubsLeft) put_l(env, stubsLeft, sl, nr);
    if (gained) put_l(env, gained, g, 2);
  }
  bufs_free(&b);
  if (rc != KH_OK) {
    throw_kh(env, rc);
    return 0;
  }
  return bad;
}

/* ---- versions (Ledger.scala:237-271 retry / reject; TrieAccounts.rootHash; copy) ---- */
JNIEXPORT jint JNICALL Java_khipu_trie_gpu_Khst_savepoint(JNIEnv* env, jclass cls, jlong handle) {
  (void)cls;
  uint32_t depth = 0;
  const int rc = kh_trie_savepoint(H(handle), &depth);
  if (rc != KH_OK) throw_kh(env, rc);
  return (jint)depth;
}
JNIEXPORT void JNICALL Java_khipu_trie_gpu_Khst_rollback(JNIEnv* env, jclass cls, jlong handle) {
  (void)cls;
  const int rc = kh_trie_rollback(H(handle));
  if (rc != KH_OK) throw_kh(env, rc);
}
JNIEXPORT void JNICALL Java_khipu_trie_gpu_Khst_release(JNIEnv* env, jclass cls, jlong handle) {
  (void)cls;
  const int rc = kh_trie_release(H(handle));
  if (rc != KH_OK) throw_kh(env, rc);
}
JNIEXPORT jint JNICALL Java_khipu_trie_gpu_Khst_savepointDepth(JNIEnv* env, jclass cls, jlong handle) {
  (void)cls;
  uint32_t depth = 0;
  const int rc = kh_trie_savepoint_depth(H(handle), &depth);
  if (rc != KH_OK) throw_kh(env, rc);
  return (jint)depth;
}

/* TrieAccounts.rootHash of pending logs (TrieAccounts.scala:73-80): the root the batch would
 * give, the handle unchanged */
JNIEXPORT jbyteArray JNICALL Java_khipu_trie_gpu_Khst_rootOf(JNIEnv* env, jclass cls, jlong handle, jbyteArray upKeys,
                                                            jbyteArray upVals, jlongArray upVoff, jbyteArray delKeys,
                                                            jint klen, jint flags) {
  (void)cls;
  const uint64_t nup = count_of(env, upVoff), ndel = klen > 0 ? (uint64_t)(len_of(env, delKeys) / klen) : 0;
  uint8_t root[32];
  Bufs b = {0};
  const uint8_t* k = in_b(env, &b, upKeys);
  const uint8_t* v = in_b(env, &b, upVals);
  const uint64_t* o = in_l(env, &b, upVoff);
  const uint8_t* d = in_b(env, &b, delKeys);
  if (bufs_failed(env, &b)) return NULL;
  const int rc = kh_trie_root_of_host(H(handle), k, v, o, nup, d, ndel, (uint32_t)klen, (uint32_t)flags, root, NULL);
  bufs_free(&b);
  if (rc != KH_OK) {
    throw_kh_commit(env, rc, H(handle), NULL);
    return NULL;
  }
  return bytes_of(env, root, 32);
}

/* MerklePatriciaTrie.copy (MerklePatriciaTrie.scala:556): a new handle (free it with free) */
JNIEXPORT jlong JNICALL Java_khipu_trie_gpu_Khst_copy(JNIEnv* env, jclass cls, jlong handle) {
  (void)cls;
  kh_trie* out = NULL;
  const int rc = kh_trie_copy(H(handle), &out);
  if (rc != KH_OK) {
    throw_kh(env, rc);
    return 0;
  }
  return (jlong)(intptr_t)out;
}

/* ---- memory of a resident handle ---- */
/* usageOut (long[6]): records, live records, heap bytes, live heap bytes, map slots, HBM bytes */
JNIEXPORT void JNICALL Java_khipu_trie_gpu_Khst_usage(JNIEnv* env, jclass cls, jlong handle, jlongArray usageOut) {
  (void)cls;
  kh_trie_usage_t u;
  const int rc = kh_trie_usage(H(handle), &u);
  if (rc != KH_OK) {
    throw_kh(env, rc);
    return;
  }
  const jlong v[6] = {(jlong)u.records,         (jlong)u.live_records, (jlong)u.heap_bytes,
                      (jlong)u.live_heap_bytes, (jlong)u.map_slots,    (jlong)u.hbm_bytes};
  put_l(env, usageOut, v, 6);
}
/* rewrite the live records densely between blocks (no savepoint open); beforeOut (long[2],
 * nullable): records / heap bytes before */
JNIEXPORT void JNICALL Java_khipu_trie_gpu_Khst_compact(JNIEnv* env, jclass cls, jlong handle, jlongArray beforeOut) {
  (void)cls;
  kh_trie_usage_t u;
  const int rc = kh_trie_compact(H(handle), &u);
  if (rc != KH_OK) {
    throw_kh(env, rc);
    return;
  }
  const jlong v[2] = {(jlong)u.records, (jlong)u.heap_bytes};
  put_l(env, beforeOut, v, 2);
}
JNIEXPORT jlong JNICALL Java_khipu_trie_gpu_Khst_size(JNIEnv* env, jclass cls, jlong handle) {
  (void)cls;
  uint64_t n = 0;
  const int rc = kh_trie_size(H(handle), &n);
  if (rc != KH_OK) throw_kh(env, rc);
  return (jlong)n;
}
/* Free the handle held in handleBox[0] and zero it there: idempotent (the library cannot guard
 * a raw pointer, so the box is what makes a second close or a finalizer harmless).  The
 * wrapper is not itself reentrant for one box: the Scala owner closes from one thread. */
JNIEXPORT void JNICALL Java_khipu_trie_gpu_Khst_free(JNIEnv* env, jclass cls, jlongArray handleBox) {
  (void)cls;
  if (!handleBox || len_of(env, handleBox) < 1) return;
  jlong h = 0;
  (*env)->GetLongArrayRegion(env, handleBox, 0, 1, &h);
  if (!h) return;
  const jlong zero = 0;
  (*env)->SetLongArrayRegion(env, handleBox, 0, 1, &zero); /* zeroed before the free: never freed twice */
  const int rc = kh_trie_free(H(h));
  if (rc != KH_OK) throw_kh(env, rc);
}
