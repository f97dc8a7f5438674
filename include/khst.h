/*
 * khst — MI355X batch state-root engine for khipu's Merkle-Patricia trie.
 * C ABI of libkhst.so (khipu_amd/libkhst.so).  Plain pointers and sizes only.
 *
 * Every entry point replaces a reference interface on the state-root path
 * (paths relative to /root/reference/khipu-base/src/main/scala/khipu/ unless
 * they start with khipu-eth/):
 *
 *   kh_kec256_batch         crypto.kec256(Array[Byte]*)            crypto/package.scala:37-47
 *                           (one call per message today; here one call per batch,
 *                           e.g. NodeDatasRequest.processResponse,
 *                           khipu-eth/.../blockchain/sync/package.scala:88-90)
 *   kh_trie_root            foldLeft(put) + rootHash over a fresh trie:
 *                           MerklePatriciaTrie.put/rootHash  trie/MerklePatriciaTrie.scala:78,157-281
 *                           as driven by TrieAccounts.flush   khipu-eth/.../ledger/TrieAccounts.scala:22-28
 *                           and GenesisDataLoader             khipu-eth/.../blockchain/data/GenesisDataLoader.scala:139-147
 *   kh_trie_roots_segmented many independent tries (TrieStorage.flush per contract,
 *                           khipu-eth/.../ledger/TrieStorage.scala:52-60; BlockWorldState.scala:243-252)
 *   kh_trie_root_nodes      rootHash + the write-back node set of MerklePatriciaTrie.changes/persist
 *                           (MerklePatriciaTrie.scala:491-516,544-554 -> NodeStorage.update,
 *                           khipu-eth/.../storage/NodeStorage.scala:16-19)
 *   kh_trie_roots_varkeys   generic unhashed keys of any length <= 32 B, branch values
 *   kh_list_roots           transactions / receipts roots (MptListValidator.scala:15-46)
 *   kh_trie_root_sharded    the same root computed from per-GPU top-nibble shards
 *   kh_trie_nodes_by_hash   Blockchain.getMptNodeByHash for HostService's GetNodeData
 *                           (khipu-eth/.../domain/Blockchain.scala:356-357, HostService.scala:103-112)
 *   kh_trie_export_nodes    the node store of a resident trie's current version (checkpoint; the
 *                           resume half is kh_trie_open_nodes)
 *   kh_forest_load_nodes    MerklePatriciaTrie(account.stateRoot, storageSource) for many contracts
 *                           at once (MerklePatriciaTrie.scala:60-66,520-542): storage tries paged
 *                           into a resident forest by (trie id, storage root), or a whole forest
 *                           resumed from a checkpoint; kh_forest_roots lists what is resident,
 *                           kh_forest_evict drops cold tries again
 *   kh_trie_open_partial    the lazy getNode of MerklePatriciaTrie(rootHash, source)
 *                           (MerklePatriciaTrie.scala:60-66,520-542): a trie opened from the nodes at
 *                           hand (a block's witness), the subtrees it lacks kept as stubs; a commit
 *                           that needs one returns KH_ENODE where the reference throws
 *                           MPTNodeMissingException, kh_trie_missing names the hashes and
 *                           kh_trie_fill_nodes takes the fetched nodes (kh_forest_load_partial: the
 *                           same for many storage tries)
 *   kh_trie_prove           the nodes MerklePatriciaTrie.get visits (MerklePatriciaTrie.scala:90-147)
 *                           for a batch of keys: an eth_getProof answer, or a block's witness
 *   kh_verify_proofs        that walk re-done from a root over the listed nodes alone
 *   kh_trie_diff_host       the keys two resident tries differ in (a parent state kept as a
 *                           kh_trie_copy against the trie the blocks were committed on): the
 *                           (upserts, deletes) of the kh_trie_apply that brings one to the other
 *   kh_trie_diffs_host      the same for many trie pairs of two forests in one call: every storage
 *                           trie a block touched, under one budget
 *   kh_verify_ranges        range responses (a page of kh_trie_range_host with its two boundary proofs,
 *                           or whole small tries) checked against their roots without a handle: nothing
 *                           left out between origin and the last key (no reference counterpart: khipu
 *                           syncs node by node; the contract is snap's, geth's VerifyRangeProof)
 *
 * Semantics shared by every trie entry point:
 *   - input i is a put(key_i, value_i); later inputs overwrite earlier ones with the
 *     same key (the foldLeft order of TrieAccounts.flush);
 *   - keys are `klen` bytes each; with KH_HASH_KEYS the trie key is kec256(key)
 *     (Address.hashedAddressEncoder, khipu-eth/.../domain/Address.scala:15-17;
 *     trie/package.scala:34-36), otherwise klen must be 32 (already keccak'd);
 *   - values are the serialised bytes (vSerializer.toBytes), packed: value i is
 *     vals[voff[i] .. voff[i+1]);
 *   - the root is kec256(encoding of the root node) even when that encoding is
 *     shorter than 32 bytes (MerklePatriciaTrie.scala:169); an empty trie has root
 *     EMPTY_TRIE_HASH = kec256(0x80) (trie/package.scala:41).
 *
 * Errors: int status; message via kh_last_error() (thread-local).  KH_EDEVICE means
 * the GPU path failed; the caller decides what to do (there is no silent fallback).
 * Threading: every call is reentrant.  Host entry points share one lazily created
 * device context per device; every call that uses a context holds its (recursive) mutex
 * for the call, and every call on a resident handle (kh_trie / forest) holds the mutex of
 * the context the handle was opened on, so calls on handles of one context from many
 * threads are serialised (a thread reading one handle's write-back set waits for another
 * thread's commit on the same context to finish, never for anything else).  A commit
 * whose in-flight tail (records, anchor map) fails leaves its handle refusing every call
 * but kh_trie_rollback (to a savepoint opened before it) and kh_trie_free.
 */
#ifndef KHST_H
#define KHST_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KH_OK 0
#define KH_EINVAL -1     /* bad argument (RLPException / MPTException analogue) */
#define KH_ENOMEM -2     /* device allocation failed */
#define KH_EDEVICE -3    /* HIP runtime / kernel failure, or no device */
#define KH_ENODE -4      /* missing node (MPTNodeMissingException analogue) */
#define KH_EINTERNAL -5
#define KH_ENOSPC -6     /* caller's output buffer too small; required sizes returned */

/* flags */
#define KH_HASH_KEYS 0x1u   /* trie key = kec256(input key) */
#define KH_EMIT_NODES 0x2u  /* resident tries: keep each commit's write-back set (kh_trie_emit_nodes) */
#define KH_SHARD_RCCL 0x4u  /* kh_trie_root_sharded: exchange over RCCL even when a device repeats (needs a
                               communicator that accepts repeats, such as the tests' loopback) */
typedef struct kh_ctx kh_ctx;
#define KH_NO_TRIE 0xFFFFFFFFu  /* kh_block_commit: an account upsert without a storage trie */

typedef struct kh_stats {
  uint64_t n_inputs;       /* puts received */
  uint64_t n_leaves;       /* distinct keys (leaves) */
  uint64_t n_branches;
  uint64_t n_extensions;
  uint64_t n_inline;       /* nodes embedded in their parent (encoding < 32 B) */
  uint64_t n_node_hashes;  /* Keccak-256 of node encodings >= 32 B, plus one per root */
  uint64_t n_node_perms;   /* Keccak-f[1600] permutations spent on node encodings */
  uint64_t n_key_perms;    /* permutations spent hashing keys (KH_HASH_KEYS) */
  uint64_t arena_bytes;    /* bytes of node RLP produced */
  uint32_t n_levels;       /* bottom-up branch levels launched */
  uint32_t full_sort;      /* 1 if the 64-bit-prefix sort had ties and a full-key sort ran */
  double t_total_ms;       /* device time of the whole build (HIP events) */
  double t_keys_ms;        /* key hashing */
  double t_sort_ms;        /* radix sort + gather + dedup */
  double t_topo_ms;        /* LCP + topology */
  double t_leaf_ms;        /* leaf encode + hash */
  double t_branch_ms;      /* all branch levels */
  uint32_t reserved0;      /* 0 (kept for the layout the JNI shim and ctypes mirror) */
  uint32_t reserved;
} kh_stats;

const char* kh_last_error(void);
const char* kh_version(void);
int kh_device_count(void);

/* Batched kec256 over n messages packed as data[off[i] .. off[i+1]).  Host buffers. */
int kh_kec256_batch(const uint8_t* data, const uint64_t* off, uint64_t n, uint8_t* out32);

/* Root of the trie holding puts (key_i, val_i), i < n.  Host buffers. */
int kh_trie_root(const uint8_t* keys, uint32_t klen, const uint8_t* vals, const uint64_t* voff, uint64_t n,
                 uint32_t flags, uint8_t root32[32], kh_stats* stats);

/* nseg independent tries; trie s holds inputs seg_off[s] .. seg_off[s+1).  roots32: nseg*32 bytes. */
int kh_trie_roots_segmented(const uint8_t* keys, uint32_t klen, const uint8_t* vals, const uint64_t* voff,
                            const uint64_t* seg_off, uint64_t nseg, uint32_t flags, uint8_t* roots32,
                            kh_stats* stats);

/* Tries over variable-length unhashed keys of 0..32 bytes (key i = keys[koff[i] ..
 * koff[i+1])): a key that is a prefix of other keys is the value of the branch where it
 * ends (the branch's 17th item, Node.scala:31-40).  nseg tries as in
 * kh_trie_roots_segmented (koff / voff indexed like the inputs).  The generic key path
 * of MerklePatriciaTrie.put with an identity key serializer (trie/package.scala:28-36). */
int kh_trie_roots_varkeys(const uint8_t* keys, const uint64_t* koff, const uint8_t* vals, const uint64_t* voff,
                          const uint64_t* seg_off, uint64_t nseg, uint8_t* roots32, kh_stats* stats);

/* List tries (transactions / receipts / ommers roots): item i of trie s, i.e. input
 * seg_off[s] + i, is put under key rlp(i) (MptListValidator.isValid,
 * khipu-eth/.../validators/MptListValidator.scala:15-46; BlockGenerator.scala:157-163);
 * items[off[j] .. off[j+1]) is the serialized item.  Keys are made on the device. */
int kh_list_roots(const uint8_t* items, const uint64_t* off, const uint64_t* seg_off, uint64_t nseg,
                  uint8_t* roots32, kh_stats* stats);

/* kh_trie_roots_segmented over ngpus GPUs of this process (SURVEY §8e, configs[3]): the
 * tries are split into contiguous ranges of about equal slot counts, one per device (a
 * device may repeat), each built as one segmented build; roots32 receives every trie's
 * root in order.  The tries are independent: no data moves between the GPUs. */
int kh_trie_roots_segmented_sharded(const int* devices, int ngpus, const uint8_t* keys, uint32_t klen,
                                    const uint8_t* vals, const uint64_t* voff, const uint64_t* seg_off, uint64_t nseg,
                                    uint32_t flags, uint8_t* roots32, kh_stats* stats);

/* The kh_trie_root result computed on ngpus GPUs of this process: the
 * puts are split into ngpus contiguous slices, slice g staged to devices[g], keys hashed
 * there, records routed to the owner of their top key nibble (q * ngpus >> 4) over RCCL
 * point-to-point (xGMI), every owner builds its subtries from nibble 1, and the 16
 * references are folded into the root branch.  Devices must be distinct for the RCCL
 * exchange; a list that repeats a device runs several shards on it (device copies).
 * The keys are exchanged first; the value lengths and bytes follow on a stream of their
 * own while every owner sorts its keys and derives the topology.
 * stats: sums over the shards; t_keys_ms / t_sort_ms / t_total_ms are the host wall
 * times of stage+hash+partition / key exchange / the whole call.  Host buffers. */
int kh_trie_root_sharded(const int* devices, int ngpus, const uint8_t* keys, uint32_t klen, const uint8_t* vals,
                         const uint64_t* voff, uint64_t n, uint32_t flags, uint8_t root32[32], kh_stats* stats);

/* kh_list_roots with the items in HBM: d_off holds the offsets of every item of the call
 * into d_items (item j at d_items[d_off[j] .. d_off[j+1]), j from h_seg_off[0]); the
 * segment offsets are host memory. */
int kh_dev_list_roots(kh_ctx* ctx, const uint8_t* d_items, const uint64_t* d_off, const uint64_t* h_seg_off,
                      uint64_t nseg, uint8_t* roots32, kh_stats* stats);

/* Root plus every node a fresh node store needs: each node reachable from the root
 * whose encoding is >= 32 B, plus the root node (MerklePatriciaTrie.scala:505-511).
 * Node j: hash hashes32[32j..), encoding rlp[off[j] .. off[j+1]) (off has n_nodes+1
 * entries).  Nodes are ordered leaves first, then branches/extensions bottom-up, the
 * root last.  On KH_ENOSPC, *n_nodes and *rlp_len report the sizes needed. */
int kh_trie_root_nodes(const uint8_t* keys, uint32_t klen, const uint8_t* vals, const uint64_t* voff, uint64_t n,
                       uint32_t flags, uint8_t root32[32], uint8_t* hashes32, uint64_t node_cap, uint8_t* rlp,
                       uint64_t rlp_cap, uint64_t* off, uint64_t* n_nodes, uint64_t* rlp_len, kh_stats* stats);

/* ---- device-resident interface (inputs already in HBM; used by bench.py and the
 *      multi-GPU driver).  One context per device; a context is not shared across
 *      threads without external synchronisation. ---- */

int kh_ctx_create(int device, kh_ctx** out);
int kh_ctx_destroy(kh_ctx* ctx);
/* Use an existing HIP stream (hipStream_t passed as void*); NULL = the context's own stream. */
int kh_ctx_set_stream(kh_ctx* ctx, void* hip_stream);

int kh_dev_kec256_batch(kh_ctx* ctx, const uint8_t* d_data, const uint64_t* d_off, uint64_t n, uint8_t* d_out32);

/* Build over device inputs.  depth0 = 0: one trie (or one per segment when d_seg is
 * non-NULL: d_seg[i] = segment id of input i, ids < nseg).  depth0 = 1, d_seg NULL:
 * the 16 top-nibble subtries of one trie, paths starting at nibble 1 (the shard
 * unit of the multi-GPU path).  Per result r (nseg or 16 of them):
 *   h_hash32[32r..)  kec256 of the top node's encoding (the root for depth0 = 0);
 *   h_enc_len[r]     that encoding's length (0 = empty);
 *   h_inline32[32r..) the encoding itself when shorter than 32 B (capped reference).
 * Outputs are host buffers; h_inline32 may be NULL. */
int kh_dev_trie_build(kh_ctx* ctx, const uint8_t* d_keys, uint32_t klen, const uint8_t* d_vals,
                      const uint64_t* d_voff, uint64_t n, const uint32_t* d_seg, uint64_t nseg, uint32_t depth0,
                      uint32_t flags, uint8_t* h_hash32, uint32_t* h_enc_len, uint8_t* h_inline32,
                      kh_stats* stats);

/* kh_dev_trie_build whose values arrive later (the multi-GPU exchange): the keys must be
 * in place when it is called; d_vals / d_voff are read only after the HIP event
 * vals_ready (a hipEvent_t recorded on any stream of the context's device; NULL = ready)
 * has completed, so the key sort and the branch topology run while the values are
 * still in flight. */
int kh_dev_trie_build_ev(kh_ctx* ctx, void* vals_ready, const uint8_t* d_keys, uint32_t klen,
                         const uint8_t* d_vals, const uint64_t* d_voff, uint64_t n, const uint32_t* d_seg,
                         uint64_t nseg, uint32_t depth0, uint32_t flags, uint8_t* h_hash32, uint32_t* h_enc_len,
                         uint8_t* h_inline32, kh_stats* stats);

/* Fold 16 capped top-nibble references (as produced by kh_dev_trie_build with depth0 = 1,
 * gathered from every shard) into the root: kec256(RLP[ref_0..ref_15, ""]).
 * Requires >= 2 non-empty references (otherwise the root is not a branch: returns KH_EINVAL
 * and the caller builds on one device). */
int kh_fold_root16(const uint8_t* hash32x16, const uint32_t* enc_len16, const uint8_t* inline32x16,
                   uint8_t root32[32]);

/* kec256 of n keys of klen bytes (device buffers; the KH_HASH_KEYS step on its own). */
int kh_dev_hash_keys(kh_ctx* ctx, const uint8_t* d_keys, uint32_t klen, uint64_t n, uint8_t* d_out32);

/* Multi-GPU routing: stable partition of n records (32-byte trie keys + packed values) by
 * owner = top nibble * nparts / 16 (nparts <= 16).  Writes the records grouped by owner
 * (input order kept inside a group, so later puts still win after the exchange):
 * d_out_keys (n*32 B), d_out_vals (total value bytes), d_out_vlen (n value lengths);
 * h_counts[p] / h_bytes[p] = records / value bytes for owner p (host).  d_keys32, d_voff,
 * d_out_keys, d_out_vals and d_out_vlen must be 8-byte aligned (KH_EINVAL otherwise). */
int kh_dev_partition(kh_ctx* ctx, const uint8_t* d_keys32, const uint8_t* d_vals, const uint64_t* d_voff,
                     uint64_t n, uint32_t nparts, uint8_t* d_out_keys, uint8_t* d_out_vals, uint64_t* d_out_vlen,
                     uint64_t* h_counts, uint64_t* h_bytes);
/* The same with the value copy deferred: it returns once the keys, the lengths, the counts
 * and the bytes per owner are in place, the value bytes still being copied on the context's stream;
 * vals_done (a hipEvent_t of the context's device) is recorded after them.  NULL
 * vals_done: kh_dev_partition. */
int kh_dev_partition_ev(kh_ctx* ctx, void* vals_done, const uint8_t* d_keys32, const uint8_t* d_vals,
                        const uint64_t* d_voff, uint64_t n, uint32_t nparts, uint8_t* d_out_keys,
                        uint8_t* d_out_vals, uint64_t* d_out_vlen, uint64_t* h_counts, uint64_t* h_bytes);
/* kh_dev_hash_keys and kh_dev_partition_ev in one call: the n klen-byte keys (addresses)
 * are kec256'd in a pass that also writes each key's owner as a byte, so the count pass
 * reads those bytes instead of the hashed keys (what the sharded step runs at N > 1).  Same outputs as kh_dev_partition_ev over
 * kh_dev_hash_keys(d_keys) (the hashed keys are written only to d_out_keys, grouped). */
int kh_dev_hash_partition_ev(kh_ctx* ctx, void* vals_done, const uint8_t* d_keys, uint32_t klen,
                             const uint8_t* d_vals, const uint64_t* d_voff, uint64_t n, uint32_t nparts,
                             uint8_t* d_out_keys, uint8_t* d_out_vals, uint64_t* d_out_vlen, uint64_t* h_counts,
                             uint64_t* h_bytes);

/* ---- fast-sync NodeData verification ----
 * NodeDatasRequest.processResponse (sync/package.scala:81-125) over a batch of peer
 * values: kec256 each value (data packed, off[n+1]), match it against the nreq
 * requested hashes (req32, req_kind[r]: 0 state trie node, 1 storage root, 2 contract
 * storage node, 3 EVM code; a duplicate hash takes the last request's kind), and
 * decode a matched trie node with PV63's MptNode rules (PV63.scala:96-127) to list the
 * children still to fetch: getStateNodeChildren / getContractMptNodeChildren
 * (sync/package.scala:127-165) — branch / extension child hashes, and for a state
 * leaf the account's codeHash (kind 3) then stateRoot (kind 1) unless empty.
 * Per value i (host buffers; any output may be NULL):
 *   hash32[32i..)          kec256(value)
 *   match[i]               matched request index, -1 if none (then nothing is decoded)
 *   status[i]              0 ok, 1 not a trie node ("Cannot decode NodeData"),
 *                          2 bad child ("unexpected value in node"), 3 bad account
 *                          ("Cannot decode Account"), 4 malformed RLP
 *   nchild[i], child32[512i..), child_kind[16i..)   children in the reference's order */
int kh_verify_nodes(const uint8_t* data, const uint64_t* off, uint64_t n, const uint8_t* req32, const uint8_t* req_kind,
                    uint64_t nreq, uint8_t* hash32, int64_t* match, uint8_t* status, uint8_t* nchild, uint8_t* child32,
                    uint8_t* child_kind);
/* The same with the children packed, as processResponse concatenates them (childHashes :::
 * hashes): value i's children are child32[32k..) / child_kind[k] for k in
 * [child_off[i], child_off[i+1]) (child_off has n+1 entries); *n_children = the total.  When
 * the total exceeds child_cap (16 n always suffices) the call returns KH_ENOSPC after writing
 * every other output, child_off and *n_children. */
int kh_verify_nodes_packed(const uint8_t* data, const uint64_t* off, uint64_t n, const uint8_t* req32,
                           const uint8_t* req_kind, uint64_t nreq, uint8_t* hash32, int64_t* match, uint8_t* status,
                           uint64_t* child_off, uint8_t* child32, uint8_t* child_kind, uint64_t child_cap,
                           uint64_t* n_children);

/* ---- resident tries and forests: incremental commit ----
 * A trie kept in HBM between commits as node records found by their anchor (trie id,
 * depth, key prefix): khipu_amd/csrc/forest.h.  Replaces the per-key fold of
 * TrieAccounts.flush / TrieStorage.flush (TrieAccounts.scala:22-28, TrieStorage.scala:43-60)
 * over MerklePatriciaTrie.put / remove (MerklePatriciaTrie.scala:157-281, 290-477): a commit
 * opens only the nodes on the changed keys' paths and rebuilds them (with the canonical
 * `fix` collapse of :430-477), O(dirty keys x depth) work.  A FOREST holds many tries
 * (contract storage tries, BlockWorldState.scala:243-252) in one handle, each op tagged
 * with its trie id; one commit re-roots every trie the block touched.  Device-buffer
 * entry points use the handle's context stream (one thread at a time per handle); the
 * _host variants take host buffers (what the JNI shim binds).
 * Semantics of a commit: nup upserts then ndel deletes, the last op on a key winning;
 * deleting an absent key is a no-op; keys are klen bytes (32, or any with KH_HASH_KEYS,
 * which must match the flag the trie was opened with). */
typedef struct kh_trie kh_trie;

/* Open a trie from n records (duplicates: the later wins).  flags: KH_HASH_KEYS, KH_EMIT_NODES. */
int kh_trie_open(kh_ctx* ctx, const uint8_t* d_keys, uint32_t klen, const uint8_t* d_vals, const uint64_t* d_voff,
                 uint64_t n, uint32_t flags, uint8_t root32[32], kh_trie** out);
int kh_trie_open_host(const uint8_t* keys, uint32_t klen, const uint8_t* vals, const uint64_t* voff, uint64_t n,
                      uint32_t flags, uint8_t root32[32], kh_trie** out);

/* Open a trie from its root hash and a node store: MerklePatriciaTrie.apply(
 * rootHash, source) with getNode (MerklePatriciaTrie.scala:60-66,520-542).  The store holds
 * n node encodings enc[off[i] .. off[i+1]), keyed by their kec256 (content addressed, as
 * NodeStorage is); the nodes reachable from root32 are decoded on the device.  The open is
 * kh_forest_load_nodes (below) of the one trie into a fresh handle, so that call's rules hold:
 *   - KH_EINVAL for a store node on the walk that is not a canonical secure-trie node, by the
 *     rules of Node.nodeDec and HexPrefix.decode for a 64-nibble key: a branch value anywhere but
 *     a value-only branch at depth 64, an embedded node of 32 B or more, a path past nibble 64, a
 *     HexPrefix flag nibble above 3, a non-zero pad nibble, a branch with children starting at
 *     nibble 64, ...; also for n >= 2^31;
 *   - KH_ENODE for a node missing from the store (MPTNodeMissingException), with one hash in
 *     missing32: the first missing one in frontier order of the first round that lacks any (the
 *     root is round 0; then children in nibble order).  The same store and root report the same
 *     hash every time;
 *   - the records come in the load's fixed order, so two opens of the same store give the same
 *     kh_trie_export_nodes order.
 * EMPTY_TRIE_HASH opens an empty trie, whatever the store holds.  A failed open leaves no handle.
 * Device form: d_off non-decreasing (a precondition); the _host form checks that (KH_EINVAL)
 * before it stages anything. */
int kh_trie_open_nodes(kh_ctx* ctx, const uint8_t root32[32], const uint8_t* d_enc, const uint64_t* d_off, uint64_t n,
                       uint32_t flags, uint8_t missing32[32], kh_trie** out);
int kh_trie_open_nodes_host(const uint8_t root32[32], const uint8_t* enc, const uint64_t* off, uint64_t n,
                            uint32_t flags, uint8_t missing32[32], kh_trie** out);

/* One commit; root32 receives the new root.  stats: n_node_hashes counts the nodes re-hashed.
 * A handle without KH_EMIT_NODES returns once the new roots are on the host: the commit's
 * record and anchor-map writes finish on the library's stream after it (every later call on
 * the handle is ordered after them; an internal failure there surfaces at the next call). */
int kh_trie_apply(kh_trie* h, const uint8_t* d_up_keys, const uint8_t* d_up_vals, const uint64_t* d_up_voff,
                  uint64_t nup, const uint8_t* d_del_keys, uint64_t ndel, uint32_t klen, uint32_t flags,
                  uint8_t root32[32], kh_stats* stats);
int kh_trie_apply_host(kh_trie* h, const uint8_t* up_keys, const uint8_t* up_vals, const uint64_t* up_voff,
                       uint64_t nup, const uint8_t* del_keys, uint64_t ndel, uint32_t klen, uint32_t flags,
                       uint8_t root32[32], kh_stats* stats);

/* A forest of tries (empty).  ctx NULL: the shared context of the current device, the one
 * the *_host entry points use (so kh_block_commit_host can pair it with a trie opened by
 * kh_trie_open_host).  Each op names its trie (any uint32 id).  After a commit,
 * h_tries / h_roots32 receive the touched tries (ascending ids) and their new roots
 * (EMPTY_TRIE_HASH for a trie left empty); KH_ENOSPC with *n_tries when cap is short. */
int kh_forest_open(kh_ctx* ctx, uint32_t flags, kh_trie** out);
int kh_forest_apply(kh_trie* f, const uint32_t* d_up_trie, const uint8_t* d_up_keys, const uint8_t* d_up_vals,
                    const uint64_t* d_up_voff, uint64_t nup, const uint32_t* d_del_trie, const uint8_t* d_del_keys,
                    uint64_t ndel, uint32_t klen, uint32_t* h_tries, uint8_t* h_roots32, uint64_t cap,
                    uint64_t* n_tries, kh_stats* stats);
int kh_forest_apply_host(kh_trie* f, const uint32_t* up_trie, const uint8_t* up_keys, const uint8_t* up_vals,
                         const uint64_t* up_voff, uint64_t nup, const uint32_t* del_trie, const uint8_t* del_keys,
                         uint64_t ndel, uint32_t klen, uint32_t* h_tries, uint8_t* h_roots32, uint64_t cap,
                         uint64_t* n_tries, kh_stats* stats);

/* The touched tries and roots of a forest's last commit (also after kh_block_commit). */
int kh_forest_last_roots(kh_trie* f, uint32_t* h_tries, uint8_t* h_roots32, uint64_t cap, uint64_t* n_tries);

/* ---- forest load, roots and eviction: the working set of storage tries paged in and out ----
 * MerklePatriciaTrie(account.stateRoot, storageSource) per contract (MerklePatriciaTrie.scala:
 * 60-66,520-542), batched: k tries (id tries[j], root roots32[32j..), host arrays) are decoded
 * from one node store (the layout of kh_trie_open_nodes: n encodings, content addressed; it may
 * hold unrelated nodes and duplicates) into the forest, beside the tries it holds.  A node two
 * listed tries share is decoded once per trie.  A root equal to EMPTY_TRIE_HASH loads nothing.
 * All or nothing: on any error the forest is exactly as before.
 *   KH_EINVAL, before anything is decoded: not a forest; an id listed twice; an id that is already
 *     resident; k or n >= 2^31.  While decoding: a node that is not a canonical secure-trie node (a
 *     branch value anywhere but a value-only branch at depth 64, an embedded node of 32 B or more, a
 *     path past nibble 64, ...), or a load that would pass 2^32 - 2 records.
 *   KH_ENODE: the walk is level-synchronous (the roots are round 0) and stops after the first
 *     round in which a hash reference is absent from the store; every missing reference of that
 *     round is reported, one entry per reference: miss_idx[e] = the list index j, miss32[32e..)
 *     the hash.  *n_missing = their number; at most miss_cap entries are written (any miss_cap of
 *     them).  The caller fetches them and retries.
 * Records are appended in a fixed order (round by round; in a round in frontier order, children
 * in nibble order, the roots in list order): the same load into two fresh forests gives the same
 * kh_trie_export_nodes order.  A successful load ends every export cursor, adds the loaded keys to
 * kh_trie_size, and leaves the last commit's roots and write-back set as they were (a load creates
 * no node).  With a savepoint open the load is journaled: kh_trie_rollback makes the loaded tries
 * non-resident again, kh_trie_release keeps them.
 * Device form: d_enc / d_off on the handle's context, d_off non-decreasing (a precondition); the
 * _host form checks that (KH_EINVAL) before it stages them.  stats (nullable): n_inputs = k,
 * n_leaves = the forest's keys, n_levels = the rounds, n_node_hashes = the store's nodes (each is
 * hashed), t_total_ms = t_sort_ms (the list checks, store hashing and sort) + t_branch_ms (the
 * rounds) + t_topo_ms (the anchor map). */
int kh_forest_load_nodes(kh_trie* f, const uint32_t* tries, const uint8_t* roots32, uint64_t k,
                         const uint8_t* d_enc, const uint64_t* d_off, uint64_t n,
                         uint32_t* miss_idx, uint8_t* miss32, uint64_t miss_cap, uint64_t* n_missing,
                         kh_stats* stats);
int kh_forest_load_nodes_host(kh_trie* f, const uint32_t* tries, const uint8_t* roots32, uint64_t k,
                              const uint8_t* enc, const uint64_t* off, uint64_t n,
                              uint32_t* miss_idx, uint8_t* miss32, uint64_t miss_cap, uint64_t* n_missing,
                              kh_stats* stats);
/* ---- partial handles: open from a witness, commit along the resident paths, fill what is missing
 * MerklePatriciaTrie(rootHash, source) loads a node only when a get, put or remove walks into it
 * (MerklePatriciaTrie.scala:60-66,520-542) and throws MPTNodeMissingException for a node its source
 * lacks; the caller fetches that node and retries.  Here a handle may hold a trie PARTLY: a
 * subtree whose node is absent from the store it was opened from is kept as a STUB, a record that
 * stands for the subtree and remembers the reference its parent holds and the hash of the node to
 * fetch.  An extension whose branch is absent is one stub with its branch: the stub still stands
 * for the extension (it is exported, proved and served by hash) and asks for the branch.  An
 * embedded node (< 32 B) is part of its parent and never a stub; a trie's root node is never a stub.
 *
 * kh_trie_open_partial / kh_forest_load_partial take the arguments and argument checks of
 * kh_trie_open_nodes / kh_forest_load_nodes and differ in this: a hash reference below a root that
 * is absent from the store makes a stub instead of ending the round.  A missing ROOT is still
 * KH_ENODE, reported as there, and nothing is loaded for any listed trie.  All or nothing, the
 * fixed record order, the journaling under a savepoint and the end of export cursors carry over.
 * kh_trie_size counts the keys the handle holds (leaves and value-only branches);
 * kh_trie_stubs the live stubs, exactly.  A handle without stubs behaves in every call as one
 * opened in full.
 *
 * Commits (kh_trie_apply, kh_forest_apply, kh_block_commit, kh_trie_root_of and their _host forms)
 * on a handle with stubs:
 *   - an untouched stub under a branch the commit opens is carried as it is: its parent's new
 *     encoding holds the reference the stub keeps.  So a put into an empty slot of a branch whose
 *     other children are all stubs commits with no fetch;
 *   - an op whose walk reaches a stub, and a delete that leaves a stub as its parent's only child
 *     (the reference's fix loads that child, MerklePatriciaTrie.scala:430-477), need a missing
 *     node: the commit returns KH_ENODE and the handle is exactly as before -- root, values, last
 *     roots, write-back set and export bytes.  Every stub any op of the batch reached is reported
 *     by that one refusal (the collapsing ones are found, and reported, only once no op reaches a
 *     stub any more);
 *   - an op that leaves the path inside an extension whose branch is a stub does not need the
 *     branch, as in the reference: the extension is split over the branch's hash;
 *   - a successful commit never creates or removes a stub, and moves none but this one: a stub
 *     that stands for the branch under an extension the store did hold is re-anchored when that
 *     extension is split or its parent collapses -- the extension is re-cut over the branch's
 *     hash, which is all the reference's put and fix read of it.
 * kh_trie_missing: the distinct (trie id, hash to fetch) pairs of the most recent commit, block
 * commit or root_of on the handle (trie id 0 on a single trie); empty unless that call returned
 * KH_ENODE for missing nodes; order unspecified; KH_ENOSPC with *n when cap is short (with cap 0,
 * the size query, kh_last_error keeps the refused commit's message).  After a block commit each of
 * the two handles holds its own list.
 *
 * kh_trie_fill_nodes: the live stubs whose node is in the store (the store layout of
 * kh_trie_open_nodes) are resolved, in the load's rounds; the children a resolved node refers to
 * and the store lacks become stubs in turn, nodes no stub names are ignored.  All or nothing: a
 * malformed node is KH_EINVAL and the handle is as before.  KH_EINVAL while a savepoint is open
 * (as kh_trie_compact).  Ends export cursors.  *n_decoded (nullable) = the store nodes decoded
 * into the handle.
 *
 * Reads: kh_trie_get gives found = KH_FOUND_UNKNOWN (empty value) for a key whose walk reaches a
 * stub, and so does kh_trie_prove, whose proof for such a key is the resident nodes of the path
 * (kh_verify_proofs calls it KH_PROOF_SHORT); kh_trie_need_host returns per key the hash of the
 * stub its walk reaches (need_flag 1, need32[32i..)) or need_flag 0 -- what to fetch before a
 * commit of those keys, the collapse case apart (kh_trie_commit_witness_host lists a batch's whole
 * need, the collapse case included).  kh_trie_export_nodes skips stubs (a branch
 * encodes a stub child by the reference the stub keeps): the export of a partial handle is the
 * witness it holds.  kh_trie_nodes_by_hash never answers from a stub.  To kh_forest_roots,
 * kh_forest_evict, kh_trie_compact, kh_trie_copy, savepoints and rollbacks a stub is a live record
 * of its trie.
 * kh_trie_open_partial with ctx NULL opens on the context the _host entry points share, as
 * kh_forest_open does (the store then lies in HBM of the current device). */
#define KH_FOUND_UNKNOWN 2
int kh_trie_open_partial(kh_ctx* ctx, const uint8_t root32[32], const uint8_t* d_enc, const uint64_t* d_off, uint64_t n,
                         uint32_t flags, uint8_t missing32[32], kh_trie** out);
int kh_trie_open_partial_host(const uint8_t root32[32], const uint8_t* enc, const uint64_t* off, uint64_t n,
                              uint32_t flags, uint8_t missing32[32], kh_trie** out);
int kh_forest_load_partial(kh_trie* f, const uint32_t* tries, const uint8_t* roots32, uint64_t k,
                           const uint8_t* d_enc, const uint64_t* d_off, uint64_t n,
                           uint32_t* miss_idx, uint8_t* miss32, uint64_t miss_cap, uint64_t* n_missing,
                           kh_stats* stats);
int kh_forest_load_partial_host(kh_trie* f, const uint32_t* tries, const uint8_t* roots32, uint64_t k,
                                const uint8_t* enc, const uint64_t* off, uint64_t n,
                                uint32_t* miss_idx, uint8_t* miss32, uint64_t miss_cap, uint64_t* n_missing,
                                kh_stats* stats);
int kh_trie_fill_nodes(kh_trie* h, const uint8_t* d_enc, const uint64_t* d_off, uint64_t n, uint64_t* n_decoded,
                       kh_stats* stats);
int kh_trie_fill_nodes_host(kh_trie* h, const uint8_t* enc, const uint64_t* off, uint64_t n, uint64_t* n_decoded,
                            kh_stats* stats);
int kh_trie_stubs(const kh_trie* h, uint64_t* n);
int kh_trie_missing(const kh_trie* h, uint32_t* tries, uint8_t* hashes32, uint64_t cap, uint64_t* n);
int kh_trie_need_host(kh_trie* h, const uint32_t* trie, const uint8_t* keys, uint32_t klen, uint64_t n,
                      uint8_t* need_flag, uint8_t* need32);

/* The commit witness of a batch: every node a handle opened by kh_trie_open_partial (or
 * kh_forest_load_partial) at the current root(s) must hold to accept the batch at the first attempt
 * -- what a full node hands a stateless verifier or a replica that works from witnesses.  All
 * arrays are host arrays.  Keys, klen, trie ids and the batch contract are those of
 * kh_trie_apply_host / kh_forest_apply_host: upserts first, then deletes; the last op on a key
 * wins, so a key in both lists is a delete; a repeated key counts once; trie ids are read on a
 * forest and ignored on a single trie (they may be NULL there).  No values are taken: the witness
 * does not depend on them.  flags: 0, or KH_HASH_KEYS on a handle opened with it.
 *
 * The witness W is a node table in the layout and order of kh_trie_prove with KH_PROVE_SHARED
 * (hashes32, rlp, off; each (record, node) once, ascending records, the upper node before the
 * branch under its extension; a node two tries of a forest hold appears once per trie).  It holds
 *   (1) the shared proof table of every op key, upserts and deletes alike -- deletes of absent
 *       keys and upserts that end at an empty slot or inside an extension included;
 *   (2) for every branch on those paths that the batch leaves with exactly one non-empty slot,
 *       that slot having held a subtree before the batch: the node hanging in it (the upper node
 *       of its record: a leaf, a branch, or an extension without its branch) when the parent
 *       refers to it by hash -- the child the reference's fix loads (MerklePatriciaTrie.scala:
 *       430-477).  An embedded child is part of the parent's bytes and adds nothing.  A slot is
 *       non-empty after the batch when a key of the post-batch key set lies under it, so a branch
 *       that loses all its keys empties its parent's slot and the parent may be the one that
 *       collapses; a root branch left one child is covered by the same rule.
 * *n_collapse (nullable) = the table nodes in (2) and not in (1).
 * W is sufficient (the partial handle opened from it commits the batch to the root the full handle
 * gives) and minimal (without any one node the open, or the commit, is refused with KH_ENODE).
 *
 * Read-only on the handle: root, records, last roots, write-back set, the kh_trie_missing list and
 * export cursors are as before; with a savepoint open it reads the commits since the savepoint.
 * Work and memory follow the ops and their paths, never the handle's size.
 *
 * KH_OK with *n_nodes = 0: no ops, empty tries only, or ids the forest does not hold.
 * KH_ENOSPC when node_cap or rlp_cap is short: only *n_nodes and *rlp_len are written, and a retry
 * with exactly those sizes succeeds.
 * KH_ENODE on a handle with stubs: the list the commit of the batch on this handle would leave in
 * kh_trie_missing -- if any op's walk reaches a stub, the distinct (trie id, hash to fetch) pairs
 * of those stubs; otherwise the stubs of unknown kind that (2) would move.  *n_missing is their
 * number, at most miss_cap pairs are written (any order), nothing else is.  A surviving stub that
 * stands for the branch under a present extension is not missing (its extension is the collapse
 * child; an extension cut down to nothing leaves no collapse child).
 * KH_EINVAL: a null handle or required output, a klen or KH_HASH_KEYS the handle's commits refuse,
 * trie ids NULL on a forest, nup + ndel >= 2^31, unknown flags.  Whether the commit would be
 * refused for another reason (the key of a value-only branch removed) is not judged: that key's
 * path is listed. */
int kh_trie_commit_witness_host(kh_trie* h, const uint32_t* up_trie, const uint8_t* up_keys, uint64_t nup,
                                const uint32_t* del_trie, const uint8_t* del_keys, uint64_t ndel, uint32_t klen,
                                uint32_t flags, uint8_t* hashes32, uint64_t node_cap, uint8_t* rlp, uint64_t rlp_cap,
                                uint64_t* off, uint64_t* n_nodes, uint64_t* rlp_len, uint64_t* n_collapse,
                                uint32_t* miss_tries, uint8_t* miss_hashes32, uint64_t miss_cap, uint64_t* n_missing);

/* Every trie the forest holds (>= 1 key), ascending ids, with its root: one streaming pass over
 * the records, read-only on the handle.  KH_ENOSPC with *n_tries when cap is short. */
int kh_forest_roots(kh_trie* f, uint32_t* h_tries, uint8_t* h_roots32, uint64_t cap, uint64_t* n_tries);
/* Drop whole tries from HBM: their records die and their anchors leave the map (kh_trie_compact
 * reclaims the space).  An id that is not resident is skipped; *n_evicted = the tries dropped.
 * The caller owns residency: afterwards the id reads as an EMPTY trie (kh_trie_get finds nothing, a
 * commit to it starts from empty), exactly like an id the forest never saw -- reload it with
 * kh_forest_load_nodes before it is used again.  The last commit's roots and write-back set are
 * untouched; export cursors end.  KH_EINVAL while a savepoint is open, as for kh_trie_compact. */
int kh_forest_evict(kh_trie* f, const uint32_t* tries, uint64_t k, uint64_t* n_evicted);

/* Subtrees of a resident trie back to stubs, by nibble path: the inverse of kh_trie_fill_nodes, and
 * the way a working set shrinks inside one large trie.  All arrays are host arrays.  Prefix i is the
 * first depths[i] nibbles of paths32[32i..) (two nibbles a byte, high nibble first; nibbles past the
 * depth are ignored) in trie tries[i] (a forest; ignored and nullable on a single trie).  It names
 * the subtree that HANGS there: the node the slot of a branch, depths[i] nibbles down, refers to -- a
 * leaf, a branch, or an extension with its branch.  The path of a branch under an extension is not
 * where a subtree hangs (the extension's path is): it reports NONE.
 *   KH_EVICT_DONE      the node there was referenced by hash: every record below it dies (stubs
 *                      among them too, their values become dead heap) and its own record becomes
 *                      the plain stub a partial load would have left; hashes32[32i..) is that hash
 *   KH_EVICT_STUB      already a stub, of either form: nothing changes; hashes32 = the hash it asks for
 *   KH_EVICT_EMBEDDED  the node there is embedded in its parent (< 32 B): never a stub; hash zero
 *   KH_EVICT_NONE      an empty slot, inside or off a leaf's or extension's path, below a leaf, below
 *                      a stub, or a trie the handle does not hold; hash zero
 * Afterwards the handle answers every call as kh_trie_open_partial / kh_forest_load_partial would
 * from a store lacking exactly those subtrees' nodes (record order apart): the root, the last
 * commit's roots and the write-back set do not change, reads answer KH_FOUND_UNKNOWN or KH_ENODE
 * with the hash, a commit that reaches the stub is refused with it, kh_trie_fill_nodes brings the
 * subtree back and kh_trie_compact reclaims the space.  kh_trie_size falls by the keys evicted and
 * kh_trie_stubs stays exact.  Nullable outputs: *n_evicted the DONE prefixes, *n_keys the keys
 * evicted, *n_records the records that died (those below the anchors; an anchor's own record is
 * rewritten in place).  Export cursors end.
 * KH_EINVAL, with the handle exactly as before: a null handle or array, tries NULL on a forest, a
 * depth of 0 (a root is never a stub) or above 64, n >= 2^31, two listed prefixes of one trie where
 * one equals or extends the other, a savepoint open.  n == 0 is KH_OK and does nothing.  The cost
 * follows the handle's records, as kh_forest_evict's: one 64-byte line a record. */
#define KH_EVICT_NONE 0
#define KH_EVICT_DONE 1
#define KH_EVICT_STUB 2
#define KH_EVICT_EMBEDDED 3
int kh_trie_evict_subtrees(kh_trie* h, const uint32_t* tries, const uint8_t* paths32, const uint8_t* depths,
                           uint64_t n, uint8_t* status, uint8_t* hashes32,
                           uint64_t* n_evicted, uint64_t* n_keys, uint64_t* n_records);

/* One block (BlockWorldState.flush, BlockWorldState.scala:243-252 then TrieAccounts.flush):
 * the storage ops into the forest, each touched trie's new root written into the stateRoot
 * field of the account upserts that name it (d_a_up_trie[i], KH_NO_TRIE for none; the body
 * RLP[nonce, balance, stateRoot, codeHash] of PV63.scala:46-51 is patched in place in
 * d_a_up_vals), then the account ops into the state trie.  One call per block. */
int kh_block_commit(kh_trie* state, kh_trie* storage, const uint32_t* d_s_up_trie, const uint8_t* d_s_up_keys,
                    const uint8_t* d_s_up_vals, const uint64_t* d_s_up_voff, uint64_t ns_up,
                    const uint32_t* d_s_del_trie, const uint8_t* d_s_del_keys, uint64_t ns_del, uint32_t s_klen,
                    const uint8_t* d_a_up_keys, uint8_t* d_a_up_vals, const uint64_t* d_a_up_voff,
                    const uint32_t* d_a_up_trie, uint64_t na_up, const uint8_t* d_a_del_keys, uint64_t na_del,
                    uint32_t a_klen, uint8_t state_root32[32], kh_stats* stats);
/* kh_block_commit from host arrays (staged in one device buffer; for a JVM caller). */
int kh_block_commit_host(kh_trie* state, kh_trie* storage, const uint32_t* s_up_trie, const uint8_t* s_up_keys,
                         const uint8_t* s_up_vals, const uint64_t* s_up_voff, uint64_t ns_up,
                         const uint32_t* s_del_trie, const uint8_t* s_del_keys, uint64_t ns_del, uint32_t s_klen,
                         const uint8_t* a_up_keys, const uint8_t* a_up_vals, const uint64_t* a_up_voff,
                         const uint32_t* a_up_trie, uint64_t na_up, const uint8_t* a_del_keys, uint64_t na_del,
                         uint32_t a_klen, uint8_t state_root32[32], kh_stats* stats);

/* ---- versioned commits ----
 * Ledger.executeBlock flushes the parallel attempt's world state and, when its root does not
 * validate, re-executes the block sequentially from the SAME parent state
 * (khipu-eth/.../ledger/Ledger.scala:237-271); validateBlockAfterExecution rejects a block whose
 * root or gas does not match (:603-620); TrieAccounts.rootHash flushes a COPY of the trie and
 * leaves the trie itself untouched (khipu-eth/.../ledger/TrieAccounts.scala:73-80, called per
 * transaction at Ledger.scala:576; MerklePatriciaTrie.copy, MerklePatriciaTrie.scala:556).
 *
 * kh_trie_savepoint opens a savepoint on a trie or forest (they nest; *depth = the number now
 * open).  Commits after it are journaled: each saves the records it rewrites and logs the
 * anchor-map slots it changes, O(changed nodes).  kh_trie_rollback returns the handle to the
 * innermost savepoint's version -- root, records, value heap, the last commit's trie list and
 * roots (kh_forest_last_roots) and write-back set (kh_trie_emit_nodes) -- and closes it;
 * kh_trie_release keeps the commits and closes it.  kh_block_commit is all or nothing on both
 * handles: a refusal or failure in either phase leaves both at the parent version. */
int kh_trie_savepoint(kh_trie* h, uint32_t* depth);
int kh_trie_rollback(kh_trie* h);
int kh_trie_release(kh_trie* h);
int kh_trie_savepoint_depth(const kh_trie* h, uint32_t* depth);

/* TrieAccounts.rootHash (TrieAccounts.scala:73-80): the root that kh_trie_apply of this batch
 * would give, the handle left unchanged (a commit between a savepoint and its rollback). */
int kh_trie_root_of(kh_trie* h, const uint8_t* d_up_keys, const uint8_t* d_up_vals, const uint64_t* d_up_voff,
                    uint64_t nup, const uint8_t* d_del_keys, uint64_t ndel, uint32_t klen, uint32_t flags,
                    uint8_t root32[32], kh_stats* stats);
int kh_trie_root_of_host(kh_trie* h, const uint8_t* up_keys, const uint8_t* up_vals, const uint64_t* up_voff,
                         uint64_t nup, const uint8_t* del_keys, uint64_t ndel, uint32_t klen, uint32_t flags,
                         uint8_t root32[32], kh_stats* stats);

/* MerklePatriciaTrie.copy (MerklePatriciaTrie.scala:556): an independent handle holding the
 * current version of h in HBM (no savepoints); free it with kh_trie_free. */
int kh_trie_copy(kh_trie* h, kh_trie** out);

/* Storage write-back hand-off of the LAST commit (open or apply) of a
 * trie opened with KH_EMIT_NODES: exactly the nodes that commit created -- every node
 * reachable from a new root whose encoding is >= 32 B and that the previous version did
 * not hold, plus a changed root node -- what persist()/changes hand to NodeStorage.update
 * (MerklePatriciaTrie.scala:491-516,544-554; BlockWorldState.scala:312-330).  Same layout
 * and KH_ENOSPC size negotiation as kh_trie_root_nodes (no re-encoding on the retry). */
int kh_trie_emit_nodes(kh_trie* h, uint8_t* hashes32, uint64_t node_cap, uint8_t* rlp, uint64_t rlp_cap,
                       uint64_t* off, uint64_t* n_nodes, uint64_t* rlp_len);

/* Batched get on a resident trie or forest: MerklePatriciaTrie.get (MerklePatriciaTrie.scala:
 * 90-147; callers Blockchain.scala:336-342) answered from the records in HBM by the commit's
 * anchor descent, so a JVM holding state in HBM can read it without its own node store.
 * n queries: key i (klen bytes; kec256'd on the device when the trie was opened with
 * KH_HASH_KEYS, as its commits are) in trie trie[i] (forests; NULL for a single trie).
 * found[i] = 1 iff the key is present (None otherwise); the values are packed into vals with
 * voff[n+1] (an absent key has an empty span).  When the values need more than val_cap
 * bytes the call returns KH_ENOSPC and writes only *val_bytes (the size needed).
 * Device-buffer form on the handle's context stream; _host form with host buffers. */
int kh_trie_get(kh_trie* h, const uint32_t* d_trie, const uint8_t* d_keys, uint32_t klen, uint64_t n,
                uint8_t* d_vals, uint64_t val_cap, uint64_t* d_voff, uint8_t* d_found, uint64_t* val_bytes);
int kh_trie_get_host(kh_trie* h, const uint32_t* trie, const uint8_t* keys, uint32_t klen, uint64_t n,
                     uint8_t* vals, uint64_t val_cap, uint64_t* voff, uint8_t* found, uint64_t* val_bytes);

/* ---- node export and nodes by hash: a resident handle's nodes read back out ----
 * The checkpoint half of kh_trie_open_nodes (a state root plus its node store is the whole
 * resumable state), for any handle: no KH_EMIT_NODES needed, no delta kept by the caller.  Both
 * calls re-encode nodes from the records in HBM (khipu_amd/csrc/export.h), read-only on the
 * handle: with a savepoint open they see the commits since it. */
#define KH_EXPORT_VERIFY 0x1u
typedef struct kh_export_cursor { uint64_t next, epoch; } kh_export_cursor;  /* zero it to start */

/* Every node of the CURRENT version of a resident trie or forest that a node store needs
 * (encoding >= 32 B, plus each trie's root node), re-encoded from the records, in chunks.
 * trie_filter: a trie id of a forest, or KH_NO_TRIE for every trie.  Each call writes the nodes
 * of as many consecutive records from cur->next as fit node_cap and rlp_cap (layout of
 * kh_trie_root_nodes; off needs node_cap + 1 entries), advances *cur and sets *done when the
 * records are exhausted.  If not even the next record fits: KH_ENOSPC with *n_nodes / *rlp_len =
 * what it needs, cursor unchanged.  Nodes come in record order, each once; a node shared by two
 * tries of a forest comes once per trie.
 * A cursor from before a commit, rollback or compaction of the handle: KH_EINVAL.
 * KH_EXPORT_VERIFY: KH_EINTERNAL if any re-hashed encoding differs from its cached reference. */
int kh_trie_export_nodes(kh_trie* h, uint32_t trie_filter, uint32_t flags, kh_export_cursor* cur,
                         uint8_t* hashes32, uint64_t node_cap, uint8_t* rlp, uint64_t rlp_cap,
                         uint64_t* off, uint64_t* n_nodes, uint64_t* rlp_len, int* done);

/* getMptNodeByHash over the current version (HostService.scala:103-112, Blockchain.scala:356):
 * found[i] = 1 and the encoding at rlp[off[i]..off[i+1]) when a node with kec256 == hashes32[32i..)
 * is reachable from a current root; else 0 and an empty span.  n <= 4096 (KH_EINVAL above).
 * One streaming pass over the records per 2048 hashes: no hash index is kept on the handle.
 * KH_ENOSPC writes only *rlp_len. */
int kh_trie_nodes_by_hash(kh_trie* h, const uint8_t* hashes32, uint64_t n, uint8_t* found,
                          uint8_t* rlp, uint64_t rlp_cap, uint64_t* off, uint64_t* rlp_len);

/* ---- Merkle proofs: the nodes on a key's path, and their check against a root ----
 * The proof of a key is the list of nodes MerklePatriciaTrie.get visits from the trie's root,
 * root first, restricted to the nodes a node store holds (encoding >= 32 B, plus the root node;
 * a node embedded in its parent is part of the parent's bytes).  The walk ends at the leaf it
 * reaches (whether or not its key matches), at an extension whose path the key leaves (listed),
 * at a branch whose slot for the key's next nibble is empty, or at a value-only branch.  An empty
 * trie, or a trie id a forest does not hold, gives an empty proof and found = 0.
 *
 * kh_trie_prove: n < 2^31 keys and trie ids exactly as in kh_trie_get_host; read-only on the
 * handle (with a savepoint open it sees the commits since).  found[i] as in kh_trie_get.  The node
 * table has the layout of kh_trie_root_nodes (node j: hash hashes32[32j..), encoding
 * rlp[off[j]..off[j+1]), off of node_cap + 1 entries); the proof of key i is the table nodes
 * path_idx[k], k in [path_off[i], path_off[i+1]) (path_off of n + 1 entries).  Without
 * KH_PROVE_SHARED the table is the concatenation of the proofs (path_idx[k] == k).  With it every
 * (record, node) appears once however many keys pass through it (a block witness), in ascending
 * record order, the node a parent refers to before the branch under its extension; a node two
 * tries of a forest hold comes once per trie.  At most 2^32 - 1 listed nodes a call (KH_EINVAL).
 * When any capacity is short: KH_ENOSPC, and only *n_nodes, *rlp_len and *n_path are written (a
 * retry with exactly those sizes succeeds). */
#define KH_PROVE_SHARED 0x1u
/* KH_PROVE_TRIE_KEYS: the keys are trie keys already (klen == 32; on a KH_HASH_KEYS handle the
 * kec256 values a range scan returns) and are not hashed.  kh_verify_proofs with flags = 0 checks
 * such proofs. */
#define KH_PROVE_TRIE_KEYS 0x2u
int kh_trie_prove(kh_trie* h, const uint32_t* trie, const uint8_t* keys, uint32_t klen, uint64_t n,
                  uint32_t flags, uint8_t* found,
                  uint8_t* hashes32, uint64_t node_cap, uint8_t* rlp, uint64_t rlp_cap, uint64_t* off,
                  uint32_t* path_idx, uint64_t path_cap, uint64_t* path_off,
                  uint64_t* n_nodes, uint64_t* rlp_len, uint64_t* n_path);

/* kh_verify_proofs: needs no handle (a checker has no trie).  Key i (klen bytes; kec256'd with
 * KH_HASH_KEYS in flags, else klen must be 32) is walked from roots32 (nroots = 1: one root for
 * every key, or n: one per key) over its listed nodes, table and path arrays as kh_trie_prove
 * returns them (plain or shared).  The first condition met, in walk order, decides status[i]:
 * the next listed node must hash to the expected reference (the root at first); a 17-item list
 * takes the key's next nibble (item 16 once the 64 nibbles are used up); a 2-item list is
 * HexPrefix-decoded (flag nibble <= 3, a zero pad nibble, no path past nibble 64); an empty child
 * item ends the walk (absent), a 32-byte string is the next expected reference, a list shorter
 * than 32 B is walked in place, anything else is a bad node.  An empty proof is ABSENT iff the
 * root is EMPTY_TRIE_HASH, else SHORT.  Values of the PROOF_VALUE keys are packed as in
 * kh_trie_get_host (KH_ENOSPC writes only *val_bytes).  off or path_off not non-decreasing, or a
 * node longer than 2^32 - 1 bytes: KH_EINVAL. */
#define KH_PROOF_ABSENT 0   /* valid: the key is not in the trie */
#define KH_PROOF_VALUE 1    /* valid: the value is returned */
#define KH_PROOF_BAD_HASH 2 /* a listed node's kec256 is not the reference that leads to it (the root for the first) */
#define KH_PROOF_BAD_NODE 3 /* a node on the walk is not a well-formed trie node, or a path index >= n_nodes */
#define KH_PROOF_SHORT 4    /* the walk reaches a hash reference and the list has no further node */
#define KH_PROOF_EXTRA 5    /* the walk ends before the list does */
int kh_verify_proofs(const uint8_t* roots32, uint64_t nroots, const uint8_t* keys, uint32_t klen, uint64_t n,
                     uint32_t flags, const uint8_t* rlp, const uint64_t* off, uint64_t n_nodes,
                     const uint32_t* path_idx, const uint64_t* path_off,
                     uint8_t* status, uint8_t* vals, uint64_t val_cap, uint64_t* voff, uint64_t* val_bytes);

/* ---- range scan: a resident trie read in key order ----
 * The first entries of [origin32, limit32] (both inclusive; NULL = 32 zero bytes / 32 bytes of 0xFF;
 * origin > limit: an empty answer) of trie `trie` (forests; ignored on a single trie; an id the
 * forest does not hold: an empty answer) in ascending key order: at most max_entries, with values
 * fitting val_cap.  Keys are TRIE keys: on a KH_HASH_KEYS handle the kec256 values (preimages
 * are not kept).  keys32 holds 32 * max_entries bytes, voff max_entries + 1 slots; entry i is
 * keys32[32i..) with the value vals[voff[i]..voff[i+1]).  *more = 1 and next32 = the first key not
 * returned when one exists in range (continue with origin = next32), else *more = 0.  No cursor
 * and no epoch: a call reads the current version (with a savepoint open, the commits since), and
 * is read-only on the handle.  Work and memory follow max_entries, not the trie's size
 * (khipu_amd/csrc/range.h).
 *   KH_ENOSPC  even the first entry's value does not fit: *val_bytes is its size, nothing else
 *              is written
 *   KH_EINVAL  max_entries == 0 or >= 2^31, or a null output
 *   KH_ENODE   (partial handles only) a missing subtree is among the first max_entries + 1 things
 *              in range, a missing subtree that meets the range counting as one thing at its
 *              lowest key: missing32 (nullable) is the hash of its node, nothing else is written
 * _host form with host buffers; kh_dev_trie_range with keys32 / vals / voff device buffers, on the
 * handle's context stream (the scalar outputs are host words, valid on return). */
int kh_trie_range_host(kh_trie* h, uint32_t trie, const uint8_t origin32[32], const uint8_t limit32[32],
                       uint64_t max_entries, uint8_t* keys32, uint8_t* vals, uint64_t val_cap, uint64_t* voff,
                       uint64_t* n_entries, uint64_t* val_bytes, int* more, uint8_t next32[32],
                       uint8_t missing32[32]);
int kh_dev_trie_range(kh_trie* h, uint32_t trie, const uint8_t origin32[32], const uint8_t limit32[32],
                      uint64_t max_entries, uint8_t* d_keys32, uint8_t* d_vals, uint64_t val_cap, uint64_t* d_voff,
                      uint64_t* n_entries, uint64_t* val_bytes, int* more, uint8_t next32[32],
                      uint8_t missing32[32]);

/* ---- batched range scan: many key ranges of a forest (or of one trie) in one call ----
 * nq requests answered in request order under ONE entry and byte budget (the serving half of a
 * GetStorageRanges response, which kh_verify_ranges checks in one call).  Request q is trie
 * tries[q] (forests; on a single trie `tries` is ignored and may be NULL; an id the forest does not
 * hold: an empty request; the same trie may be named by several requests) and the range
 * [origins32[32q..), limits32[32q..)], both inclusive (origins32 NULL: every origin 32 zero bytes;
 * limits32 NULL: every limit 32 bytes of 0xFF; origin > limit: an empty request).  Keys are TRIE
 * keys, as in kh_trie_range_host.
 *   The answer is the concatenation, in request order, of each request's entries in ascending key
 * order, cut to its longest prefix of at most max_entries entries IN TOTAL whose values fit
 * val_cap IN TOTAL.  keys32 holds 32 * max_entries bytes, voff max_entries + 1 slots, ent_off
 * nq + 1 slots: entry i is keys32[32i..) with the value vals[voff[i]..voff[i+1]); request q's
 * entries are ent_off[q] .. ent_off[q+1], and ent_off[nq] = *n_entries.
 *   *n_done is the number of leading requests answered completely; *n_done == nq: everything asked
 * for was returned.  Otherwise request *n_done is the cut one: its entries so far are returned
 * (none when the cut falls exactly on its first entry), next32 is its first key not returned
 * (continue with that as its origin), and the requests after it are unanswered -- their spans are
 * empty and they are to be asked again.  Empty requests before the cut one count as done.
 *   No cursor and no epoch; read-only on the handle; with a savepoint open a call reads the commits
 * since, as the single call does.  All requests move through the rounds of the walk together: a
 * call costs the rounds of its deepest request, and its work and memory follow max_entries + nq,
 * not the tries' sizes (khipu_amd/csrc/range.h).
 *   KH_ENOSPC  not even the first entry of the whole answer fits: *val_bytes is its size, nothing
 *              else is written
 *   KH_EINVAL  nq == 0, max_entries == 0, nq + max_entries >= 2^31, a null output, or `tries` NULL
 *              on a forest
 *   KH_ENODE   (partial handles only) a missing subtree is among the first max_entries + 1 things of
 *              the concatenated answer, a missing subtree that meets its request's range counting
 *              as one thing at its lowest key: missing32 (nullable) is the hash of its node and
 *              *n_done the index of the request it belongs to (which trie's store to fetch for);
 *              nothing else is written
 * _host form with host buffers; kh_dev_trie_ranges with tries / origins32 / limits32 / keys32 /
 * vals / voff / ent_off device buffers (voff and ent_off 8-byte aligned), on the handle's context
 * stream (the scalar outputs are host words, valid on return). */
int kh_trie_ranges_host(kh_trie* h, const uint32_t* tries, const uint8_t* origins32, const uint8_t* limits32,
                        uint64_t nq, uint64_t max_entries, uint8_t* keys32, uint8_t* vals, uint64_t val_cap,
                        uint64_t* voff, uint64_t* ent_off, uint64_t* n_entries, uint64_t* val_bytes,
                        uint64_t* n_done, uint8_t next32[32], uint8_t missing32[32]);
int kh_dev_trie_ranges(kh_trie* h, const uint32_t* d_tries, const uint8_t* d_origins32, const uint8_t* d_limits32,
                       uint64_t nq, uint64_t max_entries, uint8_t* d_keys32, uint8_t* d_vals, uint64_t val_cap,
                       uint64_t* d_voff, uint64_t* d_ent_off, uint64_t* n_entries, uint64_t* val_bytes,
                       uint64_t* n_done, uint8_t next32[32], uint8_t missing32[32]);

/* ---- trie diff: the keys whose entries differ between two resident tries, in key order ----
 * Side a is trie `trie_a` of handle a, side b trie `trie_b` of handle b: resident tries or forests
 * on the same device (the ids are read on a forest and ignored on a single trie; a == b with two
 * ids is allowed, the same (handle, id) on both sides is an empty answer; an id a forest does not
 * hold, or an empty trie, is an empty side: every key of the other side is then a difference).
 * Keys are TRIE keys (on KH_HASH_KEYS handles the kec256 values).  A difference is a key of
 * [origin32, limit32] (both inclusive and nullable, as in kh_trie_range_host) whose entry differs
 * between the sides: present on one side only, present on both with different value bytes, or
 * present on both where exactly one entry is khipu's value-only branch -- the nodes differ then,
 * and so do the roots; applying the upsert to a leaf is how khipu makes that branch.
 *   The answer is the first differences in ascending key order: at most max_entries, cut to the
 * longest prefix whose side-b values fit val_cap.  keys32 holds 32 * max_entries bytes, kinds
 * max_entries bytes, voff max_entries + 1 slots: difference i is the key keys32[32i..) of kind
 * kinds[i] with vals[voff[i]..voff[i+1]) = b's value for kinds 2 and 3, an empty span for kind 1 --
 * so the KH_DIFF_ONLY_A keys are the deletes and the others the upserts of the kh_trie_apply that
 * brings a to b.  *more = 1 and next32 = the first differing key not returned when one exists
 * (continue with origin = next32), else *more = 0.  Read-only on both handles; with a savepoint
 * open a call reads the commits since, as the range scan does.
 *   Two subtrees are skipped, unread, exactly when both sides have a node that starts at the same
 * nibble path with the same reference (a 32-byte hash, or the bytes of an embedded node): work and
 * memory follow max_entries and the changed paths, not the tries (khipu_amd/csrc/diff.h).
 *   Partial handles: a stub is a node that starts at the depth it records with the hash of the
 * missing node (its extension, when present, starts at the stub's anchor with the reference the
 * parent holds).  A stub skipped by the rule above costs nothing, so two partial handles that differ
 * only where both hold nodes diff completely; a stub that is not skipped is a missing thing at its
 * lowest key.
 *   KH_ENOSPC  not even the first difference's value fits: *val_bytes is its size, nothing else is
 *              written
 *   KH_EINVAL  max_entries == 0 or >= 2^31, a null handle or output, handles on different devices
 *   KH_ENODE   a missing thing is among the first max_entries + 1 things in range: missing32
 *              (nullable) is the hash of the missing node, the lowest in key order (side a's when
 *              both sides miss one at the same place); nothing else is written
 * _host form with host buffers; kh_dev_trie_diff with keys32 / kinds / vals / voff device buffers
 * (voff 8-byte aligned), on a's context stream (the scalar outputs are host words, valid on return). */
#define KH_DIFF_ONLY_A 1   /* the key is in a only: a delete on the way from a to b */
#define KH_DIFF_ONLY_B 2   /* the key is in b only: an upsert of b's value */
#define KH_DIFF_CHANGED 3  /* in both; values differ, or exactly one side is a value-only branch */
int kh_trie_diff_host(kh_trie* a, uint32_t trie_a, kh_trie* b, uint32_t trie_b,
                      const uint8_t origin32[32], const uint8_t limit32[32],
                      uint64_t max_entries, uint64_t val_cap,
                      uint8_t* keys32, uint8_t* kinds, uint8_t* vals, uint64_t* voff,
                      uint64_t* n_entries, uint64_t* val_bytes, int* more,
                      uint8_t next32[32], uint8_t missing32[32]);
int kh_dev_trie_diff(kh_trie* a, uint32_t trie_a, kh_trie* b, uint32_t trie_b,
                     const uint8_t origin32[32], const uint8_t limit32[32],
                     uint64_t max_entries, uint64_t val_cap,
                     uint8_t* d_keys32, uint8_t* d_kinds, uint8_t* d_vals, uint64_t* d_voff,
                     uint64_t* n_entries, uint64_t* val_bytes, int* more,
                     uint8_t next32[32], uint8_t missing32[32]);

/* ---- batched trie diff: many trie pairs of two forests (or many ranges of one pair) in one call ----
 * nq requests answered in request order under ONE entry and byte budget (a replica's (upserts,
 * deletes) of every storage trie a block touched, a parent version kept as a kh_trie_copy of the
 * forest).  Request q is kh_trie_diff_host's contract applied to trie tries_a[q] of handle a against
 * trie tries_b[q] of handle b over [origins32[32q..), limits32[32q..)], both inclusive.  tries_b
 * NULL: tries_b = tries_a (two versions of one forest).  On a single-trie handle that side's ids are
 * ignored and may be NULL.  origins32 NULL: every origin 32 zero bytes; limits32 NULL: every limit 32
 * bytes of 0xFF.  Empty requests: the same (handle, id) on both sides, an id neither side holds, two
 * empty tries, origin > limit, and a pair with equal roots (its two root probes and no round).  An id
 * held by one side only makes every key of the other side a difference.  The same pair may be named
 * by several requests.  Keys, kinds, side-b values and the value-only-branch rule are
 * kh_trie_diff_host's.
 *   The answer is the concatenation, in request order, of each request's differences in ascending
 * key order, cut to its longest prefix of at most max_entries differences IN TOTAL whose side-b
 * values fit val_cap IN TOTAL.  keys32 holds 32 * max_entries bytes, kinds max_entries bytes, voff
 * max_entries + 1 slots, ent_off nq + 1 slots: difference i is the key keys32[32i..) of kind kinds[i]
 * with the value vals[voff[i]..voff[i+1]); request q's differences are ent_off[q] .. ent_off[q+1],
 * and ent_off[nq] = *n_entries.
 *   *n_done is the number of leading requests answered completely; *n_done == nq: every difference
 * asked for was returned.  Otherwise request *n_done is the cut one: its differences so far are
 * returned (none when the cut falls exactly on its first difference), next32 is its first differing
 * key not returned (continue with that as its origin), and the requests after it are unanswered --
 * their spans are empty and they are to be asked again.  Empty requests before the cut one count as
 * done.
 *   Read-only on both handles; with a savepoint open a call reads the commits since.  All requests
 * move through the rounds of the walk together: a call costs the rounds of its deepest request, and
 * its work and memory follow max_entries + nq and the changed paths, not the tries
 * (khipu_amd/csrc/diff.h).
 *   KH_ENOSPC  not even the first difference of the whole answer fits: *val_bytes is its size,
 *              nothing else is written
 *   KH_EINVAL  nq == 0, max_entries == 0, nq + max_entries >= 2^31, a null handle or output, tries_a
 *              NULL on a forest side (a forest a, or a forest b without tries_b), handles on
 *              different devices
 *   KH_ENODE   a missing thing is among the first max_entries + 1 things of the concatenated answer:
 *              missing32 (nullable) is the hash of its node (side a's when both sides miss one at
 *              the same place) and *n_done the index of the request it belongs to; nothing else is
 *              written.  A stub that is skipped costs nothing, as in the single call.
 * _host form with host buffers; kh_dev_trie_diffs with tries_a / tries_b / origins32 / limits32 /
 * keys32 / kinds / vals / voff / ent_off device buffers (voff and ent_off 8-byte aligned), on a's
 * context stream (the scalar outputs are host words, valid on return). */
int kh_trie_diffs_host(kh_trie* a, const uint32_t* tries_a, kh_trie* b, const uint32_t* tries_b,
                       const uint8_t* origins32, const uint8_t* limits32, uint64_t nq,
                       uint64_t max_entries, uint64_t val_cap,
                       uint8_t* keys32, uint8_t* kinds, uint8_t* vals, uint64_t* voff, uint64_t* ent_off,
                       uint64_t* n_entries, uint64_t* val_bytes, uint64_t* n_done,
                       uint8_t next32[32], uint8_t missing32[32]);
int kh_dev_trie_diffs(kh_trie* a, const uint32_t* d_tries_a, kh_trie* b, const uint32_t* d_tries_b,
                      const uint8_t* d_origins32, const uint8_t* d_limits32, uint64_t nq,
                      uint64_t max_entries, uint64_t val_cap,
                      uint8_t* d_keys32, uint8_t* d_kinds, uint8_t* d_vals, uint64_t* d_voff, uint64_t* d_ent_off,
                      uint64_t* n_entries, uint64_t* val_bytes, uint64_t* n_done,
                      uint8_t next32[32], uint8_t missing32[32]);

/* ---- changes since a savepoint: a block's key delta read from the undo journal, without a copy ----
 * The keys whose entries differ between the version at an OPEN SAVEPOINT of handle h and its current
 * version, with kinds and values, in (trie id, key) order: what kh_trie_diff_host /
 * kh_trie_diffs_host give against a kh_trie_copy taken at the savepoint, read instead from the
 * records the commits since journaled and appended.  Work and scratch follow those records (the
 * keys a block changed and their paths), never the trie, and no second handle is held.
 *   Versions.  level selects the savepoint: 0 the innermost, 1 .. depth that savepoint counted from
 * the outermost (1: everything the journal holds).  S is the handle's content at that savepoint, C
 * its content now -- after the commits, kh_block_commit calls and forest loads made since.  Content
 * is a map (trie id, TRIE key) -> (value bytes, is-value-only-branch); a single trie is trie id 0.
 *   Differences.  kh_trie_diff_host's, with a = S and b = C: a key in S only (KH_DIFF_ONLY_A), in C
 * only (KH_DIFF_ONLY_B), or in both with different value bytes or where exactly one entry is a
 * value-only branch (KH_DIFF_CHANGED).  Values are C's for kinds 2 and 3; kind 1 has an empty span.
 * NOT differences: a key upserted with the bytes it had; a key deleted and put back with the same
 * bytes, in one commit or across several; a key created and deleted again since the savepoint; a
 * leaf that was only re-anchored because a sibling went and its branch collapsed.
 *   KH_CHANGES_REVERSE swaps the roles, a = C and b = S: the kinds swap and the values are the
 * savepoint's (still in the heap: it is append-only between compactions, and kh_trie_compact is
 * refused while a savepoint is open).  These are the ops that undo the commits: a replica's reorg.
 *   Answer.  The differences in ascending (trie id, key) order from (from_trie, from32) inclusive
 * (from32 NULL: from the beginning; from_trie is ignored then, and on a single trie): at most
 * max_entries, cut to the longest prefix whose values fit val_cap.  tries (nullable on a single
 * trie: max_entries ids), keys32, kinds, vals and voff (max_entries + 1 slots) have the diff's
 * layout.  *n_total (nullable) is the number of differences at or after the resume point, returned
 * or not.  *more = 1 and (next_trie, next32) = the first difference not returned when one exists,
 * else *more = 0.  There is no cursor: every call reads the journal again, so one call with
 * max_entries >= *n_total is the cheap way to take a whole answer.
 *   Read-only on the handle: root, records, last roots, write-back set, kh_trie_missing list, export
 * cursors and the journal are as before.
 *   Partial handles: the answer is exact and the call never returns KH_ENODE -- a commit creates and
 * removes no stub, and stubs are not entries; nothing is walked, so nothing missing is met.  (A diff
 * of two copies gives up where an unskipped stub lies on a changed path.)
 *   KH_EINVAL  no savepoint open, level > depth, unknown flags, max_entries == 0 or >= 2^31, a null
 *              handle or required output (tries on a forest)
 *   KH_ENOSPC  not even the first difference's value fits: *val_bytes is its size and *n_total is
 *              written; nothing else is written
 * A handle whose in-flight commit tail failed refuses the call like every other.
 * _host form with host buffers; kh_dev_trie_changes_since with tries / keys32 / kinds / vals / voff
 * device buffers (voff 8-byte aligned), on the handle's context stream (the scalar outputs are host
 * words, valid on return).  (khipu_amd/csrc/changes.h) */
#define KH_CHANGES_REVERSE 0x1u
int kh_trie_changes_since_host(kh_trie* h, uint32_t level, uint32_t flags,
                               uint32_t from_trie, const uint8_t from32[32],
                               uint64_t max_entries, uint64_t val_cap,
                               uint32_t* tries, uint8_t* keys32, uint8_t* kinds, uint8_t* vals, uint64_t* voff,
                               uint64_t* n_entries, uint64_t* val_bytes, uint64_t* n_total, int* more,
                               uint32_t* next_trie, uint8_t next32[32]);
int kh_dev_trie_changes_since(kh_trie* h, uint32_t level, uint32_t flags,
                              uint32_t from_trie, const uint8_t from32[32],
                              uint64_t max_entries, uint64_t val_cap,
                              uint32_t* d_tries, uint8_t* d_keys32, uint8_t* d_kinds, uint8_t* d_vals, uint64_t* d_voff,
                              uint64_t* n_entries, uint64_t* val_bytes, uint64_t* n_total, int* more,
                              uint32_t* next_trie, uint8_t next32[32]);

/* ---- range verification: range responses checked against a root, without a handle ----
 * The receiving half of kh_trie_range_host + kh_trie_prove(KH_PROVE_TRIE_KEYS) (snap's ranges,
 * geth's VerifyRangeProof), nr ranges a call over ONE node set.  Range s: root roots32[32s..),
 * origin origins32[32s..) (origins32 NULL: all zero), entries ent_off[s] .. ent_off[s+1] of keys32 /
 * vals / voff (entry i: key keys32[32i..), value vals[voff[i]..voff[i+1])).  Keys are 32-byte TRIE
 * keys and are never hashed here (on a KH_HASH_KEYS handle: the kec256 values a range scan
 * returns).  The node set has the layout of kh_trie_open_nodes: n_nodes encodings enc[off[j]..
 * off[j+1]), content addressed (hashed here); duplicates and strangers are fine.  proved[s] = 0:
 * the entries claim to be the whole trie, no node is read; 1: the boundary proof of origin and of
 * the last key (of origin alone without entries) is taken from the node set.  There is no limit:
 * a responder may stop anywhere, the caller compares the last key with its limit.
 * Per range, with o = origin, k_1..k_m the entries and hi = k_m (o when m = 0):
 *   1. keys strictly ascending, k_1 >= o, every value >= 1 byte -- else BAD_ORDER, decided before
 *      any node is read.
 *   2. proved = 0: OK iff the root of the trie of the entries is the root (EMPTY_TRIE_HASH for
 *      m = 0), else BAD_ROOT; more = 0.
 *   3. proved = 1: the walk goes down from the root along o's path and hi's path only.  A child of
 *      a branch whose prefix is below o's is kept as an opaque subtree (its reference: a 32-byte
 *      hash or an embedded list < 32 B), above hi's prefix likewise and more = 1, on a path it is
 *      entered (a hash absent from the node set: MISSING), strictly between it is dropped.  A
 *      leaf or extension is HexPrefix-decoded to its full prefix q: an extension that is a prefix
 *      of o or of hi is entered; else q below o: kept as the node itself, above hi: kept and
 *      more = 1, within: dropped (so a leaf in [o, hi] must be among the entries).  A value-only
 *      branch at nibble 64 counts as a leaf.  Nodes must be well formed by kh_verify_proofs'
 *      rules (and a leaf's path must end at nibble 64), else BAD_NODE.  Each path stops at its
 *      first problem; BAD_NODE on either path wins over MISSING; missing32 is the hash on o's
 *      path if that path has one, else hi's.  Nodes never met are ignored.
 *   4. m = 0 and more = 1: INCOMPLETE.
 *   5. the canonical trie over the entries (leaves) and the kept subtrees at their prefixes is
 *      hashed: OK iff its root is the given one, else BAD_ROOT -- also when a kept subtree would
 *      have to move (its parent branch would have it as the only child, an entry would run under
 *      its prefix), which only a response that omits or invents entries produces.
 * Limit: a range whose inside holds one of khipu's value-only branches (a re-put key under a
 * depth-63 branch) cannot be expressed by entries and reports BAD_ROOT.
 * An honest response cut at its end stays valid while the new last key's path is in the node
 * set: the cut entries become subtrees kept on the right and more = 1.
 * Outputs: status[s]; more[s] = 1 iff the trie holds a key above hi (meaningful for OK and
 * INCOMPLETE); missing32 (nullable) [32s..) for MISSING, zero otherwise.
 * KH_EINVAL, nothing written: a null array (vals may be NULL only when no entry has a byte);
 * ent_off, voff or off not non-decreasing (checked by kh_verify_ranges; a precondition of the
 * device form); nr, the entry total or n_nodes >= 2^31.
 * kh_dev_verify_ranges: every input array in HBM (ctx NULL: the context the host forms use), on
 * the context's stream.  d_roots32, d_origins32 and d_keys32 are read as 64-bit words: they and the
 * offset arrays must be 8-byte aligned, and d_ent_off[0] = 0 (KH_EINVAL otherwise); every value is
 * shorter than 2^32 bytes (a precondition).  status, more and missing32 are host arrays, valid on
 * return. */
#define KH_RANGE_OK 0          /* the entries are exactly the trie's content in [origin, last key] */
#define KH_RANGE_BAD_ORDER 1   /* keys not strictly ascending, first key < origin, or an empty value */
#define KH_RANGE_MISSING 2     /* a hash on a boundary path is not in the node set (missing32) */
#define KH_RANGE_BAD_NODE 3    /* a node met on a boundary path is not a well-formed trie node */
#define KH_RANGE_BAD_ROOT 4    /* the rebuilt root differs from the given one */
#define KH_RANGE_INCOMPLETE 5  /* no entries, yet the proof shows a key at or after origin */
int kh_verify_ranges(const uint8_t* roots32, const uint8_t* origins32, const uint8_t* proved, uint64_t nr,
                     const uint8_t* keys32, const uint8_t* vals, const uint64_t* voff, const uint64_t* ent_off,
                     const uint8_t* enc, const uint64_t* off, uint64_t n_nodes,
                     uint8_t* status, uint8_t* more, uint8_t* missing32);
int kh_dev_verify_ranges(kh_ctx* ctx, const uint8_t* d_roots32, const uint8_t* d_origins32, const uint8_t* d_proved,
                         uint64_t nr, const uint8_t* d_keys32, const uint8_t* d_vals, const uint64_t* d_voff,
                         const uint64_t* d_ent_off, const uint8_t* d_enc, const uint64_t* d_off, uint64_t n_nodes,
                         uint8_t* status, uint8_t* more, uint8_t* missing32);

/* Range responses INTO a partial handle: the receiving half of a range sync.  Where
 * kh_verify_ranges judges a response on its own and keeps nothing, this call replaces the stubs of
 * a partial handle (kh_trie_open_partial, kh_forest_load_partial) that lie inside the delivered
 * span with the subtrees built from the entries, and keeps the result only if no root moves: a
 * stub remembers the hash its parent holds, so the trie itself checks the rebuild.  A root-only
 * handle becomes the full resident trie page by page, usable for gets, proofs, ranges, diffs and
 * commits on the synced part the whole time; a forest takes a GetStorageRanges answer (many whole
 * small tries and one tail) in one call.
 * Inputs: the entry layout of kh_verify_ranges (range s is entries ent_off[s] .. ent_off[s+1]).
 * Keys are 32-byte TRIE keys and are never hashed: on a KH_HASH_KEYS handle they are the kec256
 * values a range scan returns.  tries[s] names range s's trie (ignored and nullable on a single
 * trie, which takes one range a call); origins32 NULL: all zero.  No node set is taken: the caller
 * first gives the response's boundary-proof nodes to kh_trie_fill_nodes (content-addressed against
 * the stubs, so harmless even if the range is then refused).
 * Per range s, trie t, origin o, entries k_1 .. k_m, hi = k_m:
 *   1. keys strictly ascending, k_1 >= o, every value >= 1 byte, else BAD_ORDER (decided before the
 *      handle is read).
 *   2. t not resident (no node at its root; forests only): the entries claim to be the WHOLE trie,
 *      which is built from empty and must hash to roots32[32s..) (required then), else BAD_ROOT;
 *      with m = 0 OK requires EMPTY_TRIE_HASH and loads nothing.
 *   3. t resident: roots32[32s..) must be its current root, else BAD_ROOT (roots32 NULL: no claim).
 *      A live stub whose missing node starts at nibble depth md below key prefix p spans
 *      [p|0..0, p|f..f]; it is INSIDE when that span lies within [o, hi] ([o, ff..ff] when m = 0).
 *      An entry whose walk reaches an inside stub drops the stub: the entries under its prefix
 *      are built in its place.  An entry that reaches any other stub needs a node the handle
 *      lacks: MISSING, and kh_trie_missing lists the (trie, hash) pairs exactly as a refused commit
 *      does.  An inside stub no entry reaches: BAD_ROOT (INCOMPLETE when m = 0).  An entry that
 *      lands on a resident leaf must carry that leaf's value.  The trie's root after the rebuild
 *      must equal its root before; everything else is BAD_ROOT: an omitted key, an invented key,
 *      a changed value, and a value-only branch inside the span (the limit of kh_verify_ranges).
 *   4. All or nothing per call: if any status is not OK the handle is exactly as before (root,
 *      records, export bytes and order, kh_trie_size, kh_trie_stubs, last roots, write-back set)
 *      and the call returns KH_OK with the statuses written: they say which ranges to drop before
 *      a retry.  The ranges are judged in stages -- order, root claims and INCOMPLETE first, then
 *      MISSING, then the rebuilt roots -- and a call refused at one stage leaves the ranges only a
 *      later stage would refuse at OK; a retry without the refused ranges reaches that stage.
 *   5. On success every listed trie keeps its root; kh_trie_size grows by *n_keys, kh_trie_stubs
 *      falls by *n_stubs; stubs_left[s] = live stubs of trie t afterwards (0: the trie is whole).
 *      On a KH_EMIT_NODES handle kh_trie_emit_nodes gives exactly the hash-referenced nodes the
 *      handle did not hold before and holds now (what a sync client writes to its store; a trie
 *      loaded whole includes its root node).  kh_forest_last_roots lists the call's tries with
 *      their unchanged roots.  Export cursors end.
 *   6. OK vouches for the HANDLE: afterwards it holds every key of the trie in [o, hi].  A response
 *      that omits a key the handle already held is not detected; kh_verify_ranges is the call that
 *      judges a response on its own.
 * KH_EINVAL, nothing changed: a null handle or required array; tries NULL on a forest; a trie id
 * listed twice; nr or the entry total >= 2^31; a savepoint open (as for kh_trie_fill_nodes); a
 * trie that is not resident named on a single-trie handle, or on a forest without roots32.
 * nr = 0 is KH_OK.  KH_ENODE is never the return code.
 * status, stubs_left (nullable), n_keys and n_stubs (nullable) are host arrays / scalars.
 * kh_dev_trie_fill_ranges: every input array in HBM on the handle's stream, with the alignment
 * rules and preconditions of kh_dev_verify_ranges (8-byte aligned roots, origins, keys and
 * offsets; d_ent_off[0] = 0; monotone offsets). */
int kh_trie_fill_ranges_host(kh_trie* h, const uint32_t* tries, const uint8_t* roots32,
                             const uint8_t* origins32, uint64_t nr,
                             const uint8_t* keys32, const uint8_t* vals, const uint64_t* voff,
                             const uint64_t* ent_off,
                             uint8_t* status, uint64_t* stubs_left,
                             uint64_t* n_keys, uint64_t* n_stubs);
int kh_dev_trie_fill_ranges(kh_trie* h, const uint32_t* d_tries, const uint8_t* d_roots32,
                            const uint8_t* d_origins32, uint64_t nr,
                            const uint8_t* d_keys32, const uint8_t* d_vals, const uint64_t* d_voff,
                            const uint64_t* d_ent_off,
                            uint8_t* status, uint64_t* stubs_left,
                            uint64_t* n_keys, uint64_t* n_stubs);

/* HBM held by a resident trie or forest.  Records and the value heap are append-only between
 * compactions: a commit appends the records and values it makes and leaves the ones it
 * replaces dead (~18 MB per configs[2] block).  records / heap_bytes: in use; live_records /
 * live_heap_bytes: the current version's (counted on the device); map_slots: anchor-map
 * capacity; hbm_bytes: every buffer the handle holds. */
typedef struct kh_trie_usage_t {
  uint64_t records, live_records, heap_bytes, live_heap_bytes, map_slots, hbm_bytes;
} kh_trie_usage_t;
int kh_trie_usage(kh_trie* h, kh_trie_usage_t* u);
/* Rewrite the live records and their values densely and rebuild the anchor map (O(records)
 * on the device; the version -- roots, last roots, write-back set -- is unchanged).  The JVM
 * calls it between blocks when dead records pass a budget.  KH_EINVAL while a savepoint is
 * open (the journal holds record indices).  before (nullable): records / heap bytes before. */
int kh_trie_compact(kh_trie* h, kh_trie_usage_t* before);
int kh_trie_size(const kh_trie* h, uint64_t* n);
int kh_trie_free(kh_trie* h);

/* Synthetic account generator (pinned in khipu_amd/csrc/synth.h): writes
 * accounts [first, first+n) of config `cfg` — 20-byte addresses (d_addr, n*20 B) and RLP
 * account bodies packed at d_vals with d_voff[n+1] (offsets relative to d_vals; d_vals
 * must hold n*96 B).  Deterministic; the CPU restatement lives in tests. */
int kh_dev_synth_accounts(kh_ctx* ctx, uint32_t cfg, uint64_t first, uint64_t n, uint8_t* d_addr,
                          uint8_t* d_vals, uint64_t* d_voff);

/* Synthetic contract storage tries [t0, t0+nt) of config cfg (pinned in
 * khipu_amd/csrc/synth.h: log-uniform 1..10^4 slots per trie, 32-byte big-endian slot
 * words as keys -- hash them with KH_HASH_KEYS -- and RLP(trimmed 1-32 byte) values).
 * Always: d_seg_off[nt+1] (each trie's first slot, from 0), *n_slots, *val_bytes.  With
 * d_keys non-NULL also the slots: keys (n_slots*32 B), packed values (d_vals, val_bytes B)
 * with d_voff[n_slots+1], and d_seg[n_slots] = trie - t0 (the segment ids of
 * kh_dev_trie_build).  Deterministic per trie: any range can be made on any GPU. */
int kh_dev_synth_storage(kh_ctx* ctx, uint32_t cfg, uint64_t t0, uint64_t nt, uint64_t* d_seg_off, uint64_t* n_slots,
                         uint64_t* val_bytes, uint8_t* d_keys, uint8_t* d_vals, uint64_t* d_voff, uint32_t* d_seg);

#ifdef __cplusplus
}
#endif
#endif /* KHST_H */
