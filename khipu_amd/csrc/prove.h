// Merkle proofs (kh_trie_prove, kh_verify_proofs): the walk that records the nodes on a key's
// path through the records, and the walk that checks such a list of nodes against a root.
//
// A proof of a key is the list of nodes MerklePatriciaTrie.get (MerklePatriciaTrie.scala:90-147)
// visits from the trie's root, root first, restricted to the nodes a node store holds (export.h's
// rule: the encoding is >= 32 B, or the node is the root).  On the records this is forest_get's
// descent: every record it passes contributes its UPPER node, then its LOWER node (the branch
// under an extension) unless the key leaves the extension.  A HIT names one such node:
// 2 * record + (1 for the lower node), the list form export_kernels.hip already encodes.
//
// KH_HD bodies only (the kernels are prove_kernels.hip's, the host replay tests/prove_host's).
#pragma once
#include "export.h"

namespace khst {

// The proof walk of one key: hit(h) for every listed node in root-first order; returns whether
// the key is present.  The count pass and the fill pass both run this body.
// A walk that reaches a stub (forest.h EL_STUB) returns 2 (KH_FOUND_UNKNOWN): the nodes listed so
// far are the resident part of the proof.
template <typename Hit>
KH_HD uint32_t prove_walk(const AMap& M, const Recs& R, uint32_t t, const uint64_t* key, Hit hit) {
  uint32_t d = 0;
  for (int step = 0; step < 70; ++step) {
    const uint32_t r = map_find(M, R, t, d, key);
    if (r == NONE) return false;  // an empty trie, or a branch's empty slot
    const uint32_t db = R.rdb[r];
    if (db == EL_STUB) {  // the extension above a missing branch is resident (export.h); the branch is not
      const uint32_t md = R.rmask[r] & 0xFF;
      if (md > d && (R.rrl[r] == 32 || d == 0)) hit(2ull * r);
      return (md > d && lcp_nibbles(load_key(key, 0), load_key(R.key(r), 0)) < (int)md) ? 0 : 2;
    }
    if (R.rrl[r] == 32 || d == 0) hit(2ull * r);
    const uint64_t* L = R.key(r);
    const bool same = L[0] == key[0] && L[1] == key[1] && L[2] == key[2] && L[3] == key[3];
    if (db == EL_LEAF) return same;  // the leaf reached, whether or not it holds the key
    if (exp_has_lower(d, db)) {
      if (lcp_nibbles(load_key(key, 0), load_key(L, 0)) < (int)db) return false;  // leaves the extension
      if (R.rbrl[r] == 32) hit(2ull * r + 1);
    }
    if (db == VB_DEPTH) return same;  // a value-only branch holds one key
    d = db + 1;
  }
  return false;
}

// ---- verification
enum ProofStatus : uint8_t {
  PROOF_ABSENT = 0,
  PROOF_VALUE = 1,
  PROOF_BAD_HASH = 2,
  PROOF_BAD_NODE = 3,
  PROOF_SHORT = 4,
  PROOF_EXTRA = 5,
};

// the node table a proof points into: encodings, their offsets and their kec256 (4 words each)
struct ProofTable {
  const uint8_t* rlp;
  const uint64_t* off;
  const uint64_t* hash;
  uint64_t n_nodes;
};

KH_HD uint32_t key_nibble(const uint8_t* key, uint32_t i) { return (i & 1) ? key[i >> 1] & 0xFu : key[i >> 1] >> 4; }

// The walk of one 32-byte key under root32 over the listed nodes path[0, np).  The first
// condition met, in walk order, decides the status; *val / *vlen name the value's bytes inside
// the table when the status is PROOF_VALUE (else *vlen = 0).
KH_HD uint8_t proof_walk(const ProofTable& T, const uint8_t* root32, const uint8_t* key, const uint32_t* path,
                         uint64_t np, const uint8_t** val, uint32_t* vlen) {
  *val = nullptr;
  *vlen = 0;
  if (np == 0) return bytes_eq32(root32, empty_root_hash()) ? PROOF_ABSENT : PROOF_SHORT;
  const uint8_t* expect = root32;
  uint64_t k = 0;
  uint32_t nib = 0;
  uint8_t end = PROOF_ABSENT;  // the status the walk ends with, if the list ends there too
  bool ended = false;
  while (!ended) {
    if (k == np) return PROOF_SHORT;
    const uint64_t j = path[k++];
    if (j >= T.n_nodes) return PROOF_BAD_NODE;
    if (!bytes_eq32((const uint8_t*)(T.hash + 4 * j), expect)) return PROOF_BAD_HASH;
    const uint64_t len64 = T.off[j + 1] - T.off[j];
    if (len64 > 0xFFFFFFFFull) return PROOF_BAD_NODE;
    const uint8_t* d = T.rlp + T.off[j];
    const uint32_t n = (uint32_t)len64;
    uint32_t pos = 0;
    bool top = true;
    for (;;) {  // the node at d[pos..): the listed one, then the nodes embedded in it
      RItem L;
      if (!rlp_at(d, n, pos, L) || !L.list) return PROOF_BAD_NODE;
      if (top && L.next != n) return PROOF_BAD_NODE;  // (bytes after the node)
      top = false;
      RItem it[17];
      const int cnt = rlp_items(d, n, L, it, 17);
      int c;  // the item that holds the child
      if (cnt == 17) {
        if (nib == 64) {  // the 64 nibbles are used up: the branch's own value
          if (it[16].list) return PROOF_BAD_NODE;
          if (it[16].len) {
            end = PROOF_VALUE;
            *val = d + it[16].off;
            *vlen = it[16].len;
          }
          ended = true;
          break;
        }
        c = (int)key_nibble(key, nib++);
      } else if (cnt == 2) {
        if (it[0].list || it[0].len == 0) return PROOF_BAD_NODE;
        const uint8_t* hp = d + it[0].off;
        const uint32_t flag = hp[0] >> 4, odd = flag & 1;
        if (flag > 3 || (!odd && (hp[0] & 0xF))) return PROOF_BAD_NODE;
        const uint32_t pn = 2 * (it[0].len - 1) + odd;
        if (nib + pn > 64) return PROOF_BAD_NODE;
        const bool leaf = (flag & 2) != 0;
        if (leaf && it[1].list) return PROOF_BAD_NODE;
        bool match = true;
        for (uint32_t i = 0; i < pn && match; ++i) {
          const uint32_t q = i + 1 - odd;  // nibble q + 1 of the HexPrefix bytes
          match = key_nibble(hp, q + 1) == key_nibble(key, nib + i);
        }
        if (!match || (leaf && nib + pn != 64)) {  // the key leaves the path: absent
          ended = true;
          break;
        }
        if (leaf) {
          end = PROOF_VALUE;
          *val = d + it[1].off;
          *vlen = it[1].len;
          ended = true;
          break;
        }
        nib += pn;
        c = 1;
      } else {
        return PROOF_BAD_NODE;  // (a list overrun included: cnt < 0)
      }
      const RItem& ch = it[c];
      if (!ch.list) {
        if (ch.len == 0) {  // an empty child: absent
          ended = true;
          break;
        }
        if (ch.len != 32) return PROOF_BAD_NODE;
        expect = d + ch.off;
        break;  // the next listed node
      }
      const uint32_t start = c ? it[c - 1].next : L.off;
      if (ch.next - start >= 32) return PROOF_BAD_NODE;  // an embedded node is shorter than a hash
      pos = start;
    }
  }
  if (k != np) {
    *val = nullptr;
    *vlen = 0;
    return PROOF_EXTRA;
  }
  return end;
}

}  // namespace khst
