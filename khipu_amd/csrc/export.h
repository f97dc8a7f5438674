// Record -> node encoding: the nodes a resident trie's records stand for, re-derived from the
// records alone (kh_trie_export_nodes, kh_trie_nodes_by_hash).  The commit path caches two capped
// references per record (forest.h); nothing here reads an encoding the commit path made: a node
// is rebuilt from the record's key, depths, child mask and value, and from the references of
// its children's records, found by their anchors.
//
// A live record r (trie t, anchor depth d, branch depth db) stands for
//   a leaf              (db == EL_LEAF):  RLP[HP(nibbles d..64, leaf), value]
//   a value-only branch (db == VB_DEPTH): vb_encode(value)
//   a branch            (db < 64):        RLP[ref_0 .. ref_15, ""], ref_c the capped reference
//                                         (rref / rrl) of the record at anchor (t, db + 1, key
//                                         with nibble db = c), for every bit c of rmask
//   and, when d < db, the extension above that branch: RLP[HP(nibbles d..db, ext), bref].
// The UPPER node of a record is the one its parent refers to (rref); the LOWER node is the
// branch under an extension (rbref).  A node belongs to a node store when its capped reference
// is a hash (length 32: the encoding is >= 32 B), or when it is a trie's root node (the upper
// node of the record at anchor depth 0; with 32-byte keys its encoding is >= 32 B as well, so
// its hash is the stored reference too and no Keccak is needed to name a node).
//
// KH_HD bodies only: 16 lanes work on a record (lane c owns child c); the bodies are written per
// lane, the sums over the 16 lanes are the caller's (shuffles in export_kernels.hip, a loop in
// the host replay of tests/export_host).
#pragma once
#include "forest.h"

namespace khst {

constexpr uint32_t EXP_LANES = 16;
constexpr uint32_t EXP_UPPER = 1, EXP_LOWER = 2;  // node selection bits
constexpr uint32_t EXP_ALL_TRIES = 0xFFFFFFFFu;   // (KH_NO_TRIE)
constexpr uint64_t EXP_NO_HIT = ~0ULL;            // by-hash: hit = 2 * record + (1: the lower node)

KH_HD bool exp_has_lower(uint32_t d, uint32_t db) { return db != EL_LEAF && d < db; }
// a node written as a list of 17 items: a branch (a value-only branch is written by vb_encode)
// A stub (forest.h EL_STUB) stands for a node the handle does not hold: it is never selected and
// never answers by hash, except for the extension it still holds above a missing branch (rmask >
// d), which is its upper node; as a child it gives its parent the reference it keeps, rref, like
// any other record.  exp_db: the depth at which a record's lower node starts.
KH_HD bool exp_is_branch(uint32_t db) { return db != EL_LEAF && db != VB_DEPTH && db != EL_STUB; }
KH_HD uint32_t exp_db(const Recs& R, uint64_t r) { return R.rdb[r] == EL_STUB ? (R.rmask[r] & 0xFFu) : R.rdb[r]; }

// the nodes of record r a node store needs (trie filter applied)
KH_HD uint32_t exp_select(const Recs& R, uint64_t r, uint32_t filter) {
  if (R.rlive[r] != REC_LIVE) return 0;
  if (filter != EXP_ALL_TRIES && R.rt[r] != filter) return 0;
  const uint32_t d = R.rd[r], db = R.rdb[r];
  if (db == EL_STUB)  // the subtree is not held; the extension above a missing branch is
    return (exp_db(R, r) > d && (R.rrl[r] == 32 || d == 0)) ? EXP_UPPER : 0;
  uint32_t sel = (R.rrl[r] == 32 || d == 0) ? EXP_UPPER : 0;
  if (exp_has_lower(d, db) && R.rbrl[r] == 32) sel |= EXP_LOWER;
  return sel;
}
// does writing the selected nodes need the children's references?
KH_HD bool exp_needs_children(const Recs& R, uint64_t r, uint32_t sel) {
  const uint32_t d = R.rd[r], db = R.rdb[r];
  if (!exp_is_branch(db)) return false;
  return (sel & EXP_LOWER) || ((sel & EXP_UPPER) && d == db);
}

// lane c: the record of child c of branch record r (NONE: no such child)
KH_HD uint32_t exp_child(const Recs& R, const AMap& M, uint64_t r, uint32_t c) {
  const uint32_t db = R.rdb[r];
  if (!exp_is_branch(db) || !((R.rmask[r] >> c) & 1)) return NONE;
  uint64_t k[4];
  for (int q = 0; q < 4; ++q) k[q] = R.rk[4 * r + q];
  set_nibble(k, db, c);
  return map_find(M, R, R.rt[r], db + 1, k);
}
// lane c: bytes of child c's item in its parent's list
KH_HD uint32_t exp_item_len(const Recs& R, uint32_t child) {
  if (child == NONE) return 1;
  const uint32_t rl = R.rrl[child];
  return rl == 32 ? 33 : rl;
}

KH_HD uint32_t exp_list_len(uint32_t payload) { return rlp_hdr_len(payload) + payload; }
KH_HD uint32_t exp_hp_item_len(uint32_t nibbles) {  // HP path as an RLP string (one byte: < 0x80)
  const uint32_t hb = nibbles / 2 + 1;
  return hb == 1 ? 1 : 1 + hb;
}
KH_HD uint32_t exp_value_item_len(const Recs& R, const uint8_t* heap, uint64_t r) {
  const uint32_t vl = R.rvl[r];
  return (uint32_t)rlp_str_len(vl, vl == 1 ? heap[R.rvo[r]] : 0x80u);
}
// encoded lengths; S = the sum of the 16 children's item lengths (branches)
KH_HD uint32_t exp_branch_len(uint32_t S) { return exp_list_len(S + 1); }
KH_HD uint32_t exp_lower_len(const Recs& R, const uint8_t* heap, uint64_t r, uint32_t S) {
  return R.rdb[r] == VB_DEPTH ? exp_list_len(16 + exp_value_item_len(R, heap, r)) : exp_branch_len(S);
}
KH_HD uint32_t exp_upper_len(const Recs& R, const uint8_t* heap, uint64_t r, uint32_t S) {
  const uint32_t d = R.rd[r], db = exp_db(R, r);
  if (db == EL_LEAF) return exp_list_len(exp_hp_item_len(64 - d) + exp_value_item_len(R, heap, r));
  if (d < db) {
    const uint32_t brl = R.rbrl[r];
    return exp_list_len(exp_hp_item_len(db - d) + (brl == 32 ? 33 : brl));
  }
  return exp_lower_len(R, heap, r, S);
}
// sizes form: node count and bytes of the selected nodes of record r
KH_HD void exp_sizes(const Recs& R, const uint8_t* heap, uint64_t r, uint32_t sel, uint32_t S, uint32_t* cnt,
                     uint32_t* bytes) {
  uint32_t n = 0, b = 0;
  if (sel & EXP_UPPER) {
    ++n;
    b += exp_upper_len(R, heap, r, S);
  }
  if (sel & EXP_LOWER) {
    ++n;
    b += exp_lower_len(R, heap, r, S);
  }
  *cnt = n;
  *bytes = b;
}

// ---- write form (per lane; pre = the sum of the item lengths of the lanes below this one)
KH_HD uint32_t exp_put_hp(const uint8_t* key, uint32_t from, uint32_t to, bool leaf, uint8_t* out, uint32_t p) {
  const uint32_t nn = to - from, odd = nn & 1, hb = nn / 2 + 1;
  if (hb > 1) out[p++] = (uint8_t)(0x80 + hb);
  const uint32_t flag = (leaf ? 2u : 0u) + odd;
  out[p++] = (uint8_t)((flag << 4) | (odd ? ((from & 1) ? key[from >> 1] & 0xF : key[from >> 1] >> 4) : 0));
  if (((from + odd) & 1) == 0) {  // whole key bytes follow
    for (uint32_t j = (from + odd) >> 1; j < (to >> 1); ++j) out[p++] = key[j];
  } else {  // (an odd branch depth under an even anchor: byte-straddling pairs)
    for (uint32_t i = from + odd; i < to; i += 2)
      out[p++] = (uint8_t)(((key[i >> 1] & 0xF) << 4) | (key[(i + 1) >> 1] >> 4));
  }
  return p;
}
// a branch body: lane 0 the list header and the empty value, lane c child c's item
KH_HD void exp_write_branch(const Recs& R, uint32_t lane, uint32_t child, uint32_t pre, uint32_t S, uint8_t* out) {
  const uint32_t hdr = rlp_hdr_len(S + 1);
  if (lane == 0) {
    vb_put_len(out, 0, S + 1, 0xC0);
    out[hdr + S] = 0x80;
  }
  uint32_t p = hdr + pre;
  if (child == NONE) {
    out[p] = 0x80;
    return;
  }
  const uint32_t rl = R.rrl[child];
  const uint8_t* ref = (const uint8_t*)&R.rref[4ull * child];
  if (rl == 32) out[p++] = 0xA0;
  for (uint32_t i = 0; i < rl; ++i) out[p++] = ref[i];
}
// a leaf or a value-only branch: lane 0 the headers, the value's bytes strided over the lanes
KH_HD void exp_write_valued(const Recs& R, const uint8_t* heap, uint64_t r, uint32_t lane, uint8_t* out) {
  const uint32_t d = R.rd[r], vl = R.rvl[r];
  const bool vb = R.rdb[r] == VB_DEPTH;
  const uint8_t* val = heap + R.rvo[r];
  const uint32_t vitem = exp_value_item_len(R, heap, r);
  const uint32_t payload = (vb ? 16 : exp_hp_item_len(64 - d)) + vitem;
  const uint32_t vstart = rlp_hdr_len(payload) + payload - vl;  // the value's bytes end the node
  if (lane == 0) {
    uint32_t p = vb_put_len(out, 0, payload, 0xC0);
    if (vb)
      for (int c = 0; c < 16; ++c) out[p++] = 0x80;
    else
      p = exp_put_hp((const uint8_t*)R.key(r), d, 64, true, out, p);
    if (vitem != vl) vb_put_len(out, p, vl, 0x80);  // (a single byte < 0x80 is its own encoding)
  }
  for (uint32_t i = lane; i < vl; i += EXP_LANES) out[vstart + i] = val[i];
}
// the extension above a branch (lane 0)
KH_HD void exp_write_ext(const Recs& R, uint64_t r, uint8_t* out) {
  const uint32_t d = R.rd[r], db = exp_db(R, r), brl = R.rbrl[r];
  const uint32_t payload = exp_hp_item_len(db - d) + (brl == 32 ? 33 : brl);
  uint32_t p = vb_put_len(out, 0, payload, 0xC0);
  p = exp_put_hp((const uint8_t*)R.key(r), d, db, false, out, p);
  const uint8_t* ref = (const uint8_t*)&R.rbref[4 * r];
  if (brl == 32) out[p++] = 0xA0;
  for (uint32_t i = 0; i < brl; ++i) out[p++] = ref[i];
}
// lane's share of the selected nodes of record r, the upper node first, packed at out; returns
// through len[2] the lengths written (0: not selected)
KH_HD void exp_write(const Recs& R, const uint8_t* heap, uint64_t r, uint32_t sel, uint32_t lane, uint32_t child,
                     uint32_t pre, uint32_t S, uint8_t* out, uint32_t len[2]) {
  const uint32_t d = R.rd[r], db = exp_db(R, r);  // (a stub is selected for its extension only: d < db)
  len[0] = len[1] = 0;
  if (sel & EXP_UPPER) {
    len[0] = exp_upper_len(R, heap, r, S);
    if (db == EL_LEAF || (db == VB_DEPTH && d == db))
      exp_write_valued(R, heap, r, lane, out);
    else if (d < db) {
      if (lane == 0) exp_write_ext(R, r, out);
    } else
      exp_write_branch(R, lane, child, pre, S, out);
  }
  if (sel & EXP_LOWER) {
    len[1] = exp_lower_len(R, heap, r, S);
    if (db == VB_DEPTH)
      exp_write_valued(R, heap, r, lane, out + len[0]);
    else
      exp_write_branch(R, lane, child, pre, S, out + len[0]);
  }
}
// the stored reference that names a selected node
KH_HD const uint8_t* exp_hash_of(const Recs& R, uint64_t r, uint32_t which) {
  return which == EXP_LOWER ? (const uint8_t*)&R.rbref[4 * r] : (const uint8_t*)&R.rref[4 * r];
}

// KH_EXPORT_VERIFY: node j of an emitted set (hashes | packed encodings | off) re-hashed with the
// library's Keccak and compared with the reference it was named by; true on a mismatch.  The
// encodings lie in an 8-byte-aligned buffer padded to a whole word (kec256_msg reads words).
KH_HD bool exp_verify(const uint8_t* hashes, const uint8_t* rlp, const uint64_t* off, uint64_t j) {
  const uint32_t len = (uint32_t)(off[j + 1] - off[j]);
  if (len < 32) return true;  // a node store holds no such node (32-byte keys: not even a root)
  uint64_t h[4];
  kec256_msg<false>(rlp + off[j], len, h);
  const uint8_t* a = hashes + 32 * j;
  const uint8_t* b = (const uint8_t*)h;
  bool bad = false;
  for (int i = 0; i < 32; ++i) bad = bad || a[i] != b[i];
  return bad;
}

// ---- by-hash: the query table (open addressing; tag = the hash's first 8 bytes, 0 = empty)
KH_HD uint64_t exp_tag(uint64_t w0) { return w0 ? w0 : 1; }
KH_HD uint32_t exp_tag_slot(uint64_t tag, uint32_t mask) { return (uint32_t)fmix64(tag) & mask; }
// every query slot holding hash w gets `hit`
KH_HD void exp_table_match(const uint64_t* tags, const uint16_t* qidx, uint32_t mask, const uint64_t* Q,
                           const uint64_t* w, uint64_t hit, uint64_t* hits) {
  const uint64_t tag = exp_tag(w[0]);
  for (uint32_t s = exp_tag_slot(tag, mask), n = 0; n <= mask; s = (s + 1) & mask, ++n) {
    const uint64_t g = tags[s];
    if (g == 0) return;
    if (g != tag) continue;
    const uint32_t q = qidx[s];
    if (Q[4 * q] == w[0] && Q[4 * q + 1] == w[1] && Q[4 * q + 2] == w[2] && Q[4 * q + 3] == w[3]) hits[q] = hit;
  }
}
// record r's two references against the table
KH_HD void exp_scan_record(const Recs& R, uint64_t r, const uint64_t* tags, const uint16_t* qidx, uint32_t mask,
                           const uint64_t* Q, uint64_t* hits) {
  if (R.rlive[r] != REC_LIVE) return;
  const uint32_t d = R.rd[r], db = R.rdb[r];
  const bool stub = db == EL_STUB;  // it answers for the extension it holds, never for the missing node
  if (stub && exp_db(R, r) <= d) return;
  uint64_t w[4];
  if (R.rrl[r] == 32) {
    for (int q = 0; q < 4; ++q) w[q] = R.rref[4 * r + q];
    exp_table_match(tags, qidx, mask, Q, w, 2 * r, hits);
  }
  if (!stub && exp_has_lower(d, db) && R.rbrl[r] == 32) {
    for (int q = 0; q < 4; ++q) w[q] = R.rbref[4 * r + q];
    exp_table_match(tags, qidx, mask, Q, w, 2 * r + 1, hits);
  }
}

}  // namespace khst
