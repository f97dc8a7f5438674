"""Device-resident interface of libkhst.so for inputs already in HBM.

torch is used only as the HBM allocator (tensors' data pointers are handed to
the C ABI); all compute is libkhst.so's HIP kernels.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import KhStats, check, lib


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class Ctx:
    """One kh_ctx (device workspace + HIP stream) per GPU."""

    def __init__(self, device=0):
        import torch
        self.torch = torch
        self.device = device
        torch.cuda.set_device(device)
        h = ctypes.c_void_p()
        check(lib().kh_ctx_create(device, ctypes.byref(h)))
        self.h = h

    def close(self):
        if self.h:
            lib().kh_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _sync(self):
        self.torch.cuda.synchronize(self.device)

    def synth_accounts(self, cfg, first, n):
        """Synthetic accounts [first, first+n) of config cfg (csrc/synth.h):
        (addresses uint8[n*20], values uint8[<=96n], offsets int64[n+1]) on the device."""
        t = self.torch
        dev = f"cuda:{self.device}"
        addr = t.empty(n * 20 + 64, dtype=t.uint8, device=dev)
        vals = t.empty(n * 96 + 64, dtype=t.uint8, device=dev)
        voff = t.empty(n + 1, dtype=t.int64, device=dev)
        self._sync()
        check(lib().kh_dev_synth_accounts(self.h, cfg, first, n, _ptr(addr), _ptr(vals), _ptr(voff)))
        return addr, vals, voff

    def storage_slot_counts(self, cfg, t0, nt):
        """Slot offsets int64[nt+1] (device) of synthetic storage tries [t0, t0+nt) and the total."""
        t = self.torch
        so = t.empty(nt + 1, dtype=t.int64, device=f"cuda:{self.device}")
        ns, vb = ctypes.c_uint64(), ctypes.c_uint64()
        self._sync()
        check(lib().kh_dev_synth_storage(self.h, cfg, t0, nt, _ptr(so), ctypes.byref(ns), ctypes.byref(vb), None, None,
                                         None, None))
        return so, int(ns.value), int(vb.value)

    def synth_storage(self, cfg, t0, nt):
        """Synthetic storage tries [t0, t0+nt) of config cfg (csrc/synth.h): (slot offsets
        int64[nt+1], keys uint8[n*32] (32-byte slot words: build with hash_keys), values,
        value offsets int64[n+1], segment ids int32[n]) on the device."""
        t = self.torch
        dev = f"cuda:{self.device}"
        so, n, vb = self.storage_slot_counts(cfg, t0, nt)
        keys = t.empty(n * 32 + 64, dtype=t.uint8, device=dev)
        vals = t.empty(vb + 64, dtype=t.uint8, device=dev)
        voff = t.empty(n + 1, dtype=t.int64, device=dev)
        seg = t.empty(n + 16, dtype=t.int32, device=dev)
        ns, vb2 = ctypes.c_uint64(), ctypes.c_uint64()
        check(lib().kh_dev_synth_storage(self.h, cfg, t0, nt, _ptr(so), ctypes.byref(ns), ctypes.byref(vb2),
                                         _ptr(keys), _ptr(vals), _ptr(voff), _ptr(seg)))
        return so, keys, vals, voff, seg

    def kec256(self, data, off, n):
        t = self.torch
        out = t.empty(32 * max(n, 1), dtype=t.uint8, device=data.device)
        self._sync()
        check(lib().kh_dev_kec256_batch(self.h, _ptr(data), _ptr(off), n, _ptr(out)))
        self._sync()
        return out[:32 * n]

    def build(self, keys, klen, vals, voff, n, seg=None, nseg=1, depth0=0, hash_keys=False, vals_ready=None):
        """Returns (hash32 [nres,32] uint8, enc_len [nres] uint32, inline [nres,32] uint8, KhStats).
        vals_ready: a torch.cuda.Event after which vals / voff are in place
        (kh_dev_trie_build_ev); the keys must be in place already, and the build does
        not synchronise the device first."""
        nres = nseg if seg is not None else (16 if depth0 == 1 else 1)
        hh = np.zeros(32 * nres, np.uint8)
        ll = np.zeros(nres, np.uint32)
        ii = np.zeros(32 * nres, np.uint8)
        st = KhStats()
        flags = _lib.KH_HASH_KEYS if hash_keys else 0
        if vals_ready is None:
            self._sync()
            ev = None
        else:
            ev = ctypes.c_void_p(vals_ready.cuda_event)
        check(lib().kh_dev_trie_build_ev(self.h, ev, _ptr(keys), klen, _ptr(vals), _ptr(voff), n, _ptr(seg), nseg,
                                         depth0, flags, hh.ctypes.data, ll.ctypes.data, ii.ctypes.data,
                                         ctypes.byref(st)))
        return hh.reshape(nres, 32), ll, ii.reshape(nres, 32), st

    def list_roots(self, items, off, seg_off):
        """kh_dev_list_roots: items / off (n + 1 int64 offsets) device tensors, seg_off host
        (numpy uint64, nseg + 1).  Returns (list of 32-byte roots, KhStats)."""
        so = np.ascontiguousarray(seg_off, dtype=np.uint64)
        nseg = len(so) - 1
        out = np.zeros(32 * max(nseg, 1), np.uint8)
        st = KhStats()
        self._sync()
        check(lib().kh_dev_list_roots(self.h, _ptr(items), _ptr(off), so.ctypes.data, nseg, out.ctypes.data,
                                      ctypes.byref(st)))
        return [out[32 * i:32 * i + 32].tobytes() for i in range(nseg)], st


def fold_root16(hash32x16, len16, inline32x16):
    """Root over 16 capped top-nibble references (kh_fold_root16)."""
    hh = np.ascontiguousarray(hash32x16, dtype=np.uint8).reshape(-1)
    ll = np.ascontiguousarray(len16, dtype=np.uint32)
    ii = np.ascontiguousarray(inline32x16, dtype=np.uint8).reshape(-1)
    out = np.zeros(32, np.uint8)
    check(lib().kh_fold_root16(hh.ctypes.data, ll.ctypes.data, ii.ctypes.data, out.ctypes.data))
    return out.tobytes()


def _pack_dev(items, device):
    """bytes list -> (uint8 data, int64 offsets[n+1]) tensors on the device."""
    import torch
    blob = b"".join(items)
    data = torch.zeros(len(blob) + 64, dtype=torch.uint8)
    if blob:
        data[:len(blob)] = torch.frombuffer(bytearray(blob), dtype=torch.uint8)
    off = torch.tensor(np.concatenate([[0], np.cumsum([len(x) for x in items], dtype=np.int64)]).astype(np.int64))
    return data.to(device), off.to(device)


class _Versioned:
    """Versioned commits shared by ResidentTrie and ResidentForest (kh_trie_savepoint /
    kh_trie_rollback / kh_trie_release; Ledger.executeBlock's retry from the parent state,
    Ledger.scala:237-271, and the rejection of validateBlockAfterExecution, :603-620)."""

    def savepoint(self):
        """Open a savepoint (they nest); returns the number now open."""
        d = ctypes.c_uint32()
        check(lib().kh_trie_savepoint(self.h, ctypes.byref(d)))
        return int(d.value)

    def rollback(self):
        """Back to the innermost savepoint's version (root, records, last roots, write-back set)."""
        self.ctx._sync()
        check(lib().kh_trie_rollback(self.h))
        self._after_rollback()

    def release(self):
        """Keep the commits since the innermost savepoint and close it."""
        check(lib().kh_trie_release(self.h))

    def savepoint_depth(self):
        d = ctypes.c_uint32()
        check(lib().kh_trie_savepoint_depth(self.h, ctypes.byref(d)))
        return int(d.value)

    def _after_rollback(self):
        pass

    def changes_since(self, level=0, reverse=False, start=None, max_entries=1024, val_cap=1 << 20):
        """One page of the keys whose entries differ between the version at an open savepoint (level
        0: the innermost; 1 .. depth: counted from the outermost) and the current version, read from
        the journal without a copy (kh_trie_changes_since_host): (entries, more, next, n_total).
        entries = [(key, kind, value)] in key order, on a forest [(trie, key, kind, value)] in (trie,
        key) order, with the kinds of diff(): savepoint = side a, current = side b, and the current
        values; reverse: the sides swapped and the savepoint's values (the ops that undo the commits).
        start / next: a key, on a forest a (trie, key) pair; n_total counts the differences from start
        on, returned or not.  KH_ENOSPC raises KhError with .val_bytes and .n_total."""
        self.ctx._sync()
        return trie_changes_since(self.h, isinstance(self, ResidentForest), level, reverse, start, max_entries, val_cap)

    def changes_since_all(self, level=0, reverse=False):
        """changes_since() in one call sized from n_total (val_cap grows on KH_ENOSPC): the (upserts,
        deletes) of the commit that brings the savepoint's version to the current one (reverse: back),
        upserts [(key, value)] and deletes [key], on a forest [(trie, key, value)] and [(trie, key)]."""
        self.ctx._sync()
        forest = isinstance(self, ResidentForest)
        n, val_cap, start, ups, dels = 1024, 1 << 20, None, [], []
        while True:
            try:
                ents, more, nxt, total = trie_changes_since(self.h, forest, level, reverse, start, n, val_cap)
            except _lib.KhError as e:
                if e.code != _lib.KH_ENOSPC:
                    raise
                n, val_cap = max(n, e.n_total), max(2 * val_cap, e.val_bytes)
                continue
            for e in ents:
                if e[-2] == _lib.KH_DIFF_ONLY_A:
                    dels.append(e[:-2] if forest else e[0])
                else:
                    ups.append(e[:-2] + e[-1:])
            if not more:
                return ups, dels
            if len(ents) < n:  # (the values cut the page, not the entries)
                val_cap *= 2
            start, n = nxt, max(n, total - len(ents))

    def usage(self):
        """{records, live_records, heap_bytes, live_heap_bytes, map_slots, hbm_bytes} (kh_trie_usage)."""
        u = _lib.KhTrieUsage()
        self.ctx._sync()
        check(lib().kh_trie_usage(self.h, ctypes.byref(u)))
        return {f: int(getattr(u, f)) for f, _ in u._fields_}

    def compact(self):
        """Rewrite the live records and values densely (kh_trie_compact); the version is unchanged.
        Returns {records, heap_bytes} before it."""
        u = _lib.KhTrieUsage()
        self.ctx._sync()
        check(lib().kh_trie_compact(self.h, ctypes.byref(u)))
        return {"records": int(u.records), "heap_bytes": int(u.heap_bytes)}

    def export_cursor(self):
        """A fresh kh_export_cursor for export_chunk."""
        return _lib.KhExportCursor()

    def export_chunk(self, cur, trie=None, verify=False, node_cap=1 << 16, rlp_cap=1 << 23):
        """One kh_trie_export_nodes call: ([(hash, encoding)], done).  KH_ENOSPC (not even the next
        record's nodes fit) and KH_EINVAL (a cursor from before a commit, rollback or compaction)
        raise; the cursor is then unchanged."""
        hs = np.zeros(32 * max(node_cap, 1), np.uint8)
        rl = np.zeros(max(rlp_cap, 1), np.uint8)
        of = np.zeros(node_cap + 1, np.uint64)
        nn, nl, done = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_int(0)
        self.ctx._sync()
        rc = lib().kh_trie_export_nodes(self.h, _lib.KH_NO_TRIE if trie is None else int(trie),
                                        _lib.KH_EXPORT_VERIFY if verify else 0, ctypes.byref(cur), hs.ctypes.data,
                                        node_cap, rl.ctypes.data, rlp_cap, of.ctypes.data, ctypes.byref(nn),
                                        ctypes.byref(nl), ctypes.byref(done))
        if rc == _lib.KH_ENOSPC:
            e = _lib.KhError(rc, lib().kh_last_error().decode(errors="replace"))
            e.needed = (int(nn.value), int(nl.value))
            raise e
        check(rc)
        return [(hs[32 * i:32 * i + 32].tobytes(), rl[of[i]:of[i + 1]].tobytes()) for i in range(nn.value)], bool(done.value)

    def export_nodes(self, trie=None, verify=False, node_cap=1 << 16, rlp_cap=1 << 23):
        """Every node of the current version a node store needs, as (hash, encoding) pairs
        (kh_trie_export_nodes driven to the end; the buffers grow when one record's nodes do not
        fit).  trie: one trie id of a forest (None: all).  verify: every encoding is re-hashed on
        the device against the reference its record caches."""
        cur = self.export_cursor()
        done = False
        while not done:
            try:
                pairs, done = self.export_chunk(cur, trie, verify, node_cap, rlp_cap)
            except _lib.KhError as e:
                if e.code != _lib.KH_ENOSPC:
                    raise
                node_cap, rlp_cap = max(node_cap, e.needed[0]), max(rlp_cap, e.needed[1])
                continue
            yield from pairs

    # ---- partial handles (from_witness / load_partial): the subtrees a handle lacks are stubs
    @property
    def stubs(self):
        """The live stubs of the handle (kh_trie_stubs); 0 on a handle that holds its tries in full."""
        n = ctypes.c_uint64()
        check(lib().kh_trie_stubs(self.h, ctypes.byref(n)))
        return int(n.value)

    def missing(self):
        """[(trie_id, hash)] the last commit, block commit or root_of needed and the handle lacks
        (kh_trie_missing): what MPTNodeMissingException names in the reference.  Empty unless that
        call raised MPTNodeMissingException.  trie_id is 0 on a ResidentTrie."""
        n = ctypes.c_uint64()
        cap = 0
        for _ in range(3):
            tries = np.zeros(max(cap, 1), np.uint32)
            hs = np.zeros(32 * max(cap, 1), np.uint8)
            rc = lib().kh_trie_missing(self.h, tries.ctypes.data, hs.ctypes.data, cap, ctypes.byref(n))
            if rc == _lib.KH_ENOSPC:
                cap = n.value
                continue
            check(rc)
            return [(int(tries[i]), hs[32 * i:32 * i + 32].tobytes()) for i in range(n.value)]
        raise RuntimeError("kh_trie_missing: size negotiation failed")

    def fill(self, nodes):
        """Resolve the stubs whose node is among `nodes` ({hash: encoding} or a list of encodings;
        kh_trie_fill_nodes); returns the number of nodes decoded into the handle."""
        if isinstance(nodes, ProofTable):
            nodes = nodes.nodes
        encs = list(nodes.values()) if isinstance(nodes, dict) else list(nodes)
        ed, eo = _pack_dev(encs, self.dev)
        n = ctypes.c_uint64()
        self.ctx._sync()
        check(lib().kh_trie_fill_nodes(self.h, _ptr(ed), _ptr(eo), len(encs), ctypes.byref(n), None))
        return int(n.value)

    def _fill_ranges(self, ranges, proof, forest):
        """kh_trie_fill_ranges_host over ranges = [(trie, root or None, origin or None, (keys, vals))]:
        -> (statuses, stubs_left, {"keys", "stubs"}).  A root of None is allowed only when no range
        carries one (no claim)."""
        ranges = [tuple(r) for r in ranges]
        if proof is not None:
            self.fill(proof)
        roots = [r for _, r, _, _ in ranges]
        if any(r is None for r in roots) and not all(r is None for r in roots):
            raise _lib.MPTException(_lib.KH_EINVAL, "a root for every range, or for none")
        claim = bool(roots) and roots[0] is not None
        nr, _, a = _range_arrays(roots if claim else [b"\0" * 32] * len(ranges), [o for _, _, o, _ in ranges],
                                 [e for _, _, _, e in ranges], None, None)
        tb = np.asarray([t for t, _, _, _ in ranges] + [0], np.uint32) if forest else None
        status, left = np.zeros(nr + 1, np.uint8), np.zeros(nr + 1, np.uint64)
        nk, ns = ctypes.c_uint64(), ctypes.c_uint64()
        self.ctx._sync()
        check(lib().kh_trie_fill_ranges_host(self.h, _at(tb), a["roots"].ctypes.data if claim else None,
                                             a["origins"].ctypes.data, nr, a["keys"].ctypes.data,
                                             a["vals"].ctypes.data, a["voff"].ctypes.data, a["ent_off"].ctypes.data,
                                             status.ctypes.data, left.ctypes.data, ctypes.byref(nk), ctypes.byref(ns)))
        return ([int(x) for x in status[:nr]], [int(x) for x in left[:nr]],
                {"keys": int(nk.value), "stubs": int(ns.value)})

    def _evict_subtrees(self, prefixes, trie_ids):
        from .codec import nibbles_to_path32
        prefixes = [list(p) for p in prefixes]
        n = len(prefixes)
        if any(len(p) > 255 for p in prefixes):
            raise ValueError("a prefix is at most 64 nibbles")
        # (a depth above 64 is passed on with its first 64 nibbles: the library refuses it)
        pb = np.frombuffer(b"".join(nibbles_to_path32(p[:64]) for p in prefixes) + b"\0", np.uint8).copy()
        db = np.asarray([len(p) for p in prefixes] + [0], np.uint8)
        tb = np.asarray(list(trie_ids) + [0], np.uint32) if trie_ids is not None else None
        status = np.zeros(max(n, 1), np.uint8)
        hs = np.zeros(32 * max(n, 1), np.uint8)
        ne, nk, nr = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        self.ctx._sync()
        check(lib().kh_trie_evict_subtrees(self.h, tb.ctypes.data if tb is not None else None, pb.ctypes.data,
                                           db.ctypes.data, n, status.ctypes.data, hs.ctypes.data, ctypes.byref(ne),
                                           ctypes.byref(nk), ctypes.byref(nr)))
        res = [(int(status[i]), hs[32 * i:32 * i + 32].tobytes()
                if status[i] in (_lib.KH_EVICT_DONE, _lib.KH_EVICT_STUB) else None) for i in range(n)]
        return res, {"evicted": int(ne.value), "keys": int(nk.value), "records": int(nr.value)}

    def _need(self, keys, trie_ids):
        keys = list(keys)
        n = len(keys)
        klen = len(keys[0]) if keys else 32
        kb = np.frombuffer(b"".join(keys) + b"\0", np.uint8).copy()
        tb = np.asarray(list(trie_ids) + [0], np.uint32) if trie_ids is not None else None
        flag = np.zeros(max(n, 1), np.uint8)
        hs = np.zeros(32 * max(n, 1), np.uint8)
        self.ctx._sync()
        check(lib().kh_trie_need_host(self.h, tb.ctypes.data if tb is not None else None, kb.ctypes.data, klen, n,
                                      flag.ctypes.data, hs.ctypes.data))
        return [hs[32 * i:32 * i + 32].tobytes() if flag[i] else None for i in range(n)]

    def commit_witness_raw(self, up_keys, up_ids, del_keys, del_ids, caps=(0, 0), miss_cap=0, flags=0):
        """One kh_trie_commit_witness_host call with the capacities caps = (nodes, encoding bytes):
        (rc, (n_nodes, rlp_len, n_collapse, n_missing), (hashes, rlp, off, miss_tries, miss_hashes))."""
        up_keys, del_keys = list(up_keys), list(del_keys)
        klen = len(up_keys[0]) if up_keys else (len(del_keys[0]) if del_keys else 32)
        ub = np.frombuffer(b"".join(up_keys) + b"\0", np.uint8).copy()
        db = np.frombuffer(b"".join(del_keys) + b"\0", np.uint8).copy()
        ut = np.asarray(list(up_ids) + [0], np.uint32) if up_ids is not None else None
        dt = np.asarray(list(del_ids) + [0], np.uint32) if del_ids is not None else None
        cn, cb = caps
        hs = np.zeros(32 * max(cn, 1), np.uint8)
        rl = np.zeros(max(cb, 1), np.uint8)
        of = np.zeros(cn + 1, np.uint64)
        mt = np.zeros(max(miss_cap, 1), np.uint32)
        mh = np.zeros(32 * max(miss_cap, 1), np.uint8)
        nn, nl, nc, nm = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        self.ctx._sync()
        rc = lib().kh_trie_commit_witness_host(
            self.h, ut.ctypes.data if ut is not None else None, ub.ctypes.data, len(up_keys),
            dt.ctypes.data if dt is not None else None, db.ctypes.data, len(del_keys), klen, flags, hs.ctypes.data, cn,
            rl.ctypes.data, cb, of.ctypes.data, ctypes.byref(nn), ctypes.byref(nl), ctypes.byref(nc), mt.ctypes.data,
            mh.ctypes.data, miss_cap, ctypes.byref(nm))
        return rc, (int(nn.value), int(nl.value), int(nc.value), int(nm.value)), (hs, rl, of, mt, mh)

    def _commit_witness(self, up_keys, up_ids, del_keys, del_ids):
        up_keys, del_keys = list(up_keys), list(del_keys)
        caps, miss_cap = (0, 0), 0
        for _ in range(4):
            rc, (nn, nl, nc, nm), (hs, rl, of, mt, mh) = self.commit_witness_raw(up_keys, up_ids, del_keys, del_ids,
                                                                                caps, miss_cap)
            if rc == _lib.KH_ENOSPC:
                caps = (nn, nl)
                continue
            if rc == _lib.KH_ENODE:
                if nm > miss_cap:
                    miss_cap = nm
                    continue
                e = _lib.MPTNodeMissingException(rc, lib().kh_last_error().decode())
                e.missing = [(int(mt[i]), mh[32 * i:32 * i + 32].tobytes()) for i in range(nm)]
                raise e
            check(rc)
            self.witness_nodes = nn  # (a forest lists a node two tries hold once per trie)
            return {hs[32 * j:32 * j + 32].tobytes(): rl[int(of[j]):int(of[j + 1])].tobytes() for j in range(nn)}, nc
        raise RuntimeError("kh_trie_commit_witness_host: size negotiation failed")

    def nodes_by_hash(self, hashes):
        """getMptNodeByHash over the current version (kh_trie_nodes_by_hash): [encoding or None]
        per 32-byte hash, at most 4096 a call."""
        hashes = list(hashes)
        n = len(hashes)
        hb = np.frombuffer(b"".join(hashes) + b"\0", np.uint8).copy()
        found = np.zeros(max(n, 1), np.uint8)
        off = np.zeros(n + 1, np.uint64)
        need = ctypes.c_uint64(0)
        cap = 0
        self.ctx._sync()
        for _ in range(2):
            rl = np.zeros(max(cap, 1), np.uint8)
            rc = lib().kh_trie_nodes_by_hash(self.h, hb.ctypes.data, n, found.ctypes.data, rl.ctypes.data, cap,
                                             off.ctypes.data, ctypes.byref(need))
            if rc == _lib.KH_ENOSPC:
                cap = need.value
                continue
            check(rc)
            return [rl[off[i]:off[i + 1]].tobytes() if found[i] else None for i in range(n)]
        raise RuntimeError("kh_trie_nodes_by_hash: size negotiation failed")


class _Unknown:
    """get's answer for a key whose walk reaches a stub of a partial handle (KH_FOUND_UNKNOWN):
    neither a value nor None.  Falsy, and equal only to itself."""

    def __bool__(self):
        return False

    def __repr__(self):
        return "UNKNOWN"


UNKNOWN = _Unknown()


class ResidentTrie(_Versioned):
    """A trie kept in HBM between commits (kh_trie_open / kh_trie_apply).

    commit(upserts, deletes) folds a block's dirty set the way TrieAccounts.flush /
    TrieStorage.flush fold their logs into MerklePatriciaTrie.put / remove
    (TrieAccounts.scala:22-28, TrieStorage.scala:43-60), rebuilding only the nodes on the
    changed paths (csrc/forest.h).  Keys are 32-byte trie keys, or raw (address / slot)
    bytes with hash_keys.  With emit=True, nodes() returns the write-back set of the last
    commit (the nodes it created).
    """

    def __init__(self, ctx, keys=(), vals=(), hash_keys=False, emit=True):
        self.ctx = ctx
        self.dev = f"cuda:{ctx.device}"
        self.h = None
        klen = len(keys[0]) if keys else 32
        kd, _ = _pack_dev(list(keys), self.dev)
        vd, vo = _pack_dev(list(vals), self.dev)
        self._open(kd, klen, vd, vo, len(keys), hash_keys, emit)

    def _open(self, kd, klen, vd, vo, n, hash_keys, emit=True):
        self.hash_keys = bool(hash_keys)  # every commit hashes its keys the same way
        h = ctypes.c_void_p()
        root = np.zeros(32, np.uint8)
        flags = (_lib.KH_HASH_KEYS if hash_keys else 0) | (_lib.KH_EMIT_NODES if emit else 0)
        self.ctx._sync()
        check(lib().kh_trie_open(self.ctx.h, _ptr(kd), klen, _ptr(vd), _ptr(vo), n, flags, root.ctypes.data,
                                 ctypes.byref(h)))
        self.h = h
        self.root = root.tobytes()

    @classmethod
    def _from_store(cls, open_fn, ctx, root, nodes, hash_keys, emit):
        """A handle opened by open_fn (kh_trie_open_nodes or kh_trie_open_partial: one signature)
        from a root hash and node encodings ({hash: encoding} or a list)."""
        t = cls.__new__(cls)
        t.ctx, t.dev, t.h = ctx, f"cuda:{ctx.device}", None
        t.hash_keys = bool(hash_keys)
        encs = list(nodes.values()) if isinstance(nodes, dict) else list(nodes)
        ed, eo = _pack_dev(encs, t.dev)
        h = ctypes.c_void_p()
        miss = np.zeros(32, np.uint8)
        flags = (_lib.KH_HASH_KEYS if hash_keys else 0) | (_lib.KH_EMIT_NODES if emit else 0)
        rb = np.frombuffer(bytes(root), np.uint8).copy()
        ctx._sync()
        rc = open_fn(ctx.h, rb.ctypes.data, _ptr(ed), _ptr(eo), len(encs), flags, miss.ctypes.data, ctypes.byref(h))
        if rc == _lib.KH_ENODE:
            e = _lib.MPTNodeMissingException(rc, lib().kh_last_error().decode())
            e.missing = miss.tobytes()
            raise e
        check(rc)
        t.h = h
        t.root = bytes(root)
        return t

    @classmethod
    def from_nodes(cls, ctx, root, nodes, hash_keys=False, emit=True):
        """Open from a root hash and a node store {hash: encoding} (kh_trie_open_nodes;
        MerklePatriciaTrie.apply(rootHash, source)).  A missing node raises
        MPTNodeMissingException with the missing hash in .missing."""
        return cls._from_store(lib().kh_trie_open_nodes, ctx, root, nodes, hash_keys, emit)

    @classmethod
    def from_witness(cls, ctx, root, nodes, hash_keys=False, emit=True):
        """Open from a root hash and the nodes at hand ({hash: encoding} or a list of encodings: a
        block's witness; kh_trie_open_partial).  Subtrees whose node is absent become stubs; only a
        missing root node raises MPTNodeMissingException (its hash in .missing)."""
        return cls._from_store(lib().kh_trie_open_partial, ctx, root, nodes, hash_keys, emit)

    def need(self, keys):
        """[hash or None] per key: the node to fetch before a commit of that key can walk past the
        stub its path reaches (kh_trie_need_host); None where the path is resident."""
        return self._need(keys, None)

    def evict_subtrees(self, prefixes):
        """Turn held subtrees back into stubs (kh_trie_evict_subtrees).  prefixes: nibble sequences,
        each naming the subtree that hangs there.  Returns ([(status, hash or None)], counters):
        status one of KH_EVICT_NONE / DONE / STUB / EMBEDDED, the hash the one to fetch to bring the
        subtree back (DONE, STUB); counters {evicted, keys, records}."""
        return self._evict_subtrees(prefixes, None)

    def fill_range(self, origin, entries, proof=None):
        """Take one range response into this partial trie (kh_trie_fill_ranges_host): entries =
        (keys, vals) in key order, 32-byte TRIE keys (the kec256 values on a hash_keys trie), origin the
        requested origin (None: zero).  proof (the response's boundary-proof nodes: a ProofTable, dict
        or list) is given to fill() first.  The stubs inside [origin, last key] are replaced by the
        subtrees built from the entries, kept only if the root does not move.  Returns (statuses,
        stubs_left, counters): statuses = [KH_RANGE_*], stubs_left = [live stubs afterwards] (0: the
        trie is whole), counters {"keys", "stubs"} gained / replaced; any status but KH_RANGE_OK
        leaves the trie exactly as it was.  The sync loop: range -> fill proof -> fill range ->
        continue from the last key + 1 while stubs_left > 0."""
        return self._fill_ranges([(0, self.root, origin, entries)], proof, False)

    def _flag(self, hash_keys):
        """The trie's key encoder is fixed at open (as the reference's implicit
        ByteArrayEncoder[K] is per trie type): None means that one; a different value raises."""
        if hash_keys is None:
            return self.hash_keys
        if bool(hash_keys) != self.hash_keys:
            raise _lib.MPTException(_lib.KH_EINVAL, f"trie opened with hash_keys={self.hash_keys}, commit asked "
                                                    f"for hash_keys={bool(hash_keys)}")
        return self.hash_keys

    def commit(self, upserts=(), deletes=(), hash_keys=None, stats=None):
        """Apply {key: value} upserts, then deletes; returns the new root."""
        ups = list(upserts.items()) if isinstance(upserts, dict) else list(upserts)
        dels = list(deletes)
        klen = len(ups[0][0]) if ups else (len(dels[0]) if dels else 32)
        uk, _ = _pack_dev([k for k, _ in ups], self.dev)
        uv, uo = _pack_dev([v for _, v in ups], self.dev)
        dk, _ = _pack_dev(dels, self.dev)
        return self.commit_dev(uk, uv, uo, len(ups), dk, len(dels), klen, hash_keys, stats)

    def commit_witness(self, upserts=(), deletes=()):
        """({hash: encoding}, n_collapse): every node a handle opened by from_witness at the current
        root needs to commit(upserts, deletes) at the first attempt -- the paths of the op keys and the
        siblings a collapsing branch is merged with (kh_trie_commit_witness_host).  Takes the batch
        commit takes; the values are ignored and the trie is left unchanged.  On a partial handle
        that lacks some of it: MPTNodeMissingException, .missing the [(0, hash)] to fetch."""
        ups = list(upserts.items()) if isinstance(upserts, dict) else list(upserts)
        return self._commit_witness([k for k, _ in ups], None, list(deletes), None)

    def commit_dev(self, up_keys, up_vals, up_voff, nup, del_keys, ndel, klen=32, hash_keys=None, stats=None):
        root = np.zeros(32, np.uint8)
        st = stats if stats is not None else KhStats()
        flags = _lib.KH_HASH_KEYS if self._flag(hash_keys) else 0
        self.ctx._sync()
        check(lib().kh_trie_apply(self.h, _ptr(up_keys), _ptr(up_vals), _ptr(up_voff), nup, _ptr(del_keys), ndel,
                                  klen, flags, root.ctypes.data, ctypes.byref(st)))
        self.root = root.tobytes()
        return self.root

    def nodes(self):
        """{hash: encoding} written back by the last commit (kh_trie_emit_nodes): the nodes it
        created, every one reachable from the new root with an encoding >= 32 B, plus a changed root."""
        return emitted_nodes(lambda *a: lib().kh_trie_emit_nodes(self.h, *a))

    def checkpoint(self, verify=False):
        """(root, {hash: encoding}): the whole resumable state of the current version (a state
        root plus its node store), what from_nodes opens again.  An empty trie: (EMPTY_TRIE_HASH, {})."""
        return self.get_root(), dict(self.export_nodes(verify=verify))

    def root_of(self, upserts=(), deletes=(), stats=None):
        """TrieAccounts.rootHash (TrieAccounts.scala:73-80): the root commit(upserts, deletes)
        would give; the trie is left unchanged (kh_trie_root_of)."""
        ups = list(upserts.items()) if isinstance(upserts, dict) else list(upserts)
        dels = list(deletes)
        klen = len(ups[0][0]) if ups else (len(dels[0]) if dels else 32)
        uk, _ = _pack_dev([k for k, _ in ups], self.dev)
        uv, uo = _pack_dev([v for _, v in ups], self.dev)
        dk, _ = _pack_dev(dels, self.dev)
        root = np.zeros(32, np.uint8)
        st = stats if stats is not None else KhStats()
        flags = _lib.KH_HASH_KEYS if self.hash_keys else 0
        self.ctx._sync()
        check(lib().kh_trie_root_of(self.h, _ptr(uk), _ptr(uv), _ptr(uo), len(ups), _ptr(dk), len(dels), klen, flags,
                                    root.ctypes.data, ctypes.byref(st)))
        return root.tobytes()

    def copy(self):
        """MerklePatriciaTrie.copy (MerklePatriciaTrie.scala:556): an independent resident trie
        holding the current version (kh_trie_copy)."""
        h = ctypes.c_void_p()
        self.ctx._sync()
        check(lib().kh_trie_copy(self.h, ctypes.byref(h)))
        t = ResidentTrie.__new__(ResidentTrie)
        t.ctx, t.dev, t.h, t.hash_keys, t.root = self.ctx, self.dev, h, self.hash_keys, self.root
        return t

    def _after_rollback(self):
        self.root = self.get_root()

    def get_root(self):
        """The handle's current root (kh_trie_root_of of an empty batch)."""
        root = np.zeros(32, np.uint8)
        check(lib().kh_trie_root_of(self.h, None, None, None, 0, None, 0, 32,
                                    _lib.KH_HASH_KEYS if self.hash_keys else 0, root.ctypes.data, None))
        return root.tobytes()

    def get(self, keys):
        """Batched get (kh_trie_get): [value or None] per key (raw keys with hash_keys)."""
        return trie_get(self.h, keys)

    def prove(self, keys, shared=False):
        """Merkle proofs (kh_trie_prove): (found, proofs), proofs[i] the node encodings on key i's
        path, root first; with shared=True also the ProofTable whose nodes each appear once."""
        self.ctx._sync()
        return _prove(self.h, keys, None, shared)

    def range(self, origin=None, limit=None, max_entries=1024, val_cap=1 << 20):
        """One page of the trie in key order (kh_trie_range_host; trie_range): (keys, vals, more, next)."""
        self.ctx._sync()
        return trie_range(self.h, origin, limit, max_entries, val_cap)

    def items(self, origin=None, limit=None, chunk=1024):
        """Generator over every (key, value) of [origin, limit] in key order, `chunk` entries a call."""
        self.ctx._sync()
        return _range_items(self.h, origin, limit, chunk, None)

    def range_proof(self, origin=None, limit=None, max_entries=1024, val_cap=1 << 20):
        """A page with its two boundary proofs: (keys, vals, more, next, ProofTable of [origin, the
        last returned key or limit]) -- the GetAccountRange shape."""
        self.ctx._sync()
        return _range_proof(self.h, origin, limit, max_entries, val_cap, None)

    def ranges(self, requests, max_entries=1024, val_cap=1 << 20):
        """Many ranges of the trie in one call (kh_trie_ranges_host; trie_ranges): requests =
        [(origin or None, limit or None)] -> (pages, n_done, next), pages[q] = (keys, vals)."""
        self.ctx._sync()
        return trie_ranges(self.h, requests, max_entries, val_cap)

    def ranges_proof(self, requests, max_entries=1024, val_cap=1 << 20):
        """ranges() plus ONE shared ProofTable for every request that needs a boundary proof, and the
        proved flags: (pages, n_done, next, table, proved), as verify_ranges takes them."""
        self.ctx._sync()
        return _ranges_proof(self.h, requests, max_entries, val_cap, False)

    def diff(self, other, origin=None, limit=None, max_entries=1024, val_cap=1 << 20, other_trie=None):
        """One page of what differs between this trie (side a) and `other` (side b: a ResidentTrie, or
        trie other_trie of a ResidentForest), in key order (kh_trie_diff_host; trie_diff): (entries,
        more, next), entries = [(key, kind, value)]."""
        self.ctx._sync()
        other.ctx._sync()
        return trie_diff(self.h, None, other.h, other_trie, origin, limit, max_entries, val_cap)

    def changes(self, other, chunk=1024, other_trie=None):
        """diff() paged to the end: (upserts, deletes) with trie keys -- committed on a copy of this
        trie they give other's root (on a handle that hashes its keys they are the kec256 values, for
        a replica that stores trie keys)."""
        self.ctx._sync()
        other.ctx._sync()
        return _diff_changes(self.h, None, other.h, other_trie, chunk)

    def diffs(self, requests, other, max_entries=1024, val_cap=1 << 20, other_trie=None):
        """Many ranges of the one pair (this trie, `other`) in one call (kh_trie_diffs_host;
        trie_diffs): requests = [(origin or None, limit or None)] -> (pages, n_done, next), pages[q] =
        [(key, kind, value)].  other: a ResidentTrie, or trie other_trie of a ResidentForest."""
        self.ctx._sync()
        other.ctx._sync()
        b_forest = isinstance(other, ResidentForest)
        return trie_diffs(self.h, False, other.h, b_forest,
                          [(other_trie if b_forest else None, None, o, l) for o, l in requests], max_entries, val_cap)

    @property
    def root_hash(self):
        return self.root

    def __len__(self):
        n = ctypes.c_uint64()
        check(lib().kh_trie_size(self.h, ctypes.byref(n)))
        return int(n.value)

    def close(self):
        if self.h:
            lib().kh_trie_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def trie_get(h, keys, trie_ids=None):
    """Batched get through kh_trie_get_host: [value bytes or None] per key
    (MerklePatriciaTrie.get, MerklePatriciaTrie.scala:90-147)."""
    keys = list(keys)
    n = len(keys)
    klen = len(keys[0]) if keys else 32
    kb = np.frombuffer(b"".join(keys) + b"\0", np.uint8).copy()
    tb = np.asarray(trie_ids, np.uint32) if trie_ids is not None else None
    found = np.zeros(max(n, 1), np.uint8)
    voff = np.zeros(n + 1, np.uint64)
    need = ctypes.c_uint64(0)
    cap = 0
    for _ in range(2):
        vals = np.zeros(max(cap, 1), np.uint8)
        rc = lib().kh_trie_get_host(h, tb.ctypes.data if tb is not None else None, kb.ctypes.data, klen, n,
                                    vals.ctypes.data, cap, voff.ctypes.data, found.ctypes.data, ctypes.byref(need))
        if rc == _lib.KH_ENOSPC:
            cap = need.value
            continue
        check(rc)
        return [UNKNOWN if found[i] == _lib.KH_FOUND_UNKNOWN else vals[voff[i]:voff[i + 1]].tobytes() if found[i]
                else None for i in range(n)]
    raise RuntimeError("kh_trie_get: size negotiation failed")


def trie_range(h, origin=None, limit=None, max_entries=1024, val_cap=1 << 20, trie=None):
    """One page of a range scan (kh_trie_range_host): (keys, vals, more, next) -- the first entries
    of [origin, limit] in key order, at most max_entries with values fitting val_cap; next is the
    first key not returned when more.  Keys are trie keys (the kec256 values on a hash_keys handle).
    KH_ENOSPC (not even the first value fits) raises KhError with the size needed in .val_bytes;
    KH_ENODE (a partial handle: the page meets a missing subtree) raises MPTNodeMissingException
    with the hash to fetch in .missing."""
    ob, lb = _packed_keys32([origin], [limit])
    o = _PageOut(max_entries, val_cap)
    o.raise_for(lib().kh_trie_range_host(h, 0 if trie is None else trie, _at(ob), _at(lb), o.n, _at(o.keys),
                                         _at(o.vals), o.val_cap, _at(o.voff), ctypes.byref(o.ne),
                                         ctypes.byref(o.vb), ctypes.byref(o.more), _at(o.nxt), _at(o.miss)))
    k = int(o.ne.value)
    return ([o.keys[32 * i:32 * i + 32].tobytes() for i in range(k)],
            [o.vals[int(o.voff[i]):int(o.voff[i + 1])].tobytes() for i in range(k)], bool(o.more.value),
            o.nxt.tobytes() if o.more.value else None)


def _at(x):
    return x.ctypes.data if x is not None else None


def _packed_keys32(origins, limits):
    """The origins and the limits of the requests of a range or diff call, each packed into one
    array of 32 bytes a request (None: the lowest / the highest key); None for a side no request gives."""
    if any(x is not None and len(x) != 32 for x in (*origins, *limits)):
        raise _lib.MPTException(_lib.KH_EINVAL, "origin and limit are 32-byte keys")

    def pack(keys, absent):
        if all(x is None for x in keys):
            return None
        return np.frombuffer(b"".join(bytes(x) if x is not None else absent for x in keys), np.uint8).copy()
    return pack(origins, b"\0" * 32), pack(limits, b"\xff" * 32)


class _PageOut:
    """The outputs of one range or diff call (kinds: a diff; nq: the requests of a batched call, with
    eoff and n_done, else more), and what its return code raises."""

    def __init__(self, max_entries, val_cap, kinds=False, nq=None):
        self.n, self.val_cap = int(max_entries), int(val_cap)
        room = self.n if 0 < self.n < (1 << 31) else 1  # (else the call refuses with KH_EINVAL before it writes)
        self.keys = np.zeros(32 * room, np.uint8)
        self.kinds = np.zeros(room, np.uint8) if kinds else None
        self.vals = np.zeros(max(self.val_cap, 1), np.uint8)
        self.voff = np.zeros(room + 1, np.uint64)
        self.eoff = np.zeros(nq + 1, np.uint64) if nq is not None else None
        self.ne, self.vb = ctypes.c_uint64(0), ctypes.c_uint64(0)
        self.more, self.nd = ctypes.c_int(0), ctypes.c_uint64(0)
        self.nxt = np.zeros(32, np.uint8)
        self.miss = np.zeros(32, np.uint8)

    def raise_for(self, rc):
        if rc == _lib.KH_ENODE:
            e = _lib.MPTNodeMissingException(rc, lib().kh_last_error().decode())
            e.missing = self.miss.tobytes()
            if self.eoff is not None:
                e.request = int(self.nd.value)
            raise e
        if rc == _lib.KH_ENOSPC:
            e = _lib.KhError(rc, lib().kh_last_error().decode())
            e.val_bytes = int(self.vb.value)
            raise e
        check(rc)

    def pages(self, entry):
        """(pages, n_done, next) of a batched call: pages[q] = [entry(key, i, value)] over request q's
        returned things i."""
        nq = len(self.eoff) - 1
        assert int(self.eoff[nq]) == int(self.ne.value)
        kb, vbuf = self.keys[:32 * int(self.ne.value)].tobytes(), self.vals[:int(self.vb.value)].tobytes()
        pages = [[entry(kb[32 * i:32 * i + 32], i, vbuf[int(self.voff[i]):int(self.voff[i + 1])])
                  for i in range(int(self.eoff[q]), int(self.eoff[q + 1]))] for q in range(nq)]
        done = int(self.nd.value)
        return pages, done, self.nxt.tobytes() if done < nq else None


def _grow_val_cap(call, val_cap):
    """call(val_cap), again with val_cap grown while it raises KH_ENOSPC -> (its result, val_cap)"""
    while True:
        try:
            return call(val_cap), val_cap
        except _lib.KhError as e:
            if e.code != _lib.KH_ENOSPC:
                raise
            val_cap = max(2 * val_cap, e.val_bytes)


def _range_items(h, origin, limit, chunk, trie, val_cap=1 << 20):
    """Every (key, value) of [origin, limit] in key order, paged by next; val_cap grows on KH_ENOSPC."""
    while True:
        (keys, vals, more, nxt), val_cap = _grow_val_cap(
            lambda cap: trie_range(h, origin, limit, chunk, cap, trie), val_cap)
        yield from zip(keys, vals)
        if not more:
            return
        origin = nxt


def trie_diff(ha, trie_a, hb, trie_b, origin=None, limit=None, max_entries=1024, val_cap=1 << 20):
    """One page of the differences between two resident tries (kh_trie_diff_host): (entries, more,
    next), entries = [(key, kind, value)] in key order -- kind KH_DIFF_ONLY_A (value b""),
    KH_DIFF_ONLY_B or KH_DIFF_CHANGED with side b's value; next is the first differing key not
    returned when more.  Keys are trie keys.  KH_ENOSPC raises KhError with .val_bytes, KH_ENODE
    (partial handles) MPTNodeMissingException with the hash to fetch in .missing."""
    ob, lb = _packed_keys32([origin], [limit])
    o = _PageOut(max_entries, val_cap, kinds=True)
    o.raise_for(lib().kh_trie_diff_host(ha, 0 if trie_a is None else trie_a, hb, 0 if trie_b is None else trie_b,
                                        _at(ob), _at(lb), o.n, o.val_cap, _at(o.keys), _at(o.kinds), _at(o.vals),
                                        _at(o.voff), ctypes.byref(o.ne), ctypes.byref(o.vb), ctypes.byref(o.more),
                                        _at(o.nxt), _at(o.miss)))
    k = int(o.ne.value)
    return ([(o.keys[32 * i:32 * i + 32].tobytes(), int(o.kinds[i]),
              o.vals[int(o.voff[i]):int(o.voff[i + 1])].tobytes()) for i in range(k)], bool(o.more.value),
            o.nxt.tobytes() if o.more.value else None)


def trie_changes_since(h, forest, level=0, reverse=False, start=None, max_entries=1024, val_cap=1 << 20):
    """One page of kh_trie_changes_since_host (_Versioned.changes_since): (entries, more, next, n_total)."""
    ft, fk = (start if forest else (0, start)) if start is not None else (0, None)
    if fk is not None and len(fk) != 32:
        raise _lib.MPTException(_lib.KH_EINVAL, "start is a 32-byte key")
    fb = np.frombuffer(bytes(fk), np.uint8).copy() if fk is not None else None
    o = _PageOut(max_entries, val_cap, kinds=True)
    tries = np.zeros(len(o.kinds), np.uint32)
    total, nt = ctypes.c_uint64(0), ctypes.c_uint32(0)
    rc = lib().kh_trie_changes_since_host(h, level, _lib.KH_CHANGES_REVERSE if reverse else 0, ft, _at(fb), o.n,
                                          o.val_cap, _at(tries), _at(o.keys), _at(o.kinds), _at(o.vals), _at(o.voff),
                                          ctypes.byref(o.ne), ctypes.byref(o.vb), ctypes.byref(total),
                                          ctypes.byref(o.more), ctypes.byref(nt), _at(o.nxt))
    try:
        o.raise_for(rc)
    except _lib.KhError as e:
        if e.code == _lib.KH_ENOSPC:
            e.n_total = int(total.value)
        raise
    k = int(o.ne.value)
    ents = [(o.keys[32 * i:32 * i + 32].tobytes(), int(o.kinds[i]), o.vals[int(o.voff[i]):int(o.voff[i + 1])].tobytes())
            for i in range(k)]
    nxt = o.nxt.tobytes() if o.more.value else None
    if forest:
        ents = [(int(tries[i]),) + e for i, e in enumerate(ents)]
        nxt = (int(nt.value), nxt) if o.more.value else None
    return ents, bool(o.more.value), nxt, int(total.value)


def changes_counters():
    """The radix sorts of the last changes-since call (2 or more words: it fell back to the full-key
    order): measurements and tests only."""
    return int(lib().khst_changes_sorts())


def _add_changes(ents, ups, dels):
    """the differences [(key, kind, value)] as upserts and deletes of the commit that brings a to b"""
    for k, kind, v in ents:
        if kind == _lib.KH_DIFF_ONLY_A:
            dels.append(k)
        else:
            ups.append((k, v))


def _diff_changes(ha, trie_a, hb, trie_b, chunk, val_cap=1 << 20):
    """Every difference, paged by next (val_cap grows on KH_ENOSPC), as the (upserts, deletes) of the
    commit that brings side a to side b."""
    ups, dels, origin = [], [], None
    while True:
        (ents, more, nxt), val_cap = _grow_val_cap(
            lambda cap: trie_diff(ha, trie_a, hb, trie_b, origin, None, chunk, cap), val_cap)
        _add_changes(ents, ups, dels)
        if not more:
            return ups, dels
        origin = nxt


def diff_counters():
    """(rounds past the root pair, frontier items selected) of the last diff: measurements only."""
    return int(lib().khst_diff_rounds()), int(lib().khst_diff_visited())


def trie_diffs(ha, a_forest, hb, b_forest, requests, max_entries=1024, val_cap=1 << 20):
    """Many trie pairs in one call (kh_trie_diffs_host).  requests: [(trie_a, trie_b, origin, limit)]
    -- trie_a / trie_b the ids on a forest side (ignored on a single trie; trie_b None: trie_a),
    origin / limit None: the lowest / the highest key.
    -> (pages, n_done, next): pages[q] = [(key, kind, value)] of request q, the requests answered in
    order under max_entries differences and val_cap side-b value bytes IN TOTAL; n_done leading
    requests are answered completely; when n_done < len(requests), request n_done is the cut one,
    next its first differing key not returned (else None), and the requests after it are unanswered
    (empty pages).  Keys are trie keys.  KH_ENOSPC raises KhError with .val_bytes; KH_ENODE raises
    MPTNodeMissingException with the hash to fetch in .missing and the request in .request."""
    reqs = [tuple(q) for q in requests]
    nq = len(reqs)
    ta = tb = None
    if a_forest or b_forest:
        ta = np.asarray([t or 0 for t, _, _, _ in reqs] + [0], np.uint32)
    if b_forest and any(u is not None for _, u, _, _ in reqs):
        tb = np.asarray([(t or 0) if u is None else u for t, u, _, _ in reqs] + [0], np.uint32)
    ob, lb = _packed_keys32([o for _, _, o, _ in reqs], [l for _, _, _, l in reqs])
    o = _PageOut(max_entries, val_cap, kinds=True, nq=nq)
    o.raise_for(lib().kh_trie_diffs_host(ha, _at(ta), hb, _at(tb), _at(ob), _at(lb), nq, o.n, o.val_cap,
                                         _at(o.keys), _at(o.kinds), _at(o.vals), _at(o.voff), _at(o.eoff),
                                         ctypes.byref(o.ne), ctypes.byref(o.vb), ctypes.byref(o.nd), _at(o.nxt),
                                         _at(o.miss)))
    return o.pages(lambda key, i, value: (key, int(o.kinds[i]), value))


def _diffs_changes(ha, a_forest, hb, b_forest, pairs, chunk, val_cap=1 << 20):
    """Every difference of every pair [(trie_a, trie_b)], kh_trie_diffs_host paged to the end by
    n_done / next (val_cap grows on KH_ENOSPC): [(upserts, deletes)] per pair."""
    out = [([], []) for _ in pairs]
    reqs = [(t, u, None, None) for t, u in pairs]
    first = 0  # the pair reqs[0] belongs to
    while reqs:
        (pages, done, nxt), val_cap = _grow_val_cap(
            lambda cap: trie_diffs(ha, a_forest, hb, b_forest, reqs, chunk, cap), val_cap)
        for q, page in enumerate(pages[:done + 1]):
            _add_changes(page, *out[first + q])
        if done == len(reqs):
            break
        reqs = [(reqs[done][0], reqs[done][1], nxt, None)] + reqs[done + 1:]
        first += done
    return out


def diffs_counters():
    """(rounds past the root pairs, frontier items selected) of the last batched diff: measurements only."""
    return int(lib().khst_diffs_rounds()), int(lib().khst_diffs_visited())


def _range_proof(h, origin, limit, max_entries, val_cap, trie):
    """A page and the two boundary proofs a range response carries: (keys, vals, more, next, table),
    table the shared ProofTable of [origin, the last returned key or limit] (trie keys)."""
    keys, vals, more, nxt = trie_range(h, origin, limit, max_entries, val_cap, trie)
    ends = [origin if origin is not None else b"\0" * 32,
            keys[-1] if keys else (limit if limit is not None else b"\xff" * 32)]
    _, table = trie_prove(h, ends, None if trie is None else [trie, trie], shared=True, trie_keys=True)
    return keys, vals, more, nxt, table


def trie_ranges(h, requests, max_entries=1024, val_cap=1 << 20, forest=False):
    """Many ranges in one call (kh_trie_ranges_host).  requests: [(trie_id, origin, limit)] on a
    forest, [(origin, limit)] on a single trie (origin / limit None: the lowest / the highest key).
    -> (pages, n_done, next): pages[q] = (keys, vals) of request q, the requests answered in order
    under max_entries entries and val_cap value bytes IN TOTAL; n_done leading requests are answered
    completely; when n_done < len(requests), request n_done is the cut one, next its first key not
    returned (else None), and the requests after it are unanswered (empty pages).  Keys are trie
    keys.  KH_ENOSPC raises KhError with .val_bytes; KH_ENODE raises MPTNodeMissingException with
    the hash to fetch in .missing and the request it belongs to in .request."""
    reqs = [tuple(q) for q in requests]
    if not forest:
        reqs = [(0, o, l) for o, l in reqs]
    nq = len(reqs)
    tb = np.asarray([t for t, _, _ in reqs] + [0], np.uint32) if forest else None
    ob, lb = _packed_keys32([o for _, o, _ in reqs], [l for _, _, l in reqs])
    o = _PageOut(max_entries, val_cap, nq=nq)
    o.raise_for(lib().kh_trie_ranges_host(h, _at(tb), _at(ob), _at(lb), nq, o.n, _at(o.keys), _at(o.vals),
                                          o.val_cap, _at(o.voff), _at(o.eoff), ctypes.byref(o.ne),
                                          ctypes.byref(o.vb), ctypes.byref(o.nd), _at(o.nxt), _at(o.miss)))
    pages, done, nxt = o.pages(lambda key, i, value: (key, value))
    return [([k for k, _ in p], [v for _, v in p]) for p in pages], done, nxt


def _ranges_proof(h, requests, max_entries, val_cap, forest):
    """trie_ranges and the boundary proofs its response carries, in ONE shared table of one
    kh_trie_prove(KH_PROVE_TRIE_KEYS | KH_PROVE_SHARED) call: proved[q] = 1 for the cut request and
    for every answered request whose origin is not zero or whose limit is not all-0xFF, each proved
    over [origin, its last returned key, or its limit when it returned none].
    -> (pages, n_done, next, table, proved)"""
    reqs = [tuple(q) for q in requests]
    pages, done, nxt = trie_ranges(h, reqs, max_entries, val_cap, forest)
    if not forest:
        reqs = [(0, o, l) for o, l in reqs]
    zero, ff = b"\0" * 32, b"\xff" * 32
    proved, ends, ids = [], [], []
    for q, (t, o, l) in enumerate(reqs):
        o, l = o if o is not None else zero, l if l is not None else ff
        p = q == done or (q < done and (o != zero or l != ff))
        proved.append(int(p))
        if p:
            ends += [o, pages[q][0][-1] if pages[q][0] else l]
            ids += [t, t]
    if ends:
        _, table = trie_prove(h, ends, ids if forest else None, shared=True, trie_keys=True)
    else:
        table = ProofTable([], [], [], [0])
    return pages, done, nxt, table, proved


class ProofTable:
    """The node table of a kh_trie_prove call and the paths into it: nodes[j] has hash hashes[j];
    the proof of key i is nodes[path_idx[k]] for k in [path_off[i], path_off[i + 1])."""

    def __init__(self, hashes, nodes, path_idx, path_off):
        self.hashes, self.nodes = hashes, nodes
        self.path_idx = np.asarray(path_idx, np.uint32)
        self.path_off = np.asarray(path_off, np.uint64)

    def proof(self, i):
        return [self.nodes[j] for j in self.path_idx[int(self.path_off[i]):int(self.path_off[i + 1])]]

    def proofs(self):
        return [self.proof(i) for i in range(len(self.path_off) - 1)]


def trie_prove_raw(h, keys, trie_ids=None, shared=False, caps=None, trie_keys=False):
    """One kh_trie_prove call with the capacities caps = (nodes, encoding bytes, path entries):
    (rc, (n_nodes, rlp_len, n_path), arrays), arrays = (found, hashes, rlp, off, path_idx, path_off).
    trie_keys: KH_PROVE_TRIE_KEYS (the keys are trie keys, as a range scan returns them)."""
    keys = list(keys)
    n = len(keys)
    klen = len(keys[0]) if keys else 32
    kb = np.frombuffer(b"".join(keys) + b"\0", np.uint8).copy()
    tb = np.asarray(trie_ids, np.uint32) if trie_ids is not None else None
    cn, cb, cp = caps or (0, 0, 0)
    found = np.zeros(max(n, 1), np.uint8)
    hs = np.zeros(32 * max(cn, 1), np.uint8)
    rl = np.zeros(max(cb, 1), np.uint8)
    of = np.zeros(cn + 1, np.uint64)
    pi = np.zeros(max(cp, 1), np.uint32)
    po = np.zeros(n + 1, np.uint64)
    nn, nl, npth = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    rc = lib().kh_trie_prove(h, tb.ctypes.data if tb is not None else None, kb.ctypes.data, klen, n,
                             (_lib.KH_PROVE_SHARED if shared else 0) | (_lib.KH_PROVE_TRIE_KEYS if trie_keys else 0),
                             found.ctypes.data, hs.ctypes.data, cn,
                             rl.ctypes.data, cb, of.ctypes.data, pi.ctypes.data, cp, po.ctypes.data,
                             ctypes.byref(nn), ctypes.byref(nl), ctypes.byref(npth))
    return rc, (int(nn.value), int(nl.value), int(npth.value)), (found, hs, rl, of, pi, po)


def trie_prove(h, keys, trie_ids=None, shared=False, trie_keys=False):
    """Merkle proofs through kh_trie_prove (sizes negotiated): (found, ProofTable)."""
    keys = list(keys)
    caps = None
    for _ in range(3):
        rc, sizes, (found, hs, rl, of, pi, po) = trie_prove_raw(h, keys, trie_ids, shared, caps, trie_keys)
        if rc == _lib.KH_ENOSPC:
            caps = sizes
            continue
        check(rc)
        nn, _, npth = sizes
        table = ProofTable([hs[32 * j:32 * j + 32].tobytes() for j in range(nn)],
                           [rl[int(of[j]):int(of[j + 1])].tobytes() for j in range(nn)], pi[:npth].copy(), po)
        # (2, KH_FOUND_UNKNOWN: the walk reaches a stub of a partial handle)
        return [2 if f == _lib.KH_FOUND_UNKNOWN else bool(f) for f in found[:len(keys)]], table
    raise RuntimeError("kh_trie_prove: size negotiation failed")


def _prove(h, keys, trie_ids, shared):
    found, table = trie_prove(h, keys, trie_ids, shared)
    return (found, table.proofs(), table) if shared else (found, table.proofs())


def verify_proofs(roots, keys, proofs_or_table, hash_keys=False):
    """kh_verify_proofs: (status, values) per key, values[i] the bytes where status[i] is
    KH_PROOF_VALUE, else None.  roots: one 32-byte root for every key, or a list of one per key;
    proofs_or_table: a list of proofs (each a list of node encodings, root first) or the
    ProofTable a shared prove returned."""
    keys = list(keys)
    n = len(keys)
    if isinstance(roots, (bytes, bytearray)):
        roots = [bytes(roots)]
    roots = list(roots)
    if isinstance(proofs_or_table, ProofTable):
        nodes, pi, po = proofs_or_table.nodes, proofs_or_table.path_idx, proofs_or_table.path_off
    else:
        nodes = [e for p in proofs_or_table for e in p]
        pi = np.arange(len(nodes), dtype=np.uint32)
        po = np.zeros(n + 1, np.uint64)
        np.cumsum([len(p) for p in proofs_or_table], out=po[1:])
    klen = len(keys[0]) if keys else 32
    kb = np.frombuffer(b"".join(keys) + b"\0", np.uint8).copy()
    rb = np.frombuffer(b"".join(roots) + b"\0", np.uint8).copy()
    rl = np.frombuffer(b"".join(nodes) + b"\0", np.uint8).copy()
    of = np.zeros(len(nodes) + 1, np.uint64)
    np.cumsum([len(e) for e in nodes], out=of[1:])
    pi = np.ascontiguousarray(np.append(pi, np.uint32(0)), np.uint32)
    po = np.ascontiguousarray(po, np.uint64)
    status = np.zeros(max(n, 1), np.uint8)
    voff = np.zeros(n + 1, np.uint64)
    need = ctypes.c_uint64(0)
    cap = 0
    for _ in range(2):
        vals = np.zeros(max(cap, 1), np.uint8)
        rc = lib().kh_verify_proofs(rb.ctypes.data, len(roots), kb.ctypes.data, klen, n,
                                    _lib.KH_HASH_KEYS if hash_keys else 0, rl.ctypes.data, of.ctypes.data, len(nodes),
                                    pi.ctypes.data, po.ctypes.data, status.ctypes.data, vals.ctypes.data, cap,
                                    voff.ctypes.data, ctypes.byref(need))
        if rc == _lib.KH_ENOSPC:
            cap = need.value
            continue
        check(rc)
        st = [int(s) for s in status[:n]]
        return st, [vals[int(voff[i]):int(voff[i + 1])].tobytes() if st[i] == _lib.KH_PROOF_VALUE else None
                    for i in range(n)]
    raise RuntimeError("kh_verify_proofs: size negotiation failed")


def _range_arrays(roots, origins, responses, nodes, proved):
    """The packed arrays of a kh_verify_ranges call (numpy, kept alive by the caller)."""
    roots, responses = list(roots), [(list(k), list(v)) for k, v in responses]
    nr = len(roots)
    if origins is not None:
        origins = [o if o is not None else b"\0" * 32 for o in origins]
    if isinstance(nodes, ProofTable):
        nodes = nodes.nodes
    elif isinstance(nodes, dict):
        nodes = list(nodes.values())
    nodes = list(nodes) if nodes is not None else []
    if proved is None:
        proved = [1] * nr
    if len(responses) != nr or len(proved) != nr or (origins is not None and len(origins) != nr):
        raise _lib.MPTException(_lib.KH_EINVAL, "one origin, response and proved flag per root")
    keys = [k for ks, _ in responses for k in ks]
    vals = [v for _, vs in responses for v in vs]
    if any(len(ks) != len(vs) for ks, vs in responses) or any(len(k) != 32 for k in keys) or \
            any(len(r) != 32 for r in roots) or (origins is not None and any(len(o) != 32 for o in origins)):
        raise _lib.MPTException(_lib.KH_EINVAL, "keys, roots and origins are 32 bytes; one value per key")
    a = {
        "roots": np.frombuffer(b"".join(roots) + b"\0", np.uint8).copy(),
        "origins": np.frombuffer(b"".join(origins) + b"\0", np.uint8).copy() if origins is not None else None,
        "proved": np.asarray(list(proved) + [0], np.uint8),
        "keys": np.frombuffer(b"".join(keys) + b"\0", np.uint8).copy(),
        "vals": np.frombuffer(b"".join(vals) + b"\0", np.uint8).copy(),
        "voff": np.zeros(len(keys) + 1, np.uint64),
        "ent_off": np.zeros(nr + 1, np.uint64),
        "enc": np.frombuffer(b"".join(nodes) + b"\0", np.uint8).copy(),
        "off": np.zeros(len(nodes) + 1, np.uint64),
    }
    np.cumsum([len(v) for v in vals], out=a["voff"][1:])
    np.cumsum([len(ks) for ks, _ in responses], out=a["ent_off"][1:])
    np.cumsum([len(e) for e in nodes], out=a["off"][1:])
    return nr, len(nodes), a


def verify_ranges(roots, origins, responses, nodes, proved=None):
    """kh_verify_ranges: range responses checked against their roots without a handle, many in one
    call over ONE node set.  roots[s]: the 32-byte root; origins[s]: the 32-byte origin (origins
    None, or an entry None: zero); responses[s] = (keys, vals), the entries in key order (32-byte
    trie keys); nodes: a list or dict of node encodings, or the ProofTable range_proof returns;
    proved[s] (default all 1): 0 claims the entries are the whole trie and reads no node.  Returns
    [(status, more, missing or None)] per range: status a KH_RANGE_* code, more whether the trie
    holds a key above the last entry, missing the absent hash when status is KH_RANGE_MISSING."""
    nr, nn, a = _range_arrays(roots, origins, responses, nodes, proved)
    status, more, miss = np.zeros(nr + 1, np.uint8), np.zeros(nr + 1, np.uint8), np.zeros(32 * nr + 1, np.uint8)
    check(lib().kh_verify_ranges(a["roots"].ctypes.data, a["origins"].ctypes.data if a["origins"] is not None else None,
                                 a["proved"].ctypes.data, nr, a["keys"].ctypes.data, a["vals"].ctypes.data,
                                 a["voff"].ctypes.data, a["ent_off"].ctypes.data, a["enc"].ctypes.data,
                                 a["off"].ctypes.data, nn, status.ctypes.data, more.ctypes.data, miss.ctypes.data))
    return [(int(status[s]), bool(more[s]),
             miss[32 * s:32 * s + 32].tobytes() if status[s] == _lib.KH_RANGE_MISSING else None) for s in range(nr)]


def verify_range(root, origin, keys, vals, nodes):
    """One range through verify_ranges: (status, more, missing or None).  nodes None: the entries
    claim to be the whole trie (proved = 0)."""
    return verify_ranges([root], [origin], [(keys, vals)], nodes if nodes is not None else [],
                         [0 if nodes is None else 1])[0]


def emitted_nodes(call):
    """Size negotiation of kh_trie_emit_nodes (KH_ENOSPC reports the sizes; no re-encoding).
    Another thread's commit on the handle may replace the set between the size query and the
    read (the reader then sees KH_ENOSPC with the new sizes): the query is repeated."""
    nn, nl = ctypes.c_uint64(0), ctypes.c_uint64(0)
    cap_n, cap_b = 0, 0
    for _ in range(16):
        hs = np.zeros(32 * max(cap_n, 1), np.uint8)
        rl = np.zeros(max(cap_b, 1), np.uint8)
        of = np.zeros(cap_n + 1, np.uint64)
        rc = call(hs.ctypes.data, cap_n, rl.ctypes.data, cap_b, of.ctypes.data, ctypes.byref(nn), ctypes.byref(nl))
        if rc == _lib.KH_ENOSPC:
            cap_n, cap_b = nn.value, nl.value
            continue
        check(rc)
        return {hs[32 * i:32 * i + 32].tobytes(): rl[of[i]:of[i + 1]].tobytes() for i in range(nn.value)}
    raise RuntimeError("kh_trie_emit_nodes: size negotiation failed")


class ResidentForest(_Versioned):
    """Many tries in one handle (contract storage tries; kh_forest_open / kh_forest_apply,
    SURVEY §8 a12): each op names its trie id; one commit re-roots every touched trie."""

    def __init__(self, ctx, hash_keys=False, emit=False):
        self.ctx = ctx
        self.dev = f"cuda:{ctx.device}"
        self.hash_keys = bool(hash_keys)
        h = ctypes.c_void_p()
        flags = (_lib.KH_HASH_KEYS if hash_keys else 0) | (_lib.KH_EMIT_NODES if emit else 0)
        check(lib().kh_forest_open(ctx.h, flags, ctypes.byref(h)))
        self.h = h

    def commit(self, upserts=(), deletes=(), stats=None):
        """upserts: [(trie_id, key, value)], deletes: [(trie_id, key)] -> {trie_id: new root}."""
        import torch
        ups, dels = list(upserts), list(deletes)
        klen = len(ups[0][1]) if ups else (len(dels[0][1]) if dels else 32)
        uk, _ = _pack_dev([k for _, k, _ in ups], self.dev)
        uv, uo = _pack_dev([v for _, _, v in ups], self.dev)
        dk, _ = _pack_dev([k for _, k in dels], self.dev)
        ut = torch.tensor([t for t, _, _ in ups] + [0], dtype=torch.int64).to(torch.int32).to(self.dev)
        dt = torch.tensor([t for t, _ in dels] + [0], dtype=torch.int64).to(torch.int32).to(self.dev)
        cap = len(ups) + len(dels) + 1
        tries = np.zeros(cap, np.uint32)
        roots = np.zeros(32 * cap, np.uint8)
        nt = ctypes.c_uint64()
        st = stats if stats is not None else KhStats()
        self.ctx._sync()
        check(lib().kh_forest_apply(self.h, _ptr(ut), _ptr(uk), _ptr(uv), _ptr(uo), len(ups), _ptr(dt), _ptr(dk),
                                    len(dels), klen, tries.ctypes.data, roots.ctypes.data, cap, ctypes.byref(nt),
                                    ctypes.byref(st)))
        return {int(tries[i]): roots[32 * i:32 * i + 32].tobytes() for i in range(nt.value)}

    def commit_witness(self, upserts=(), deletes=()):
        """As ResidentTrie.commit_witness for commit's [(trie_id, key, value)] upserts and
        [(trie_id, key)] deletes: ({hash: encoding}, n_collapse), what load_partial needs at the
        current roots; .missing of the exception is [(trie_id, hash)]."""
        ups, dels = list(upserts), list(deletes)
        return self._commit_witness([k for _, k, _ in ups], [t for t, _, _ in ups], [k for _, k in dels],
                                    [t for t, _ in dels])

    @classmethod
    def from_nodes(cls, ctx, roots, nodes, hash_keys=False, emit=False):
        """A forest resumed from {trie_id: root} and a node store {hash: encoding} (what
        checkpoint() returns): kh_forest_open then load_nodes."""
        f = cls(ctx, hash_keys=hash_keys, emit=emit)
        f.load_nodes(roots, nodes)
        return f

    def load_nodes_raw(self, ids, roots, encs, miss_cap=None, partial=False):
        """One kh_forest_load_nodes (partial: kh_forest_load_partial) call: (rc, n_missing,
        [(list index, hash)] written)."""
        ids, roots, encs = list(ids), list(roots), list(encs)
        k = len(ids)
        tb = np.asarray(ids + [0], np.uint32)
        rb = np.frombuffer(b"".join(bytes(r) for r in roots) + b"\0", np.uint8).copy()
        ed, eo = _pack_dev(encs, self.dev)
        cap = k if miss_cap is None else miss_cap
        mi = np.zeros(max(cap, 1), np.uint32)
        mh = np.zeros(32 * max(cap, 1), np.uint8)
        nm = ctypes.c_uint64(0)
        self.ctx._sync()
        call = lib().kh_forest_load_partial if partial else lib().kh_forest_load_nodes
        rc = call(self.h, tb.ctypes.data, rb.ctypes.data, k, _ptr(ed), _ptr(eo), len(encs), mi.ctypes.data,
                  mh.ctypes.data, cap, ctypes.byref(nm), None)
        w = min(int(nm.value), cap)
        return rc, int(nm.value), [(int(mi[e]), mh[32 * e:32 * e + 32].tobytes()) for e in range(w)]

    def load_partial(self, roots, nodes):
        """Page tries in from the nodes at hand (kh_forest_load_partial): as load_nodes, but a subtree
        whose node is absent becomes a stub; only a missing root node raises."""
        return self.load_nodes(roots, nodes, partial=True)

    def need(self, queries):
        """queries: [(trie_id, key)] -> [hash or None], as ResidentTrie.need."""
        q = list(queries)
        return self._need([k for _, k in q], [t for t, _ in q])

    def evict_subtrees(self, prefixes, tries=True):
        """prefixes: [(trie_id, nibbles)] -> ([(status, hash or None)], counters), as
        ResidentTrie.evict_subtrees.  (tries=None passes no trie array: the library refuses it.)"""
        q = list(prefixes)
        return self._evict_subtrees([p for _, p in q], [t for t, _ in q] if tries is not None else None)

    def fill_ranges(self, ranges, proof=None):
        """Take range responses into the forest, many in one call (kh_trie_fill_ranges_host): ranges =
        [(trie_id, root, origin or None, (keys, vals))], a trie named once.  A trie the forest does
        not hold is taken WHOLE from its entries (they must hash to root); a resident partial trie
        has the stubs inside [origin, last key] replaced, root its current root (every root None: no
        claim, resident tries only).  proof is given to fill() first.  All or nothing over the call;
        returns (statuses, stubs_left, counters) as ResidentTrie.fill_range -- the GetStorageRanges
        shape: many whole small tries and one tail."""
        return self._fill_ranges(ranges, proof, True)

    def load_nodes(self, roots, nodes, partial=False):
        """Page tries in (kh_forest_load_nodes): roots {trie_id: root}, nodes {hash: encoding} or a
        list of encodings.  All or nothing.  Nodes missing from the store raise
        MPTNodeMissingException with .missing = [(trie_id, hash)]: every missing reference of the
        first round of the walk that lacks one."""
        ids = list(roots)
        encs = list(nodes.values()) if isinstance(nodes, dict) else list(nodes)
        cap = max(len(ids), 16)
        for _ in range(2):
            rc, nm, miss = self.load_nodes_raw(ids, [roots[t] for t in ids], encs, cap, partial)
            if rc == _lib.KH_ENODE and nm > cap:
                cap = nm
                continue
            if rc == _lib.KH_ENODE:
                e = _lib.MPTNodeMissingException(rc, lib().kh_last_error().decode())
                e.missing = [(ids[j], h) for j, h in miss]
                raise e
            check(rc)
            return
        raise RuntimeError("kh_forest_load_nodes: size negotiation failed")

    def roots(self):
        """{trie_id: root} of every trie the forest holds (kh_forest_roots)."""
        n = ctypes.c_uint64()
        cap = 0
        for _ in range(3):
            tries = np.zeros(max(cap, 1), np.uint32)
            roots = np.zeros(32 * max(cap, 1), np.uint8)
            self.ctx._sync()
            rc = lib().kh_forest_roots(self.h, tries.ctypes.data, roots.ctypes.data, cap, ctypes.byref(n))
            if rc == _lib.KH_ENOSPC:
                cap = n.value
                continue
            check(rc)
            return {int(tries[i]): roots[32 * i:32 * i + 32].tobytes() for i in range(n.value)}
        raise RuntimeError("kh_forest_roots: size negotiation failed")

    def evict(self, ids):
        """Drop whole tries from HBM (kh_forest_evict); returns the number dropped.  An evicted id
        reads as an empty trie until it is loaded again."""
        ids = list(ids)
        tb = np.asarray(ids + [0], np.uint32)
        n = ctypes.c_uint64()
        self.ctx._sync()
        check(lib().kh_forest_evict(self.h, tb.ctypes.data, len(ids), ctypes.byref(n)))
        return int(n.value)

    def checkpoint(self, verify=False):
        """({trie_id: root}, {hash: encoding}): the resumable state of the current version, what
        from_nodes / load_nodes take."""
        return self.roots(), dict(self.export_nodes(verify=verify))

    def nodes(self):
        return emitted_nodes(lambda *a: lib().kh_trie_emit_nodes(self.h, *a))

    def get(self, queries):
        """queries: [(trie_id, key)] -> [value or None] (kh_trie_get)."""
        q = list(queries)
        return trie_get(self.h, [k for _, k in q], [t for t, _ in q])

    def prove(self, queries, shared=False):
        """queries: [(trie_id, key)] -> (found, proofs[, ProofTable]) as ResidentTrie.prove, each
        proof under its own trie's root."""
        q = list(queries)
        self.ctx._sync()
        return _prove(self.h, [k for _, k in q], [t for t, _ in q], shared)

    def range(self, trie, origin=None, limit=None, max_entries=1024, val_cap=1 << 20):
        """One page of trie `trie` in key order (kh_trie_range_host): (keys, vals, more, next); an id
        the forest does not hold is empty."""
        self.ctx._sync()
        return trie_range(self.h, origin, limit, max_entries, val_cap, trie)

    def items(self, trie, origin=None, limit=None, chunk=1024):
        """Generator over every (key, value) of trie `trie` within [origin, limit], in key order."""
        self.ctx._sync()
        return _range_items(self.h, origin, limit, chunk, trie)

    def range_proof(self, trie, origin=None, limit=None, max_entries=1024, val_cap=1 << 20):
        """ResidentTrie.range_proof for one trie of the forest."""
        self.ctx._sync()
        return _range_proof(self.h, origin, limit, max_entries, val_cap, trie)

    def ranges(self, requests, max_entries=1024, val_cap=1 << 20):
        """Many ranges in one call (kh_trie_ranges_host; trie_ranges): requests = [(trie_id, origin or
        None, limit or None)] -> (pages, n_done, next), pages[q] = (keys, vals)."""
        self.ctx._sync()
        return trie_ranges(self.h, requests, max_entries, val_cap, forest=True)

    def ranges_proof(self, requests, max_entries=1024, val_cap=1 << 20):
        """ranges() plus ONE shared ProofTable for every request that needs a boundary proof, and the
        proved flags: (pages, n_done, next, table, proved), as verify_ranges takes them."""
        self.ctx._sync()
        return _ranges_proof(self.h, requests, max_entries, val_cap, True)

    def diff(self, trie, other, other_trie=None, origin=None, limit=None, max_entries=1024, val_cap=1 << 20):
        """One page of what differs between trie `trie` (side a) and `other` (side b: a ResidentTrie, or
        trie other_trie of a ResidentForest, this one included), in key order (kh_trie_diff_host;
        trie_diff): (entries, more, next), entries = [(key, kind, value)]."""
        self.ctx._sync()
        other.ctx._sync()
        return trie_diff(self.h, trie, other.h, other_trie, origin, limit, max_entries, val_cap)

    def changes(self, trie, other, other_trie=None, chunk=1024):
        """diff() paged to the end: the (upserts, deletes) that bring trie `trie` to side b."""
        self.ctx._sync()
        other.ctx._sync()
        return _diff_changes(self.h, trie, other.h, other_trie, chunk)

    def diffs(self, requests, other=None, max_entries=1024, val_cap=1 << 20):
        """Many trie pairs in one call (kh_trie_diffs_host; trie_diffs): requests = [(trie, other_trie
        or None, origin or None, limit or None)], trie of this forest (side a) against other_trie
        (None: the same id) of `other` (side b: a ResidentForest, None for this one, or a
        ResidentTrie) -> (pages, n_done, next), pages[q] = [(key, kind, value)]."""
        other = self if other is None else other
        self.ctx._sync()
        other.ctx._sync()
        return trie_diffs(self.h, True, other.h, isinstance(other, ResidentForest), requests, max_entries, val_cap)

    def changes_all(self, other, tries=None, chunk=4096):
        """diffs() of trie t of this forest against trie t of `other`, for every t of `tries`, paged
        to the end by n_done / next: {t: (upserts, deletes)} for the ids that differ -- committed on
        this forest they give other's tries.  tries=None: the ids of roots() of both sides, those
        whose roots are equal dropped on the host."""
        if tries is None:
            mine, theirs = self.roots(), other.roots()
            tries = sorted(t for t in set(mine) | set(theirs) if mine.get(t) != theirs.get(t))
        tries = list(tries)
        self.ctx._sync()
        other.ctx._sync()
        got = _diffs_changes(self.h, True, other.h, True, [(t, None) for t in tries], chunk)
        return {t: ud for t, ud in zip(tries, got) if ud[0] or ud[1]}

    def copy(self):
        """An independent resident forest holding the current version of every trie (kh_trie_copy):
        how a parent version of a storage forest is kept."""
        h = ctypes.c_void_p()
        self.ctx._sync()
        check(lib().kh_trie_copy(self.h, ctypes.byref(h)))
        f = ResidentForest.__new__(ResidentForest)
        f.ctx, f.dev, f.h, f.hash_keys = self.ctx, self.dev, h, self.hash_keys
        return f

    def last_roots(self):
        """{trie_id: root} of the last commit (kh_forest_last_roots; also after block_commit)."""
        n = ctypes.c_uint64()
        rc = lib().kh_forest_last_roots(self.h, None, None, 0, ctypes.byref(n))
        if rc not in (_lib.KH_OK, _lib.KH_ENOSPC):
            check(rc)
        cap = n.value
        tries = np.zeros(max(cap, 1), np.uint32)
        roots = np.zeros(32 * max(cap, 1), np.uint8)
        check(lib().kh_forest_last_roots(self.h, tries.ctypes.data, roots.ctypes.data, cap, ctypes.byref(n)))
        return {int(tries[i]): roots[32 * i:32 * i + 32].tobytes() for i in range(n.value)}

    def __len__(self):
        n = ctypes.c_uint64()
        check(lib().kh_trie_size(self.h, ctypes.byref(n)))
        return int(n.value)

    def close(self):
        if self.h:
            lib().kh_trie_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def block_commit(state, forest, s_up_trie, s_up_keys, s_up_vals, s_up_voff, ns_up, s_del_trie, s_del_keys, ns_del,
                 a_up_keys, a_up_vals, a_up_voff, a_up_trie, na_up, a_del_keys, na_del, s_klen=32, a_klen=32,
                 stats=None):
    """One block through kh_block_commit (device tensors): the storage ops into the forest,
    the touched tries' new roots written into the stateRoot of the account upserts that name
    them (a_up_trie, KH_NO_TRIE for none; a_up_vals is patched in place), then the account
    ops into the state trie.  Returns the new state root."""
    root = np.zeros(32, np.uint8)
    st = stats if stats is not None else KhStats()
    state.ctx._sync()
    check(lib().kh_block_commit(state.h, forest.h, _ptr(s_up_trie), _ptr(s_up_keys), _ptr(s_up_vals), _ptr(s_up_voff),
                                ns_up, _ptr(s_del_trie), _ptr(s_del_keys), ns_del, s_klen, _ptr(a_up_keys),
                                _ptr(a_up_vals), _ptr(a_up_voff), _ptr(a_up_trie), na_up, _ptr(a_del_keys), na_del,
                                a_klen, root.ctypes.data, ctypes.byref(st)))
    state.root = root.tobytes()
    return state.root


def block_commit_host(state, forest, s_up_trie, s_up_keys, s_up_vals, s_up_voff, s_del_trie, s_del_keys,
                      a_up_keys, a_up_vals, a_up_voff, a_up_trie, a_del_keys, s_klen=32, a_klen=32, stats=None):
    """kh_block_commit_host: the same block from host (numpy) arrays; counts from the shapes."""
    keep = []  # contiguous copies stay alive through the call

    def p(a):
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        keep.append(a)
        return a.ctypes.data
    ns_up = 0 if s_up_trie is None else len(s_up_trie)
    ns_del = 0 if s_del_trie is None else len(s_del_trie)
    na_up = len(a_up_voff) - 1
    na_del = 0 if a_del_keys is None else len(a_del_keys) // a_klen
    root = np.zeros(32, np.uint8)
    st = stats if stats is not None else KhStats()
    state.ctx._sync()
    check(lib().kh_block_commit_host(state.h, forest.h, p(s_up_trie), p(s_up_keys), p(s_up_vals), p(s_up_voff), ns_up,
                                     p(s_del_trie), p(s_del_keys), ns_del, s_klen, p(a_up_keys), p(a_up_vals),
                                     p(a_up_voff), p(a_up_trie), na_up, p(a_del_keys), na_del, a_klen,
                                     root.ctypes.data, ctypes.byref(st)))
    del keep
    state.root = root.tobytes()
    return state.root
