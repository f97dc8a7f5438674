"""Range fills (kh_trie_fill_ranges_host): what it costs to make a root-only handle the full resident
trie page by page, beside the one route there was before -- verify every page without a handle and
open the trie from all entries at the end.

  python scripts/fill_ranges_bench.py [--accounts 1000000] [--pages 1000,100000] [--reps 20] [--warmup 3] [--out FILE]

N synthetic accounts (csrc/synth.h, config 3) under hashed keys in a full resident trie that serves
the boundary proofs (kh_trie_prove, trie keys); the pages are cut from the sorted content.  From
one session, the wall clock around each call and stream events around it (every call ends in a
synchronise):
  (a) sync      per page size: a root-only handle takes every page -- kh_trie_fill_nodes over the
                page's boundary proof (nothing else goes through it), then kh_trie_fill_ranges_host.
                Per fill call the median after the warm-up calls; the whole sync (proof fills and
                range fills summed) once.  A page size with fewer calls a sync than warm-ups + reps
                is synced again from a fresh root-only handle until there are enough.
  (b) baseline  kh_verify_ranges per page over the same proof, then ONE kh_trie_open_host over all
                entries: nothing is resident until that open returns.  Wall clock (the stateless
                calls run on the library's shared context).
  (c) storage   a GetStorageRanges-shaped call into a forest: 2,000 whole ten-slot tries and the tail
                page of one larger, partly resident trie, in ONE kh_trie_fill_ranges_host; a fresh
                forest each repetition.
Prints one JSON line; --out also writes it.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from khipu_amd._lib import check, lib  # noqa: E402
from khipu_amd.device import Ctx, ResidentForest, ResidentTrie, trie_prove  # noqa: E402
from tests.blocks import CFG, hash_keys  # noqa: E402

DEV = "cuda:0"
u64 = ctypes.c_uint64
ZERO = b"\x00" * 32


def med(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "calls": len(xs)}


def timed(stream, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record(stream)
    r = fn()
    e1.record(stream)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1), r


def step(k):
    return ((int.from_bytes(k, "big") + 1) % (1 << 256)).to_bytes(32, "big")


def sorted_content(keys, vals, voff, n):
    """(keys [n, 32], packed values, offsets) in key order, on the host."""
    kk = keys.view(n, 32).cpu().numpy()
    be = kk.view(">u8")
    order = np.lexsort((be[:, 3], be[:, 2], be[:, 1], be[:, 0]))
    vo = voff[:n + 1].cpu().numpy().astype(np.uint64)
    lens = np.diff(vo)[order]
    nvo = np.zeros(n + 1, np.uint64)
    np.cumsum(lens, out=nvo[1:])
    hv = vals.cpu().numpy()
    out = np.zeros(int(nvo[-1]) + 64, np.uint8)
    at = vo[:-1][order].astype(np.int64)
    for c in range(0, n, 1 << 16):  # (in chunks: the byte index of a 1M-account gather is not held at once)
        e = min(c + (1 << 16), n)
        b0, b1 = int(nvo[c]), int(nvo[e])
        ln = lens[c:e].astype(np.int64)
        src = np.repeat(at[c:e] - (nvo[c:e].astype(np.int64) - b0), ln) + np.arange(b1 - b0, dtype=np.int64)
        out[b0:b1] = hv[src]
    return np.ascontiguousarray(kk[order]), out, nvo


def pack(encs):
    off = np.zeros(len(encs) + 1, np.uint64)
    np.cumsum([len(e) for e in encs], out=off[1:])
    return np.frombuffer(b"".join(encs) + b"\0", np.uint8).copy(), off


def fill_call(h, tries, roots, origins, nr, K, V, VO, eo):
    st, left = np.zeros(nr + 1, np.uint8), np.zeros(nr + 1, np.uint64)
    nk, ns = u64(), u64()
    rc = lib().kh_trie_fill_ranges_host(h, tries.ctypes.data if tries is not None else None, roots.ctypes.data,
                                        origins.ctypes.data, nr, K.ctypes.data, V.ctypes.data, VO.ctypes.data,
                                        eo.ctypes.data, st.ctypes.data, left.ctypes.data, ctypes.byref(nk),
                                        ctypes.byref(ns))
    check(rc)
    assert not st[:nr].any(), st[:nr]
    return left[:nr], nk.value, ns.value


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--accounts", type=int, default=1_000_000)
    p.add_argument("--pages", default="1000,100000")
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--storage-tries", type=int, default=2000)
    p.add_argument("--out")
    a = p.parse_args()
    n = a.accounts
    ctx = Ctx(0)
    addr, vals, voff = ctx.synth_accounts(CFG, 0, n)
    keys = hash_keys(ctx, addr, 20, n)
    full = ResidentTrie.__new__(ResidentTrie)
    full.ctx, full.dev, full.h = ctx, DEV, None
    full._open(keys, 32, vals, voff, n, False, emit=False)
    torch.cuda.synchronize()
    K, V, VO = sorted_content(keys, vals, voff, n)
    root = full.root
    rootb = np.frombuffer(root, np.uint8).copy()
    root_enc = full.nodes_by_hash([root])[0]
    stream = torch.cuda.Stream()  # the handles' calls run on their context's stream: one the events can be recorded on
    check(lib().kh_ctx_set_stream(ctx.h, ctypes.c_void_p(stream.cuda_stream)))
    res = {"accounts": n, "reps": a.reps, "warmup": a.warmup, "root": root.hex(), "sync": {}, "baseline": {}}

    def pages_of(size):
        """(first entry, one past the last, origin, proof encodings) per page, the proofs from the full handle"""
        out, origin = [], ZERO
        for s in range(0, n, size):
            e = min(s + size, n)
            hi = K[e - 1].tobytes()
            _, table = trie_prove(full.h, [origin, hi], None, shared=True, trie_keys=True)
            out.append((s, e, origin, list(table.nodes)))
            origin = step(hi)
        return out

    for size in [int(x) for x in a.pages.split(",")]:
        pg = pages_of(size)
        fw, fe, whole = [], [], None
        while len(fw) < a.warmup + a.reps:
            t = ResidentTrie.from_witness(ctx, root, {root: root_enc}, emit=False)
            proof_ms = fill_ms = 0.0
            for s, e, origin, proof in pg:
                w, _, _ = timed(stream, lambda: t.fill(proof))
                proof_ms += w
                ob, eo = np.frombuffer(origin, np.uint8).copy(), np.asarray([s, e], np.uint64)
                w, ev, (left, _, _) = timed(stream, lambda: fill_call(t.h, None, rootb, ob, 1, K, V, VO, eo))
                fill_ms += w
                fw.append(w), fe.append(ev)
            assert left[0] == 0 and t.stubs == 0 and len(t) == n and t.get_root() == root
            whole = {"pages": len(pg), "proof_fills_wall_ms": round(proof_ms, 1), "range_fills_wall_ms": round(fill_ms, 1),
                     "total_wall_ms": round(proof_ms + fill_ms, 1)}
            t.close()
        res["sync"][str(size)] = {"fill_call_wall_ms": med(fw[a.warmup:]), "fill_call_event_ms": med(fe[a.warmup:]),
                                  "whole_sync": whole}
        # (b) the same pages verified without a handle, then one open over all entries
        vw = []
        one = np.ones(1, np.uint8)
        for s, e, origin, proof in pg:
            enc, off = pack(proof)
            ob, eo = np.frombuffer(origin, np.uint8).copy(), np.asarray([s, e], np.uint64)
            st, more, miss = np.zeros(2, np.uint8), np.zeros(2, np.uint8), np.zeros(33, np.uint8)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            check(lib().kh_verify_ranges(rootb.ctypes.data, ob.ctypes.data, one.ctypes.data, 1, K.ctypes.data,
                                         V.ctypes.data, VO.ctypes.data, eo.ctypes.data, enc.ctypes.data, off.ctypes.data,
                                         len(proof), st.ctypes.data, more.ctypes.data, miss.ctypes.data))
            vw.append((time.perf_counter() - t0) * 1e3)
            assert st[0] == 0
        h, r2 = ctypes.c_void_p(), np.zeros(32, np.uint8)
        t0 = time.perf_counter()
        check(lib().kh_trie_open_host(K.ctypes.data, 32, V.ctypes.data, VO.ctypes.data, n, 0, r2.ctypes.data, ctypes.byref(h)))
        open_ms = (time.perf_counter() - t0) * 1e3
        assert r2.tobytes() == root
        check(lib().kh_trie_free(h))
        res["baseline"][str(size)] = {"verify_call_wall_ms": med(vw[a.warmup:] if len(vw) > a.warmup else vw),
                                      "verify_total_wall_ms": round(sum(vw), 1), "open_host_wall_ms": round(open_ms, 1),
                                      "total_wall_ms": round(sum(vw) + open_ms, 1)}
    # (c) 2,000 whole ten-slot tries and one tail in one call
    nt, tail_id, tail_n = a.storage_tries, a.storage_tries + 7, 5000
    rng = np.random.default_rng(5)

    def slots(k):
        kk = rng.integers(0, 256, (k, 32), dtype=np.uint8)
        be = kk.view(">u8")
        return np.ascontiguousarray(kk[np.lexsort((be[:, 3], be[:, 2], be[:, 1], be[:, 0]))])
    sk = np.concatenate([slots(10) for _ in range(nt)] + [slots(tail_n)])
    ne = len(sk)
    sv = rng.integers(1, 256, ne * 33, dtype=np.uint8)
    svo = np.arange(ne + 1, dtype=np.uint64) * 33
    ids = np.concatenate([np.repeat(np.arange(nt, dtype=np.uint32), 10), np.full(tail_n, tail_id, np.uint32)])
    srv = ResidentForest(ctx, emit=False)
    ht, hr, ntr = np.zeros(nt + 1, np.uint32), np.zeros(32 * (nt + 1), np.uint8), u64()
    check(lib().kh_forest_apply_host(srv.h, ids.ctypes.data, sk.ctypes.data, sv.ctypes.data, svo.ctypes.data, ne, None,
                                     None, 0, 32, ht.ctypes.data, hr.ctypes.data, nt + 1, ctypes.byref(ntr), None))
    roots = {int(ht[i]): hr[32 * i:32 * i + 32].tobytes() for i in range(ntr.value)}
    cut = tail_n - 1000  # the tail: the last 1,000 slots of the larger trie
    t_origin = sk[10 * nt + cut].tobytes()
    _, table = trie_prove(srv.h, [t_origin, sk[-1].tobytes()], [tail_id, tail_id], shared=True, trie_keys=True)
    witness = list(table.nodes)
    tr = np.concatenate([np.arange(nt, dtype=np.uint32), np.asarray([tail_id], np.uint32)])
    rb = np.frombuffer(b"".join(roots[int(t)] for t in tr), np.uint8).copy()
    og = np.zeros(32 * (nt + 1), np.uint8)
    og[32 * nt:] = np.frombuffer(t_origin, np.uint8)
    # the call's entries: every whole trie, then the tail from its cut
    sk2 = np.concatenate([sk[:10 * nt], sk[10 * nt + cut:]])
    sv2 = np.concatenate([sv[:330 * nt], sv[33 * (10 * nt + cut):]])
    ne2 = len(sk2)
    svo2 = np.arange(ne2 + 1, dtype=np.uint64) * 33
    eo = np.concatenate([np.arange(nt + 1, dtype=np.uint64) * 10, np.asarray([ne2], np.uint64)])
    cw, ce = [], []
    for rep in range(a.warmup + a.reps):
        f = ResidentForest(ctx, emit=False)
        f.load_partial({tail_id: roots[tail_id]}, witness)
        w, ev, (left, nk, ns) = timed(stream, lambda: fill_call(f.h, tr, rb, og, nt + 1, sk2, sv2, svo2, eo))
        assert nk >= 10 * nt and not left[:nt].any() and f.roots() == roots
        if rep >= a.warmup:
            cw.append(w), ce.append(ev)
        f.close()
    res["storage"] = {"whole_tries": nt, "slots_each": 10, "tail_entries": tail_n - cut, "ranges": nt + 1, "entries": ne2,
                      "fill_call_wall_ms": med(cw), "fill_call_event_ms": med(ce)}
    srv.close()
    full.close()
    torch.cuda.synchronize()
    check(lib().kh_ctx_set_stream(ctx.h, None))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
