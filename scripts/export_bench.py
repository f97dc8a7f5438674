"""Node export and nodes-by-hash on a resident state trie of N synthetic accounts.

  python scripts/export_bench.py --n 1000000 [--dict] --out profiles/NAME.json

Measures, on one GPU, wall clock around the C ABI calls (buffers allocated once, outside):
  - the full export (kh_trie_export_nodes driven to the end into 1M-node / 256 MiB host buffers),
    with and without KH_EXPORT_VERIFY: nodes/s and GB/s of encodings + hashes to the host;
  - warm kh_trie_nodes_by_hash of 400 hashes spread over the store (one GetNodeData message,
    max-mpt-components-per-message = 400): median and spread of --reps calls;
  - with --dict, the stated baseline: the same 400 nodes fetched one by one from a Python dict
    of the exported store.
One JSON object; nothing here is gated."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--cfg", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--hash-reps", type=int, default=20)
    ap.add_argument("--dict", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from khipu_amd import _lib
    from khipu_amd._lib import check, lib
    from khipu_amd.device import Ctx, ResidentTrie
    ctx = Ctx(0)
    addr, vals, voff = ctx.synth_accounts(a.cfg, 0, a.n)
    t = ResidentTrie.__new__(ResidentTrie)
    t.ctx, t.dev, t.h = ctx, "cuda:0", None
    t0 = time.perf_counter()
    t._open(addr, 20, vals, voff, a.n, True, emit=False)
    torch.cuda.synchronize()
    open_s = time.perf_counter() - t0
    del addr, vals, voff
    use = t.usage()
    node_cap, rlp_cap = 1 << 20, 256 << 20
    hs = np.zeros(32 * node_cap, np.uint8)
    rl = np.zeros(rlp_cap, np.uint8)
    of = np.zeros(node_cap + 1, np.uint64)
    nn, nl, done = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_int(0)

    def export(flags, keep=None, sample=None):
        cur = _lib.KhExportCursor()
        nodes = nbytes = calls = 0
        done.value = 0
        t0 = time.perf_counter()
        while not done.value:
            check(lib().kh_trie_export_nodes(t.h, _lib.KH_NO_TRIE, flags, ctypes.byref(cur), hs.ctypes.data, node_cap,
                                             rl.ctypes.data, rlp_cap, of.ctypes.data, ctypes.byref(nn), ctypes.byref(nl),
                                             ctypes.byref(done)))
            k = nn.value
            if keep is not None:  # (not timed runs: the dict baseline's store)
                for i in range(k):
                    keep[hs[32 * i:32 * i + 32].tobytes()] = rl[of[i]:of[i + 1]].tobytes()
            if sample is not None and k:
                for i in range(0, k, max(k // 512, 1)):
                    sample.append(hs[32 * i:32 * i + 32].tobytes())
            nodes += k
            nbytes += nl.value
            calls += 1
        return time.perf_counter() - t0, nodes, nbytes, calls

    sample = []
    export(0, sample=sample)  # warm-up: buffers sized, pages touched
    res = {"n_accounts": a.n, "cfg": a.cfg, "open_s": round(open_s, 3), "usage": use, "node_cap": node_cap,
           "rlp_cap": rlp_cap}
    for name, flags in (("export", 0), ("export_verify", _lib.KH_EXPORT_VERIFY)):
        runs = [export(flags) for _ in range(a.reps)]
        s = sorted(r[0] for r in runs)
        _, nodes, nbytes, calls = runs[0]
        med = statistics.median(s)
        res[name] = {"seconds": [round(x, 4) for x in s], "nodes": nodes, "rlp_bytes": nbytes, "calls": calls,
                     "nodes_per_s": round(nodes / med), "gb_per_s_to_host": round((nbytes + 40 * nodes) / med / 1e9, 3)}
    # 400 hashes spread over the store
    step = max(len(sample) // 400, 1)
    q = sample[::step][:400]
    hb = np.frombuffer(b"".join(q), np.uint8).copy()
    found = np.zeros(len(q), np.uint8)
    off = np.zeros(len(q) + 1, np.uint64)
    need = ctypes.c_uint64(0)
    out = np.zeros(1 << 20, np.uint8)

    def by_hash():
        t0 = time.perf_counter()
        check(lib().kh_trie_nodes_by_hash(t.h, hb.ctypes.data, len(q), found.ctypes.data, out.ctypes.data, out.size,
                                          off.ctypes.data, ctypes.byref(need)))
        return time.perf_counter() - t0
    for _ in range(3):
        by_hash()
    assert int(found.sum()) == len(q)
    ts = sorted(by_hash() for _ in range(a.hash_reps))
    rec_bytes = use["records"] * 128
    res["by_hash_400"] = {"hashes": len(q), "ms_median": round(1e3 * statistics.median(ts), 3),
                          "ms_min": round(1e3 * ts[0], 3), "ms_max": round(1e3 * ts[-1], 3),
                          "record_bytes": rec_bytes,
                          "record_gb_per_s_at_median": round(rec_bytes / statistics.median(ts) / 1e9, 1)}
    if a.dict:
        store = {}
        export(0, keep=store)
        ds = []
        for _ in range(a.hash_reps):
            t0 = time.perf_counter()
            got = [store.get(h) for h in q]
            ds.append(time.perf_counter() - t0)
        assert all(g is not None for g in got)
        res["dict_400"] = {"entries": len(store), "ms_median": round(1e3 * statistics.median(ds), 4)}
    t.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
