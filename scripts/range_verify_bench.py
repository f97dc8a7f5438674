"""Range verification (kh_verify_ranges / kh_dev_verify_ranges) on a synthetic hashed account trie
("Range verification").

  python scripts/range_verify_bench.py [--n 1000000] [--out profiles/range_verify.json]

One GPU; random origins, medians of --reps calls after 3 warm-ups.  Every timed call is measured
as host wall clock around the C ABI call; the device form also between two events on the
context's stream.
  page_1000, page_100000   one proved page served by range_proof, verified: host form (inputs
                           staged from host memory) and device form (inputs already in HBM)
  storage                  one call of --tries unproved ten-slot storage tries plus one proved tail,
                           and the same ranges as --tries + 1 single-range calls
Baselines in the same session: kh_trie_root / kh_trie_roots_segmented over the same entries, on
arrays packed beforehand (a trie built from the entries alone: the floor), and kh_verify_proofs of
the two boundary keys.
--bench-parent / --bench-this: bench.py result lines of the parent's build and of this tree,
recorded beside the measurements.  One JSON object; nothing here is gated."""
import argparse
import ctypes
import json
import os
import random
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--cfg", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--pages", default="1000,100000")
    ap.add_argument("--tries", type=int, default=2000)
    ap.add_argument("--slots", type=int, default=10)
    ap.add_argument("--bench-parent", default="")
    ap.add_argument("--bench-this", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from khipu_amd import _lib
    from khipu_amd._lib import KhStats, check, lib
    from khipu_amd.device import Ctx, ResidentTrie, _range_arrays, verify_proofs
    from khipu_amd.trie import trie_root, trie_roots
    L = lib()
    res = {"n_accounts": a.n, "cfg": a.cfg, "reps": a.reps}
    warm = 3

    def stats(ts):
        ts = sorted(ts)
        return {"median": round(statistics.median(ts), 3), "min": round(ts[0], 3), "max": round(ts[-1], 3)}

    def timed(fn, reps=None):
        out = []
        for i in range((reps or a.reps) + warm):
            t0 = time.perf_counter()
            fn()
            t1 = time.perf_counter()
            if i >= warm:
                out.append(1e3 * (t1 - t0))
        return stats(out)

    ctx = Ctx(0)
    addr, vals, voff = ctx.synth_accounts(a.cfg, 0, a.n)
    t = ResidentTrie.__new__(ResidentTrie)
    t.ctx, t.dev, t.h = ctx, "cuda:0", None
    t._open(addr, 20, vals, voff, a.n, True, emit=False)
    torch.cuda.synchronize()
    root = t.root
    stream = torch.cuda.Stream()
    check(L.kh_ctx_set_stream(ctx.h, ctypes.c_void_p(stream.cuda_stream)))
    rnd = random.Random(5)

    def host_call(nr, nn, arr):
        status, more, miss = np.zeros(nr, np.uint8), np.zeros(nr, np.uint8), np.zeros(32 * nr, np.uint8)
        p = {k: (v.ctypes.data if v is not None else None) for k, v in arr.items()}

        def call(keep=arr):  # (the arrays live as long as the call that points into them)
            check(L.kh_verify_ranges(p["roots"], p["origins"], p["proved"], nr, p["keys"], p["vals"], p["voff"],
                                     p["ent_off"], p["enc"], p["off"], nn, status.ctypes.data, more.ctypes.data,
                                     miss.ctypes.data))
        return call, status, more

    def dev_call(nr, nn, arr):
        d = {k: torch.from_numpy(v.view(np.int64) if v.dtype == np.uint64 else v).to("cuda:0") for k, v in arr.items()
             if v is not None}
        status, more = np.zeros(nr, np.uint8), np.zeros(nr, np.uint8)
        p = {k: ctypes.c_void_p(v.data_ptr()) for k, v in d.items()}
        torch.cuda.synchronize()

        def call():
            check(L.kh_dev_verify_ranges(ctx.h, p["roots"], p.get("origins"), p["proved"], nr, p["keys"], p["vals"],
                                         p["voff"], p["ent_off"], p["enc"], p["off"], nn, status.ctypes.data,
                                         more.ctypes.data, None))
        return call, status, more, d

    def dev_timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        wall, dev = [], []
        for i in range(a.reps + warm):
            with torch.cuda.stream(stream):
                e0.record()
                t0 = time.perf_counter()
                call()
                t1 = time.perf_counter()
                e1.record()
            e1.synchronize()
            if i >= warm:
                wall.append(1e3 * (t1 - t0))
                dev.append(e0.elapsed_time(e1))
        return {"wall_ms": stats(wall), "stream_event_ms": stats(dev)}

    tail = None
    for c in [int(p) for p in a.pages.split(",")]:
        # a page above an origin in the lower 85 % of the (uniform) hashed key space: full, with more = 1
        origin = rnd.randrange(int(0.85 * 2 ** 256)).to_bytes(32, "big")
        keys, pvals, more, _, table = t.range_proof(origin, None, c, val_cap=256 * c)
        assert len(keys) == c and more
        args = ([root], [origin], [(keys, pvals)], table, None)
        nr, nn, arr = _range_arrays(*args)
        out = {"entries": c, "value_bytes": int(arr["voff"][-1]), "proof_nodes": nn}
        call, status, mo = host_call(nr, nn, arr)
        out["verify_host_form_wall_ms"] = timed(call)
        assert status[0] == _lib.KH_RANGE_OK and mo[0] == 1
        call, status, mo, keep = dev_call(nr, nn, arr)
        out["verify_device_form"] = dev_timed(call)
        assert status[0] == _lib.KH_RANGE_OK and mo[0] == 1
        # the floor: a trie built from the entries alone; and the two boundary proofs checked singly
        kb = arr["keys"][:32 * c]
        out["trie_root_of_entries_wall_ms"] = timed(lambda: trie_root(kb, (arr["vals"], arr["voff"])))
        ends = [origin, keys[-1]]
        out["verify_proofs_of_2_keys_wall_ms"] = timed(lambda: verify_proofs(root, ends, table))
        res[f"page_{c}"] = out
        if tail is None:
            tail = (origin, keys, pvals, table)
        del keep
    # a storage-ranges response: whole small tries and one proved tail
    nt, sl = a.tries, a.slots
    g = np.random.default_rng(11)
    sk = [sorted(bytes(g.integers(0, 256, 32, dtype=np.uint8)) for _ in range(sl)) for _ in range(nt)]
    sv = [[b"\xa0" + bytes(g.integers(0, 256, 32, dtype=np.uint8)) for _ in range(sl)] for _ in range(nt)]
    sroots = trie_roots(list(zip(sk, sv)))
    o, keys, pvals, table = tail
    args = (list(sroots) + [root], [None] * nt + [o], list(zip(sk, sv)) + [(keys, pvals)], table, [0] * nt + [1])
    nr, nn, arr = _range_arrays(*args)
    out = {"tries": nt, "slots": sl, "tail_entries": len(keys)}
    call, status, mo = host_call(nr, nn, arr)
    out["one_call_host_form_wall_ms"] = timed(call)
    assert (status == _lib.KH_RANGE_OK).all() and mo[nt] == 1
    call, status, mo, keep = dev_call(nr, nn, arr)
    out["one_call_device_form"] = dev_timed(call)
    assert (status == _lib.KH_RANGE_OK).all()
    singles = [host_call(*_range_arrays([args[0][s]], [args[1][s]], [args[2][s]], table if args[4][s] else [],
                                        [args[4][s]]))[0] for s in range(nr)]

    def all_single():
        for f in singles:
            f()
    out["single_range_calls_wall_ms"] = timed(all_single)
    # the floor on the call's own packed arrays: the nt whole tries are its first nt segments
    sroot = np.zeros(32 * nt, np.uint8)
    st = KhStats()

    def seg_roots():
        check(L.kh_trie_roots_segmented(arr["keys"].ctypes.data, 32, arr["vals"].ctypes.data, arr["voff"].ctypes.data,
                                        arr["ent_off"].ctypes.data, nt, 0, sroot.ctypes.data, ctypes.byref(st)))
    out["trie_roots_segmented_wall_ms"] = timed(seg_roots)
    assert sroot.tobytes() == b"".join(sroots)
    res["storage"] = out
    for name, path in (("bench_parent", a.bench_parent), ("bench_this", a.bench_this)):
        if path and os.path.exists(path):
            with open(path) as f:
                lines = [ln for ln in f.read().split("\n") if ln.startswith("{")]
            res[name] = json.loads(lines[-1]) if lines else None
    t.close()
    check(L.kh_ctx_set_stream(ctx.h, None))
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
