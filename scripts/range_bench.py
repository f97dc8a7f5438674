"""Range scans on a resident state trie of N synthetic accounts, hashed keys ("Range scan").

  python scripts/range_bench.py --n 1000000 --out profiles/range_scan.json

On one GPU, for a handle of N accounts and one of 10 N (the claim under test: a page's cost follows
the page, not the trie), warm, buffers allocated once outside the clock:
  - kh_trie_range_host of 1,000 and 100,000 entries from random origins: median wall clock around
    the call, the event-to-event time on the handle's stream (it spans the whole call, the idle gaps
    while the host reads a round's counters included), and the rounds taken;
  - the stated baseline, the nearest existing read: kh_trie_get_host of the same number of known
    keys on the same handle in the same session (the per-entry descent).
One JSON object; nothing here is gated."""
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
    ap.add_argument("--scale", type=int, default=10)
    ap.add_argument("--cfg", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--pages", default="1000,100000")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from khipu_amd import _lib
    from khipu_amd._lib import check, lib
    from khipu_amd.device import Ctx, ResidentTrie
    pages = [int(p) for p in a.pages.split(",")]
    lib().khst_range_rounds.restype = ctypes.c_uint32
    res = {"cfg": a.cfg, "reps": a.reps, "handles": []}

    def stats(ts):
        ts = sorted(ts)
        return {"median": round(statistics.median(ts), 3), "min": round(ts[0], 3), "max": round(ts[-1], 3)}

    for n in (a.n, a.scale * a.n):
        ctx = Ctx(0)
        addr, vals, voff = ctx.synth_accounts(a.cfg, 0, n)
        t = ResidentTrie.__new__(ResidentTrie)
        t.ctx, t.dev, t.h = ctx, "cuda:0", None
        t._open(addr, 20, vals, voff, n, True, emit=False)
        torch.cuda.synchronize()
        # the handle's calls run on its context's stream: a stream the events below can be recorded on
        stream = torch.cuda.Stream()
        check(lib().kh_ctx_set_stream(ctx.h, ctypes.c_void_p(stream.cuda_stream)))
        addrs = addr[:n * 20].view(-1, 20)
        rnd = random.Random(5)
        out = {"n_accounts": n, "usage": t.usage()}
        for c in pages:
            keys = np.zeros(32 * c, np.uint8)
            vbuf = np.zeros(256 * c, np.uint8)
            vo = np.zeros(c + 1, np.uint64)
            nxt = np.zeros(32, np.uint8)
            ne, vb, more = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_int(0)
            # origins in the lower 85 % of the (uniform) hashed key space: a full page lies above each
            origins = [np.frombuffer(rnd.randrange(int(0.85 * 2 ** 256)).to_bytes(32, "big"), np.uint8).copy()
                       for _ in range(a.reps + 3)]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            wall, dev, rounds = [], [], []
            for i, og in enumerate(origins):
                with torch.cuda.stream(stream):
                    e0.record()
                    t0 = time.perf_counter()
                    check(lib().kh_trie_range_host(t.h, 0, og.ctypes.data, None, c, keys.ctypes.data, vbuf.ctypes.data,
                                                   vbuf.size, vo.ctypes.data, ctypes.byref(ne), ctypes.byref(vb),
                                                   ctypes.byref(more), nxt.ctypes.data, None))
                    t1 = time.perf_counter()
                    e1.record()
                e1.synchronize()
                assert ne.value == c and more.value == 1, (ne.value, more.value)
                assert keys[:32].tobytes() >= og.tobytes() and keys[32 * (c - 1):32 * c].tobytes() < nxt.tobytes()
                if i >= 3:  # (three warm-up calls)
                    wall.append(1e3 * (t1 - t0))
                    dev.append(e0.elapsed_time(e1))
                    rounds.append(int(lib().khst_range_rounds()))
            page_bytes = int(vb.value)
            # the baseline: get of c known keys (raw addresses, hashed on the device as a commit does)
            pick = addrs[torch.randint(0, n, (c,), device=addrs.device, generator=None)].cpu().numpy().copy()
            found = np.zeros(c, np.uint8)
            gw = []
            for i in range(a.reps + 3):
                t0 = time.perf_counter()
                check(lib().kh_trie_get_host(t.h, None, pick.ctypes.data, 20, c, vbuf.ctypes.data, vbuf.size,
                                             vo.ctypes.data, found.ctypes.data, ctypes.byref(vb)))
                t1 = time.perf_counter()
                if i >= 3:
                    gw.append(1e3 * (t1 - t0))
            assert int(found.sum()) == c
            out[f"range_{c}"] = {"wall_ms": stats(wall), "stream_event_ms": stats(dev), "rounds": sorted(set(rounds)),
                                 "value_bytes": page_bytes}
            out[f"get_{c}"] = {"wall_ms": stats(gw)}
        res["handles"].append(out)
        t.close()
        del addr, vals, voff, addrs
        torch.cuda.synchronize()
        check(lib().kh_ctx_set_stream(ctx.h, None))
        ctx.close()
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
