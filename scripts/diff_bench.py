"""Trie diff on a resident state trie of N synthetic accounts, hashed keys ("Trie diff").

  python scripts/diff_bench.py --n 1000000 --out profiles/trie_diff.json

On one GPU: a handle of N accounts and its copy(); one block committed on the original (18,000
updates, 1,000 inserts, 1,000 deletes); then the copy (side a) diffed against the original (side b),
warm, buffers allocated once outside the clock:
  - the whole key space in one call, and pages of 1,000 differences followed by `next`: the median of
    20 calls after 3 warm-ups of the wall clock around the call and of the event-to-event time on the
    handle's stream (it spans the whole call, the idle gaps while the host reads a round's counters
    included), the rounds taken and the frontier items selected;
  - the stated baseline, the only way to the same answer without this call, in the same session: a
    complete range scan of both handles (pages of 100,000 entries) merged on the host.
Full handles only.  One JSON object; nothing here is gated."""
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--updates", type=int, default=18_000)
    ap.add_argument("--inserts", type=int, default=1_000)
    ap.add_argument("--deletes", type=int, default=1_000)
    ap.add_argument("--page", type=int, default=1_000)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from khipu_amd._lib import check, lib
    from khipu_amd.device import Ctx, ResidentTrie, diff_counters
    n, nu, ni, nd = a.n, a.updates, a.inserts, a.deletes
    assert 2 * nu + nd <= n
    ctx = Ctx(0)
    addr, vals, voff = ctx.synth_accounts(a.cfg, 0, n + ni)
    t = ResidentTrie.__new__(ResidentTrie)
    t.ctx, t.dev, t.h, t.hash_keys = ctx, "cuda:0", None, True
    t._open(addr, 20, vals, voff, n, True, emit=False)
    base = t.copy()
    # the block: accounts [0, nu) take the values of accounts [nu, 2 nu), accounts [n, n + ni) are new,
    # the last nd accounts go
    off = voff.cpu().numpy()
    up_keys = torch.cat([addr[:20 * nu], addr[20 * n:20 * (n + ni)]]).contiguous()
    up_vals = torch.cat([vals[int(off[nu]):int(off[2 * nu])], vals[int(off[n]):int(off[n + ni])]]).contiguous()
    uo = np.concatenate([off[nu:2 * nu] - off[nu], off[n:n + ni + 1] - off[n] + (off[2 * nu] - off[nu])]).astype(np.int64)
    up_voff = torch.from_numpy(uo).to("cuda:0")
    del_keys = addr[20 * (n - nd):20 * n].contiguous()
    t.commit_dev(up_keys, up_vals, up_voff, nu + ni, del_keys, nd, klen=20)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()  # the handles' calls run on their context's stream: one the events can be recorded on
    check(lib().kh_ctx_set_stream(ctx.h, ctypes.c_void_p(stream.cuda_stream)))
    want = None  # the differences: nd + ni + the updates whose new value differs from the old one
    res = {"n_accounts": n, "cfg": a.cfg, "reps": a.reps, "block": {"updates": nu, "inserts": ni, "deletes": nd},
           "usage": t.usage()}

    def stats(ts):
        ts = sorted(ts)
        return {"median": round(statistics.median(ts), 3), "min": round(ts[0], 3), "max": round(ts[-1], 3)}

    cap = 1 << 16
    assert nu + ni + nd < cap
    keys = np.zeros(32 * cap, np.uint8)
    kinds = np.zeros(cap, np.uint8)
    vbuf = np.zeros(128 * cap, np.uint8)
    vo = np.zeros(cap + 1, np.uint64)
    nxt = np.zeros(32, np.uint8)
    ne, vb, more = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_int(0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def call(origin, mx):
        with torch.cuda.stream(stream):
            e0.record()
            t0 = time.perf_counter()
            check(lib().kh_trie_diff_host(base.h, 0, t.h, 0, origin, None, mx, vbuf.size, keys.ctypes.data,
                                          kinds.ctypes.data, vbuf.ctypes.data, vo.ctypes.data, ctypes.byref(ne),
                                          ctypes.byref(vb), ctypes.byref(more), nxt.ctypes.data, None))
            t1 = time.perf_counter()
            e1.record()
        e1.synchronize()
        return 1e3 * (t1 - t0), e0.elapsed_time(e1), diff_counters()

    # (a) the whole key space in one call
    wall, dev, cost = [], [], set()
    for i in range(a.reps + 3):
        w, d, c = call(None, cap)
        want = int(ne.value) if want is None else want
        assert ne.value == want and more.value == 0, (ne.value, more.value)
        if i >= 3:
            wall.append(w)
            dev.append(d)
            cost.add(c)
    hist = np.bincount(kinds[:want], minlength=4)
    # (synthetic accounts repeat a few values: an update to an equal value is no difference; the
    # baseline's merge below is what the keys are held to)
    assert (int(hist[1]), int(hist[2])) == (nd, ni) and 0.99 * nu <= int(hist[3]) <= nu, hist
    res["whole"] = {"differences": want, "kinds_1_2_3": [int(hist[1]), int(hist[2]), int(hist[3])], "value_bytes": int(vb.value), "wall_ms": stats(wall), "stream_event_ms": stats(dev),
                    "rounds_visited": sorted(cost)}
    whole_keys = keys[:32 * want].copy()
    # (b) pages of a.page differences, followed by next to the end, reps calls after 3 warm-ups
    wall, dev, cost, got, origin, calls = [], [], set(), [], None, 0
    for _ in range(3):
        call(None, a.page)
    while calls < a.reps:
        w, d, c = call(origin, a.page)
        calls += 1
        wall.append(w)
        dev.append(d)
        cost.add(c)
        got.append(keys[:32 * ne.value].copy())
        if not more.value:
            break
        okeep = nxt.copy()  # (next32 is overwritten by the call that reads it as its origin)
        origin = okeep.ctypes.data
    got = np.concatenate(got)
    assert got.tobytes() == whole_keys[:got.size].tobytes()
    res["paged"] = {"page": a.page, "calls": calls, "differences": got.size // 32, "wall_ms": stats(wall),
                    "stream_event_ms": stats(dev), "rounds_visited": sorted(cost)}
    # the baseline: both handles scanned completely, merged on the host
    chunk = 100_000
    rk = np.zeros(32 * chunk, np.uint8)
    rv = np.zeros(128 * chunk, np.uint8)
    ro = np.zeros(chunk + 1, np.uint64)

    def scan(h):
        out, origin = {}, None
        keep = None
        while True:
            check(lib().kh_trie_range_host(h, 0, origin, None, chunk, rk.ctypes.data, rv.ctypes.data, rv.size,
                                           ro.ctypes.data, ctypes.byref(ne), ctypes.byref(vb), ctypes.byref(more),
                                           nxt.ctypes.data, None))
            k = int(ne.value)
            kb, vbytes, o = rk[:32 * k].tobytes(), rv[:int(vb.value)].tobytes(), ro[:k + 1].tolist()
            for j in range(k):
                out[kb[32 * j:32 * j + 32]] = vbytes[o[j]:o[j + 1]]
            if not more.value:
                return out
            keep = nxt.copy()
            origin = keep.ctypes.data

    t0 = time.perf_counter()
    ca, cb = scan(base.h), scan(t.h)
    t1 = time.perf_counter()
    merged = sorted([k for k in ca if cb.get(k) != ca[k]] + [k for k in cb if k not in ca])
    t2 = time.perf_counter()
    assert b"".join(merged) == whole_keys.tobytes()
    res["baseline_scan_both_and_merge"] = {"calls": 1, "scan_ms": round(1e3 * (t1 - t0), 1),
                                           "merge_ms": round(1e3 * (t2 - t1), 1), "entries": len(ca) + len(cb)}
    res["baseline_over_whole_diff"] = round(1e3 * (t2 - t0) / res["whole"]["wall_ms"]["median"], 1)
    torch.cuda.synchronize()
    check(lib().kh_ctx_set_stream(ctx.h, None))
    for h in (t, base):
        h.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
