"""The batched trie diff (kh_trie_diffs_host) against the single call, one GPU ("Batched
trie diff").

  python scripts/diffs_bench.py [--out profiles/trie_diffs.json] [--bench-lines FILE]

Legs, all in this one session, the median of --reps calls after 3 warm-ups, host buffers allocated
once outside the clock; per leg the wall clock around the call(s), the event-to-event time on the
handle's stream (it spans the idle gaps while the host reads a round's counters), the rounds and the
selected items (khst_diffs_* / khst_diff_*):
  the block workload   a forest of --tries ten-slot storage tries plus one trie of --big slots
                       (scripts/ranges_bench.py's forest), its copy(), and one block on the original
                       that changes --changed slots in each small trie and --big-changed in the large
                       one; the copy is side a, the original side b
    a  all --tries + 1 pairs in one kh_trie_diffs_host call
    b  the same answer, compared byte for byte, as --tries + 1 kh_trie_diff_host calls (the baseline)
  one pair             nq = 1 batched against the single call on scripts/diff_bench.py's pair: --n
                       synthetic accounts, a block of 18,000 updates, 1,000 inserts and 1,000 deletes
--bench-lines: a file of "LABEL {bench.py result line}" lines (the parent's build and this tree,
alternating), recorded beside the measurements.  One JSON object; nothing here is gated."""
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
    ap.add_argument("--tries", type=int, default=2000)
    ap.add_argument("--slots", type=int, default=10)
    ap.add_argument("--big", type=int, default=100_000)
    ap.add_argument("--changed", type=int, default=3)
    ap.add_argument("--big-changed", type=int, default=1000)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--cfg", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--bench-lines", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from khipu_amd._lib import KH_OK, check, lib
    from khipu_amd.device import Ctx, ResidentForest, ResidentTrie, diff_counters, diffs_counters
    L = lib()
    warm = 3
    res = {"reps": a.reps, "warmups": warm}

    def stats(ts):
        ts = sorted(ts)
        return {"median": round(statistics.median(ts), 3), "min": round(ts[0], 3), "max": round(ts[-1], 3)}

    def timed(stream, call):
        """call() -> (rounds, visited) it took (the last call's, or their sums); wall, stream events, cost."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        wall, dev, cost = [], [], set()
        for i in range(a.reps + warm):
            with torch.cuda.stream(stream):
                e0.record()
                t0 = time.perf_counter()
                c = call()
                t1 = time.perf_counter()
                e1.record()
            e1.synchronize()
            if i >= warm:
                wall.append(1e3 * (t1 - t0))
                dev.append(e0.elapsed_time(e1))
                cost.add(c)
        return {"wall_ms": stats(wall), "stream_event_ms": stats(dev), "rounds_visited": sorted(cost)}

    class Out:
        """Output buffers of a call of at most mx differences and nq requests."""

        def __init__(self, mx, nq, val_bytes):
            self.mx, self.nq = mx, nq
            self.keys = np.zeros(32 * mx, np.uint8)
            self.kinds = np.zeros(mx, np.uint8)
            self.vals = np.zeros(val_bytes * mx, np.uint8)
            self.voff = np.zeros(mx + 1, np.uint64)
            self.eoff = np.zeros(nq + 1, np.uint64)
            self.nxt = np.zeros(32, np.uint8)
            self.ne, self.vb, self.nd = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
            self.more = ctypes.c_int(0)

    def batched(ha, hb, o, tries):
        rc = L.kh_trie_diffs_host(ha, tries.ctypes.data if tries is not None else None, hb, None, None, None, o.nq, o.mx,
                                  o.vals.size, o.keys.ctypes.data, o.kinds.ctypes.data, o.vals.ctypes.data,
                                  o.voff.ctypes.data, o.eoff.ctypes.data, ctypes.byref(o.ne), ctypes.byref(o.vb),
                                  ctypes.byref(o.nd), o.nxt.ctypes.data, None)
        assert rc == KH_OK, rc
        return diffs_counters()

    def single(ha, hb, o, trie):
        rc = L.kh_trie_diff_host(ha, trie, hb, trie, None, None, o.mx, o.vals.size, o.keys.ctypes.data,
                                 o.kinds.ctypes.data, o.vals.ctypes.data, o.voff.ctypes.data, ctypes.byref(o.ne),
                                 ctypes.byref(o.vb), ctypes.byref(o.more), o.nxt.ctypes.data, None)
        assert rc == KH_OK and not o.more.value, rc
        return diff_counters()

    # ---- the block workload
    nt, sl = a.tries, a.slots
    g = np.random.default_rng(11)
    ctx = Ctx(0)
    f = ResidentForest(ctx, emit=False)
    big_id = nt + 1
    small = [(t, g.bytes(32), b"\xa0" + g.bytes(32)) for t in range(1, nt + 1) for _ in range(sl)]
    big = [(big_id, g.bytes(32), b"\xa0" + g.bytes(32)) for _ in range(a.big)]
    f.commit(small + big)
    parent = f.copy()
    assert parent.roots() == f.roots()
    # the block: in each small trie one slot rewritten, one deleted, one new (a.changed = 3: else
    # rewrites alone); in the large trie a.big_changed slots rewritten
    ups, dels = [], []
    for t in range(1, nt + 1):
        mine = small[(t - 1) * sl:t * sl]
        if a.changed == 3 and sl >= 2:
            ups += [(t, mine[0][1], b"\xa0" + g.bytes(32)), (t, g.bytes(32), b"\xa0" + g.bytes(32))]
            dels.append((t, mine[1][1]))
        else:
            ups += [(t, k, b"\xa0" + g.bytes(32)) for _, k, _ in mine[:a.changed]]
    ups += [(big_id, k, b"\xa0" + g.bytes(32)) for _, k, _ in big[:a.big_changed]]
    f.commit(ups, dels)
    n_diff = nt * a.changed + a.big_changed
    del small, big, ups, dels
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    check(L.kh_ctx_set_stream(ctx.h, ctypes.c_void_p(stream.cuda_stream)))
    nq = nt + 1
    tries = np.arange(1, nq + 1, dtype=np.uint32)
    o = Out(n_diff + 16, nq, 40)
    leg_a = timed(stream, lambda: batched(parent.h, f.h, o, tries))
    assert o.ne.value == n_diff and o.nd.value == nq, (o.ne.value, o.nd.value)
    leg_a.update(requests=nq, differences=n_diff, value_bytes=int(o.vb.value),
                 answer_bytes=int(33 * n_diff + o.vb.value + 8 * (n_diff + 1) + 8 * (nq + 1)))
    answer = (o.keys[:32 * n_diff].tobytes(), o.kinds[:n_diff].tobytes(), o.vals[:int(o.vb.value)].tobytes())
    o1 = Out(a.big_changed + 16, 1, 40)
    got = [[], [], []]

    def all_single(keep=False):
        r = v = 0
        for t in range(1, nq + 1):
            c = single(parent.h, f.h, o1, t)
            r, v = r + c[0], v + c[1]
            if keep:
                got[0].append(o1.keys[:32 * o1.ne.value].tobytes())
                got[1].append(o1.kinds[:o1.ne.value].tobytes())
                got[2].append(o1.vals[:o1.vb.value].tobytes())
        return r, v
    all_single(keep=True)
    assert tuple(b"".join(x) for x in got) == answer  # the same answer, byte for byte
    leg_b = timed(stream, all_single)
    leg_b.update(calls=nq, note="rounds_visited: the sums over the calls")
    res["block_workload"] = {"tries": nt, "slots": sl, "big_trie_slots": a.big, "changed_per_small_trie": a.changed,
                             "changed_in_big_trie": a.big_changed, "usage": f.usage(), "a_one_batched_call": leg_a,
                             "b_single_calls": leg_b,
                             "b_over_a_wall": round(leg_b["wall_ms"]["median"] / leg_a["wall_ms"]["median"], 2)}
    check(L.kh_ctx_set_stream(ctx.h, None))
    for h in (f, parent):
        h.close()
    ctx.close()
    torch.cuda.empty_cache()

    # ---- one pair: scripts/diff_bench.py's 1M-account pair
    n, nu, ni, nd = a.n, 18_000, 1_000, 1_000
    ctx = Ctx(0)
    addr, vals, voff = ctx.synth_accounts(a.cfg, 0, n + ni)
    t = ResidentTrie.__new__(ResidentTrie)
    t.ctx, t.dev, t.h, t.hash_keys = ctx, "cuda:0", None, True
    t._open(addr, 20, vals, voff, n, True, emit=False)
    base = t.copy()
    off = voff.cpu().numpy()
    up_keys = torch.cat([addr[:20 * nu], addr[20 * n:20 * (n + ni)]]).contiguous()
    up_vals = torch.cat([vals[int(off[nu]):int(off[2 * nu])], vals[int(off[n]):int(off[n + ni])]]).contiguous()
    uo = np.concatenate([off[nu:2 * nu] - off[nu], off[n:n + ni + 1] - off[n] + (off[2 * nu] - off[nu])]).astype(np.int64)
    t.commit_dev(up_keys, up_vals, torch.from_numpy(uo).to("cuda:0"), nu + ni, addr[20 * (n - nd):20 * n].contiguous(), nd,
                 klen=20)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    check(L.kh_ctx_set_stream(ctx.h, ctypes.c_void_p(stream.cuda_stream)))
    one = {}
    for label, mx in (("whole", 1 << 16), ("page_1000", 1000)):
        os_, ob_ = Out(mx, 1, 128), Out(mx, 1, 128)
        leg_s = timed(stream, lambda: single_page(L, base.h, t.h, os_, diff_counters))
        leg_1 = timed(stream, lambda: batched(base.h, t.h, ob_, None))
        k = int(os_.ne.value)
        assert ob_.ne.value == k and ob_.keys[:32 * k].tobytes() == os_.keys[:32 * k].tobytes() and \
            ob_.vals[:ob_.vb.value].tobytes() == os_.vals[:os_.vb.value].tobytes() and \
            (ob_.nd.value == 0) == bool(os_.more.value)
        one[label] = {"max_entries": mx, "differences": k, "single_call": leg_s, "batched_nq1": leg_1,
                      "batched_over_single_wall": round(leg_1["wall_ms"]["median"] / leg_s["wall_ms"]["median"], 3)}
    res["one_pair"] = {"n_accounts": n, "cfg": a.cfg, "block": {"updates": nu, "inserts": ni, "deletes": nd}, **one}
    check(L.kh_ctx_set_stream(ctx.h, None))
    for h in (t, base):
        h.close()
    ctx.close()
    if a.bench_lines and os.path.exists(a.bench_lines):
        rows = []
        with open(a.bench_lines) as fh:
            for ln in fh:
                label, _, js = ln.strip().partition(" ")
                if js.startswith("{"):
                    d = json.loads(js)
                    rows.append({"build": label, "ms_per_step": round(d["ms_per_step"], 3),
                                 "device_ms_per_step": d.get("device_ms_per_step"), "state_root": d.get("state_root")})
        res["hot_path_bench"] = {"command": "bench.py --gpus 1 --steps 5 --warmup 2 --no-cpu --no-host-path",
                                 "runs_in_order": rows}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


def single_page(L, ha, hb, o, counters):
    """One kh_trie_diff_host page of the single pair (more may be set)."""
    rc = L.kh_trie_diff_host(ha, 0, hb, 0, None, None, o.mx, o.vals.size, o.keys.ctypes.data, o.kinds.ctypes.data,
                             o.vals.ctypes.data, o.voff.ctypes.data, ctypes.byref(o.ne), ctypes.byref(o.vb),
                             ctypes.byref(o.more), o.nxt.ctypes.data, None)
    assert rc == 0, rc
    return counters()


if __name__ == "__main__":
    main()
