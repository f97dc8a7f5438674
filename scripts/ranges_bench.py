"""The batched range scan (kh_trie_ranges_host) against the single call, one GPU ("Batched
range scan").

  python scripts/ranges_bench.py [--out profiles/range_batch.json] [--bench-lines FILE]

Two handles, built once:
  - a forest of --tries ten-slot storage tries plus one trie of --big slots (the shape of
    scripts/range_verify_bench.py's mixed call, served instead of verified);
  - a hashed trie of --n synthetic accounts.
Legs, all in this one session, the median of --reps calls after 3 warm-ups, buffers allocated once
outside the clock; per leg the wall clock around the call(s), the event-to-event time on the
handle's stream (it spans the idle gaps while the host reads a round's counters) and the rounds
(khst_range_rounds):
  a  one batched call: the --tries whole tries plus a 1,000-entry tail of the big trie
  b  the same answer as --tries + 1 single kh_trie_range_host calls            (a's baseline)
  c  one batched call of --pages pages of --page entries at random origins of the account trie,
     against the same pages as --pages single calls                            (its baseline)
  d  nq = 1 batched against the single call, one page of --page entries
--bench-lines: a file of "LABEL {bench.py result line}" lines (the parent's build and this tree,
alternating), recorded beside the measurements.  One JSON object; nothing here is gated."""
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
    ap.add_argument("--tries", type=int, default=2000)
    ap.add_argument("--slots", type=int, default=10)
    ap.add_argument("--big", type=int, default=100_000)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--cfg", type=int, default=3)
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--page", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--bench-lines", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from khipu_amd._lib import KH_OK, check, lib
    from khipu_amd.device import Ctx, ResidentForest, ResidentTrie
    L = lib()
    L.khst_range_rounds.restype = ctypes.c_uint32
    warm = 3
    res = {"reps": a.reps, "warmups": warm}

    def stats(ts):
        ts = sorted(ts)
        return {"median": round(statistics.median(ts), 3), "min": round(ts[0], 3), "max": round(ts[-1], 3)}

    def timed(stream, call):
        """call() -> the rounds it took (the last scan's, or their sum); wall, stream events, rounds."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        wall, dev, rounds = [], [], []
        for i in range(a.reps + warm):
            with torch.cuda.stream(stream):
                e0.record()
                t0 = time.perf_counter()
                r = call()
                t1 = time.perf_counter()
                e1.record()
            e1.synchronize()
            if i >= warm:
                wall.append(1e3 * (t1 - t0))
                dev.append(e0.elapsed_time(e1))
                rounds.append(r)
        return {"wall_ms": stats(wall), "stream_event_ms": stats(dev), "rounds": sorted(set(rounds))}

    class Out:
        """Output buffers of a call of at most mx entries and nq requests."""

        def __init__(self, mx, nq, val_bytes):
            self.mx, self.nq = mx, nq
            self.keys = np.zeros(32 * mx, np.uint8)
            self.vals = np.zeros(val_bytes * mx, np.uint8)
            self.voff = np.zeros(mx + 1, np.uint64)
            self.eoff = np.zeros(nq + 1, np.uint64)
            self.nxt = np.zeros(32, np.uint8)
            self.ne, self.vb, self.nd = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
            self.more = ctypes.c_int(0)

    def batched(h, o, tries, origins, limits):
        rc = L.kh_trie_ranges_host(h, tries.ctypes.data if tries is not None else None,
                                   origins.ctypes.data if origins is not None else None,
                                   limits.ctypes.data if limits is not None else None, o.nq, o.mx, o.keys.ctypes.data,
                                   o.vals.ctypes.data, o.vals.size, o.voff.ctypes.data, o.eoff.ctypes.data,
                                   ctypes.byref(o.ne), ctypes.byref(o.vb), ctypes.byref(o.nd), o.nxt.ctypes.data, None)
        assert rc == KH_OK, rc
        return int(L.khst_range_rounds())

    def single(h, o, trie, origin, limit, mx):
        rc = L.kh_trie_range_host(h, trie, origin.ctypes.data if origin is not None else None,
                                  limit.ctypes.data if limit is not None else None, mx, o.keys.ctypes.data,
                                  o.vals.ctypes.data, o.vals.size, o.voff.ctypes.data, ctypes.byref(o.ne),
                                  ctypes.byref(o.vb), ctypes.byref(o.more), o.nxt.ctypes.data, None)
        assert rc == KH_OK, rc
        return int(L.khst_range_rounds())

    rnd = random.Random(5)

    def origin():  # in the lower 85 % of a uniform key space: a full page lies above it
        return np.frombuffer(rnd.randrange(int(0.85 * 2 ** 256)).to_bytes(32, "big"), np.uint8).copy()

    # ---- the storage forest: legs a and b
    nt, sl, tail = a.tries, a.slots, 1000
    g = np.random.default_rng(11)
    ctx = Ctx(0)
    f = ResidentForest(ctx, emit=False)
    big_id = nt + 1
    ups = [(t, g.bytes(32), b"\xa0" + g.bytes(32)) for t in range(1, nt + 1) for _ in range(sl)]
    ups += [(big_id, g.bytes(32), b"\xa0" + g.bytes(32)) for _ in range(a.big)]
    f.commit(ups)
    del ups
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    check(L.kh_ctx_set_stream(ctx.h, ctypes.c_void_p(stream.cuda_stream)))
    nq, mx = nt + 1, nt * sl + tail
    tries = np.arange(1, nq + 1, dtype=np.uint32)
    origins = np.zeros(32 * nq, np.uint8)
    tail_origin = origin()
    origins[32 * nt:] = tail_origin
    o = Out(mx, nq, 40)
    leg_a = timed(stream, lambda: batched(f.h, o, tries, origins, None))
    assert o.ne.value == mx and o.nd.value == nt and int(o.eoff[nt]) == nt * sl, (o.ne.value, o.nd.value)
    leg_a.update(requests=nq, entries=mx, value_bytes=int(o.vb.value))
    answer = (o.keys.tobytes(), o.vals[:int(o.vb.value)].tobytes())
    o1 = Out(tail, 1, 40)
    got = [[], []]

    def all_single(keep=False):
        r = 0
        for t in range(1, nt + 1):
            r += single(f.h, o1, t, None, None, tail)
            if keep:
                got[0].append(o1.keys[:32 * o1.ne.value].tobytes())
                got[1].append(o1.vals[:o1.vb.value].tobytes())
        r += single(f.h, o1, big_id, tail_origin, None, tail)
        if keep:
            got[0].append(o1.keys[:32 * o1.ne.value].tobytes())
            got[1].append(o1.vals[:o1.vb.value].tobytes())
        return r
    all_single(keep=True)
    assert (b"".join(got[0]), b"".join(got[1])) == answer  # the same answer
    leg_b = timed(stream, all_single)
    leg_b.update(calls=nq, note="rounds: the sum over the calls")
    res["storage_forest"] = {"tries": nt, "slots": sl, "big_trie_slots": a.big, "tail_entries": tail, "usage": f.usage(),
                             "a_one_batched_call": leg_a, "b_single_calls": leg_b,
                             "b_over_a_wall": round(leg_b["wall_ms"]["median"] / leg_a["wall_ms"]["median"], 2)}
    check(L.kh_ctx_set_stream(ctx.h, None))
    f.close()
    ctx.close()
    torch.cuda.empty_cache()

    # ---- the account trie: legs c and d
    ctx = Ctx(0)
    addr, vals, voff = ctx.synth_accounts(a.cfg, 0, a.n)
    t = ResidentTrie.__new__(ResidentTrie)
    t.ctx, t.dev, t.h = ctx, "cuda:0", None
    t._open(addr, 20, vals, voff, a.n, True, emit=False)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    check(L.kh_ctx_set_stream(ctx.h, ctypes.c_void_p(stream.cuda_stream)))
    np_, pg = a.pages, a.page
    ogs = sorted((origin() for _ in range(np_)), key=lambda x: x.tobytes())
    o1 = Out(pg, 1, 256)
    limits = np.zeros(32 * np_, np.uint8)
    pages = []
    for i, og in enumerate(ogs):  # the pages' last keys: the limits of the batched requests
        single(t.h, o1, 0, og, None, pg)
        assert o1.ne.value == pg and o1.more.value == 1
        limits[32 * i:32 * i + 32] = o1.keys[32 * (pg - 1):32 * pg]
        pages.append(o1.keys.tobytes())
    origins = np.concatenate(ogs)

    def pages_single():
        return sum(single(t.h, o1, 0, og, None, pg) for og in ogs)
    leg_c1 = timed(stream, pages_single)
    leg_c1.update(calls=np_, note="rounds: the sum over the calls")
    oc = Out(np_ * pg, np_, 256)
    leg_c = timed(stream, lambda: batched(t.h, oc, None, origins, limits))
    assert oc.ne.value == np_ * pg and oc.nd.value == np_ and oc.keys.tobytes() == b"".join(pages)
    leg_c.update(requests=np_, entries=np_ * pg, value_bytes=int(oc.vb.value))
    od = Out(pg, 1, 256)
    leg_d1 = timed(stream, lambda: single(t.h, o1, 0, ogs[0], None, pg))
    leg_d = timed(stream, lambda: batched(t.h, od, None, ogs[0], None))
    assert od.ne.value == pg and od.nd.value == 0 and od.keys.tobytes() == pages[0] and \
        od.nxt.tobytes() == o1.nxt.tobytes()
    res["account_trie"] = {"n_accounts": a.n, "cfg": a.cfg, "pages": np_, "page_entries": pg,
                           "c_one_batched_call": leg_c, "c_single_calls": leg_c1,
                           "c_single_over_batched_wall": round(leg_c1["wall_ms"]["median"] / leg_c["wall_ms"]["median"], 2),
                           "d_batched_nq1": leg_d, "d_single_call": leg_d1,
                           "d_batched_over_single_wall": round(leg_d["wall_ms"]["median"] / leg_d1["wall_ms"]["median"], 3)}
    t.close()
    check(L.kh_ctx_set_stream(ctx.h, None))
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


if __name__ == "__main__":
    main()
