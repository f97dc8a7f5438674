"""Subtrees of a resident trie evicted to stubs (kh_trie_evict_subtrees): what the call costs on a
1M-account handle, what it frees once compacted, and what the same end state costs today.

  python scripts/evict_bench.py [--accounts 1000000] [--reps 5] [--warmup 1] [--out FILE]

N synthetic accounts (csrc/synth.h, config 3) under hashed keys in a full resident trie.  Two calls,
each on a fresh kh_trie_copy of that handle per repetition (an eviction cannot be repeated on the
handle it changed):
  top_nibble  the 16 depth-2 prefixes under one top nibble, one call
  depth3      all 4,096 depth-3 prefixes, one call
with kh_trie_usage before and after, and the kh_trie_compact that follows.  Times are the wall clock
around the call and event to event on the handle's stream, medians after the warm-ups.  Nothing is
filled back.
Baseline (once, same session, for top_nibble's end state): kh_trie_prove with KH_PROVE_SHARED over
the keys to keep on the full handle, kh_trie_open_partial from that witness, and the HBM of both
handles held at once, which is what freeing the old one afterwards cannot avoid.
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

from khipu_amd import codec  # noqa: E402
from khipu_amd._lib import check, lib  # noqa: E402
from khipu_amd.device import Ctx, ResidentTrie  # noqa: E402
from tests.blocks import CFG, hash_keys  # noqa: E402

DEV = "cuda:0"


def med(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def timed(stream, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record(stream)
    r = fn()
    e1.record(stream)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1), r


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--accounts", type=int, default=1_000_000)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--nibble", type=int, default=7)
    p.add_argument("--no-baseline", action="store_true")
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
    stream = torch.cuda.Stream()  # the handles' calls run on their context's stream: one the events can be recorded on
    check(lib().kh_ctx_set_stream(ctx.h, ctypes.c_void_p(stream.cuda_stream)))
    top = keys.view(n, 32)[:, 0] >> 4
    under = int((top == a.nibble).sum().item())
    cases = {"top_nibble": [(a.nibble, b) for b in range(16)],
             "depth3": [(x, y, z) for x in range(16) for y in range(16) for z in range(16)]}
    res = {"accounts": n, "reps": a.reps, "warmup": a.warmup, "nibble": a.nibble, "root": full.root.hex(),
           "usage_full": full.usage()}
    for name, prefixes in cases.items():
        m = len(prefixes)
        pb = np.frombuffer(b"".join(codec.nibbles_to_path32(q) for q in prefixes), np.uint8).copy()
        db = np.asarray([len(q) for q in prefixes], np.uint8)
        status, hs = np.zeros(m, np.uint8), np.zeros(32 * m, np.uint8)
        cnt = [ctypes.c_uint64() for _ in range(3)]
        ew, ee, cw, ce = [], [], [], []
        for rep in range(a.warmup + a.reps):
            c = full.copy()
            u0 = c.usage()
            w, e, _ = timed(stream, lambda: check(lib().kh_trie_evict_subtrees(
                c.h, None, pb.ctypes.data, db.ctypes.data, m, status.ctypes.data, hs.ctypes.data, *map(ctypes.byref, cnt))))
            u1, size, stubs = c.usage(), len(c), c.stubs
            assert c.get_root() == full.root and size == n - cnt[1].value and stubs == cnt[0].value
            w2, e2, _ = timed(stream, c.compact)
            u2 = c.usage()
            assert c.get_root() == full.root and len(c) == size and c.stubs == stubs
            c.close()
            if rep >= a.warmup:
                ew.append(w), ee.append(e), cw.append(w2), ce.append(e2)
        if name == "top_nibble":
            assert cnt[1].value == under
        res[name] = {"prefixes": m, "status_counts": {str(s): int((status == s).sum()) for s in range(4)},
                     "evicted": cnt[0].value, "keys_evicted": cnt[1].value, "records_died": cnt[2].value,
                     "evict_wall_ms": med(ew), "evict_event_ms": med(ee), "compact_wall_ms": med(cw),
                     "compact_event_ms": med(ce), "usage_before": u0, "usage_after_evict": u1,
                     "usage_after_compact": u2}
    if not a.no_baseline:
        # today's way to the end state of top_nibble: prove the kept keys, open a second handle, free the first
        kb = keys.view(n, 32)[top != a.nibble].contiguous().reshape(-1).cpu().numpy().tobytes()
        kept = [kb[32 * i:32 * i + 32] for i in range(len(kb) // 32)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, _, table = full.prove(kept, shared=True)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        part = ResidentTrie.from_witness(ctx, full.root, table.nodes, emit=False)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        assert len(part) == n - under and part.get_root() == full.root
        up = part.usage()
        res["baseline_top_nibble"] = {"kept_keys": len(kept), "witness_nodes": len(table.nodes),
                                      "prove_shared_wall_ms": round((t1 - t0) * 1e3, 1),
                                      "from_witness_wall_ms": round((t2 - t1) * 1e3, 1),
                                      "total_wall_ms": round((t2 - t0) * 1e3, 1), "stubs": part.stubs,
                                      "usage_new_handle": up,
                                      "peak_hbm_bytes_both_handles": res["usage_full"]["hbm_bytes"] + up["hbm_bytes"],
                                      "note": "host arrays in and out, as a caller of the Python layer pays them; once"}
        part.close()
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
