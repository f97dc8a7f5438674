"""Changes since a savepoint against what it replaces, on resident state tries of synthetic accounts,
hashed keys ("Changes since a savepoint").

  python scripts/changes_bench.py --n 1000000 10000000 --out profiles/changes_since.json

On one GPU, per trie size N: a handle of N accounts; then per block (18,000 updates, 1,000 inserts,
1,000 deletes, every block other keys), warm, buffers allocated once outside the clock:
  - what callers did at the parent commit's interface: kh_trie_copy of the trie before the block (the
    wall clock around the call and a device synchronise; the HBM the copy holds, kh_trie_usage), the
    block committed, kh_trie_diff_host of the copy against the handle;
  - this call: a savepoint before the block, kh_trie_changes_since_host after it -- in the same
    session on the same handle and block, the two answers compared key by key, kind by kind.
The median, min and max of --reps blocks after 3 warm-up blocks of each wall clock (both calls end in
a stream synchronise of their own).  The work of changes-since follows the journal, so its time at
the sizes given should agree; the ratio is reported.  One JSON object; nothing here is gated."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def stats(ts):
    ts = sorted(ts)
    return {"median": round(statistics.median(ts), 3), "min": round(ts[0], 3), "max": round(ts[-1], 3)}


def one_size(a, n):
    import torch
    from khipu_amd._lib import check, lib
    from khipu_amd.device import Ctx, ResidentTrie, changes_counters
    nu, ni, nd = a.updates, a.inserts, a.deletes
    blocks = a.reps + 3
    assert blocks * (nu + nd) + 2 * nu <= n
    ctx = Ctx(0)
    addr, vals, voff = ctx.synth_accounts(a.cfg, 0, n + blocks * ni)
    off = voff.cpu().numpy().astype(np.int64)
    t = ResidentTrie.__new__(ResidentTrie)
    t.ctx, t.dev, t.h, t.hash_keys = ctx, "cuda:0", None, True
    t._open(addr, 20, vals, voff, n, True, emit=False)
    cap = 1 << 16
    assert nu + ni + nd < cap
    out = [dict(keys=np.zeros(32 * cap, np.uint8), kinds=np.zeros(cap, np.uint8), vbuf=np.zeros(128 * cap, np.uint8),
                vo=np.zeros(cap + 1, np.uint64)) for _ in range(2)]
    tries = np.zeros(cap, np.uint32)
    nxt = np.zeros(32, np.uint8)
    ne, vb, tot, more, nt = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_int(0), ctypes.c_uint32(0)
    t_copy, t_diff, t_chg, t_commit, hbm, ndiff, sorts = [], [], [], [], set(), [], set()

    def span(lo, hi):
        return vals[int(off[lo]):int(off[hi])], off[lo:hi + 1] - off[lo]

    for b in range(blocks):
        # the block: accounts [b nu, (b + 1) nu) take the values of accounts further on, accounts
        # [n + b ni, n + (b + 1) ni) are new, nd accounts from the end go
        u0, src, i0, d1 = b * nu, blocks * nu + b * 7, n + b * ni, n - b * nd
        uv, uo = span(src, src + nu)
        iv, io = span(i0, i0 + ni)
        up_keys = torch.cat([addr[20 * u0:20 * (u0 + nu)], addr[20 * i0:20 * (i0 + ni)]]).contiguous()
        up_vals = torch.cat([uv, iv]).contiguous()
        up_voff = torch.from_numpy(np.concatenate([uo, io[1:] + uo[-1]]).astype(np.int64)).to("cuda:0")
        del_keys = addr[20 * (d1 - nd):20 * d1].contiguous()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        base = t.copy()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        t.savepoint()
        t2 = time.perf_counter()
        t.commit_dev(up_keys, up_vals, up_voff, nu + ni, del_keys, nd, klen=20)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        o = out[0]
        check(lib().kh_trie_changes_since_host(t.h, 0, 0, 0, None, cap, o["vbuf"].size, tries.ctypes.data,
                                               o["keys"].ctypes.data, o["kinds"].ctypes.data, o["vbuf"].ctypes.data,
                                               o["vo"].ctypes.data, ctypes.byref(ne), ctypes.byref(vb), ctypes.byref(tot),
                                               ctypes.byref(more), ctypes.byref(nt), nxt.ctypes.data))
        t4 = time.perf_counter()
        k, kb = int(ne.value), int(vb.value)
        assert more.value == 0 and tot.value == k
        o = out[1]
        t5 = time.perf_counter()
        check(lib().kh_trie_diff_host(base.h, 0, t.h, 0, None, None, cap, o["vbuf"].size, o["keys"].ctypes.data,
                                      o["kinds"].ctypes.data, o["vbuf"].ctypes.data, o["vo"].ctypes.data, ctypes.byref(ne),
                                      ctypes.byref(vb), ctypes.byref(more), nxt.ctypes.data, None))
        t6 = time.perf_counter()
        assert (int(ne.value), int(vb.value), more.value) == (k, kb, 0), (ne.value, k)
        for f, m in (("keys", 32 * k), ("kinds", k), ("vbuf", kb), ("vo", k + 1)):
            assert out[0][f][:m].tobytes() == out[1][f][:m].tobytes(), f
        hist = np.bincount(out[0]["kinds"][:k], minlength=4)
        assert (int(hist[1]), int(hist[2])) == (nd, ni) and 0.99 * nu <= int(hist[3]) <= nu, hist
        if b >= 3:
            t_copy.append(1e3 * (t1 - t0))
            t_commit.append(1e3 * (t3 - t2))
            t_chg.append(1e3 * (t4 - t3))
            t_diff.append(1e3 * (t6 - t5))
            hbm.add(base.usage()["hbm_bytes"])
            ndiff.append(k)
            sorts.add(changes_counters())
        t.release()
        base.close()
    res = {"n_accounts": n, "blocks": a.reps, "differences": stats(ndiff), "radix_sorts_a_call": sorted(sorts),
           "changes_since_ms": stats(t_chg), "copy_ms": stats(t_copy), "diff_against_copy_ms": stats(t_diff),
           "commit_under_savepoint_ms": stats(t_commit), "copy_hbm_bytes": max(hbm), "usage": t.usage()}
    res["copy_plus_diff_over_changes_since"] = round(
        (res["copy_ms"]["median"] + res["diff_against_copy_ms"]["median"]) / res["changes_since_ms"]["median"], 1)
    t.close()
    del addr, vals, voff
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--cfg", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--updates", type=int, default=18_000)
    ap.add_argument("--inserts", type=int, default=1_000)
    ap.add_argument("--deletes", type=int, default=1_000)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    res = {"cfg": a.cfg, "block": {"updates": a.updates, "inserts": a.inserts, "deletes": a.deletes},
           "sizes": [one_size(a, n) for n in a.n]}
    if len(res["sizes"]) > 1:
        lo, hi = res["sizes"][0], res["sizes"][-1]
        res["changes_since_ms_ratio_last_over_first"] = round(
            hi["changes_since_ms"]["median"] / lo["changes_since_ms"]["median"], 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
