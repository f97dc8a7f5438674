"""A state trie held as the witness of one block instead of whole (kh_trie_open_partial):
what it costs to open, what it saves in HBM, and what a block's commit costs on it.

  python scripts/partial_bench.py [--accounts 1000000] [--dirty 20000] [--reps 11] [--out FILE]

N synthetic accounts (csrc/synth.h, config 3) in a full resident trie; one configs[2]-shaped block
(90 % updates, 5 % inserts, 5 % deletes of `dirty` accounts); its witness = kh_trie_prove with
KH_PROVE_SHARED over the block's keys on the full handle.  The partial handle is opened from that
witness; what a delete's collapse still needs is fetched by hash from the full handle in the
reference's retry loop (kh_trie_missing -> kh_trie_nodes_by_hash -> kh_trie_fill_nodes) before
anything is timed.  The block is then timed on both handles as kh_trie_root_of (a journaled commit
and its rollback, so every repetition starts from the same version; the same root is required),
the median of `reps`, and once as a plain commit.  Prints one JSON line; --out also writes it.
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

from khipu_amd import _lib  # noqa: E402
from khipu_amd._lib import KhStats, check, lib  # noqa: E402
from khipu_amd.device import Ctx, ResidentForest, ResidentTrie, _pack_dev, _ptr  # noqa: E402
from tests.blocks import CFG, hash_keys  # noqa: E402

DEV = "cuda:0"


def rows(t, n):
    b = t[:32 * n].cpu().numpy().tobytes()
    return [b[32 * i:32 * i + 32] for i in range(n)]


def spans(vals, voff, n):
    o = voff[:n + 1].cpu().numpy()
    b = vals[:int(o[n])].cpu().numpy().tobytes()
    return [b[int(o[i]):int(o[i + 1])] for i in range(n)]


def timed(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        out.append(((time.perf_counter() - t0) * 1e3, r))
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--accounts", type=int, default=1_000_000)
    p.add_argument("--dirty", type=int, default=20_000)
    p.add_argument("--reps", type=int, default=11)
    p.add_argument("--out")
    a = p.parse_args()
    n, dirty = a.accounts, a.dirty
    nins = ndel = dirty // 20
    nupd = dirty - nins - ndel
    ctx = Ctx(0)
    g = torch.Generator(device=DEV)
    g.manual_seed(5)
    addr, vals, voff = ctx.synth_accounts(CFG, 0, n)
    keys = hash_keys(ctx, addr, 20, n)
    full = ResidentTrie.__new__(ResidentTrie)
    full.ctx, full.dev, full.h = ctx, DEV, None
    full._open(keys, 32, vals, voff, n, False, emit=False)
    # the block: updates of random accounts, fresh accounts, deletes from the tail
    idx = torch.randperm(n - ndel, generator=g, device=DEV)[:nupd]
    _, ub, uo = ctx.synth_accounts(CFG, 2 * 10**9, nupd)
    a2, ib, io = ctx.synth_accounts(CFG, 10**9, nins)
    ups = list(zip(rows(keys.view(n, 32)[idx].reshape(-1).contiguous(), nupd), spans(ub, uo, nupd)))
    ups += list(zip(rows(hash_keys(ctx, a2, 20, nins), nins), spans(ib, io, nins)))
    dels = rows(keys[32 * (n - ndel):].contiguous(), ndel)
    # its witness
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _, _, table = full.prove([k for k, _ in ups] + dels, shared=True)
    prove_ms = (time.perf_counter() - t0) * 1e3
    encs = table.nodes
    ed, eo = _pack_dev(encs, DEV)
    rb = np.frombuffer(full.root, np.uint8).copy()
    miss = np.zeros(32, np.uint8)

    def open_partial():
        h = ctypes.c_void_p()
        check(lib().kh_trie_open_partial(ctx.h, rb.ctypes.data, _ptr(ed), _ptr(eo), len(encs), 0, miss.ctypes.data,
                                         ctypes.byref(h)))
        return h
    opens = timed(open_partial, 3)
    for _, h in opens[:-1]:
        lib().kh_trie_free(h)
    part = ResidentTrie.__new__(ResidentTrie)
    part.ctx, part.dev, part.h, part.hash_keys, part.root = ctx, DEV, opens[-1][1], False, full.root
    # the same load through the forest entry point, for the library's own HIP-event time
    st = KhStats()
    f = ResidentForest(ctx)
    ids, nm = np.zeros(1, np.uint32), ctypes.c_uint64()
    check(lib().kh_forest_load_partial(f.h, ids.ctypes.data, rb.ctypes.data, 1, _ptr(ed), _ptr(eo), len(encs), None, None,
                                       0, ctypes.byref(nm), ctypes.byref(st)))
    f.close()
    stubs0, keys0 = part.stubs, len(part)
    # what the deletes' collapses still need: the reference's retry loop, untimed
    rounds = fetched = 0
    while True:
        try:
            want = part.root_of(ups, dels)
            break
        except _lib.MPTNodeMissingException:
            hs = [h for _, h in part.missing()]
            got = []
            for i in range(0, len(hs), 4096):
                got += full.nodes_by_hash(hs[i:i + 4096])
            assert all(e is not None for e in got)
            part.fill(got)
            rounds += 1
            fetched += len(hs)
    assert full.root_of(ups, dels) == want
    uk, _ = _pack_dev([k for k, _ in ups], DEV)
    uv, uoff = _pack_dev([v for _, v in ups], DEV)
    dk, _ = _pack_dev(dels, DEV)

    def root_of(t):
        root = np.zeros(32, np.uint8)
        check(lib().kh_trie_root_of(t.h, _ptr(uk), _ptr(uv), _ptr(uoff), len(ups), _ptr(dk), len(dels), 32, 0,
                                    root.ctypes.data, None))
        return root.tobytes()
    res = {}
    for name, t in (("full", full), ("partial", part)):
        root_of(t)  # warm-up
        ts = timed(lambda: root_of(t), a.reps)
        assert all(r == want for _, r in ts)
        res[name] = {"root_of_ms_median": statistics.median(x for x, _ in ts), "root_of_ms_min": min(x for x, _ in ts),
                     "hbm_bytes": t.usage()["hbm_bytes"], "records": t.usage()["live_records"]}
    for name, t in (("full", full), ("partial", part)):
        (ms, r), = timed(lambda: t.commit_dev(uk, uv, uoff, len(ups), dk, len(dels)), 1)
        assert r == want
        res[name]["commit_ms_once"] = ms
    out = {"accounts": n, "dirty": dirty, "updates": nupd, "inserts": nins, "deletes": ndel, "reps": a.reps,
           "witness_nodes": len(encs), "witness_bytes": sum(len(e) for e in encs), "prove_ms_wall": prove_ms,
           "open_partial_ms_wall": [x for x, _ in opens], "load_partial_event_ms": st.t_total_ms,
           "load_partial_rounds": st.n_levels, "stubs_after_open": stubs0, "keys_after_open": keys0,
           "fetch_rounds": rounds, "fetched_nodes": fetched, "stubs": part.stubs, "root": want.hex(), **res}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
