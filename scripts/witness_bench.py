"""The commit witness of a block's account batch (kh_trie_commit_witness_host): what the call costs
on a 1M-account handle, beside the shared proof of the same keys and the fetch loop it replaces.

  python scripts/witness_bench.py [--accounts 1000000] [--dirty 20000] [--reps 20] [--warmup 3] [--out FILE]

N synthetic accounts (csrc/synth.h, config 3) under hashed keys in a full resident trie, and one
account batch in the shape of configs[2] (tests/blocks.py): 90% updates of random accounts, 5%
inserts of fresh addresses, 5% deletes.  From one session, medians after the warm-ups of the wall
clock around each call and of stream events around it (both calls end in a synchronise):
  witness       kh_trie_commit_witness_host with buffers of exactly the sizes it reports
  prove_shared  kh_trie_prove(KH_PROVE_SHARED) over the same keys on the same handle: the yardstick,
                the witness being that work plus the join, the visited set and the depth rounds
and once: the handle opened from the witness commits the batch to the root kh_trie_root_of gives on
the full handle; the fetch loop of tests/test_gpu_partial.py::test_fetch_loop from a root-only
handle for the same batch -- its refusals and its total time, the nodes served from a dict.
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

from khipu_amd import _lib  # noqa: E402
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
    p.add_argument("--dirty", type=int, default=20_000)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--no-loop", action="store_true")
    p.add_argument("--out")
    a = p.parse_args()
    n = a.accounts
    nins = ndel = a.dirty // 20
    nupd = a.dirty - nins - ndel
    ctx = Ctx(0)
    addr, vals, voff = ctx.synth_accounts(CFG, 0, n)
    keys = hash_keys(ctx, addr, 20, n)
    full = ResidentTrie.__new__(ResidentTrie)
    full.ctx, full.dev, full.h = ctx, DEV, None
    full._open(keys, 32, vals, voff, n, False, emit=False)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()  # the handle's calls run on its context's stream: one the events can be recorded on
    check(lib().kh_ctx_set_stream(ctx.h, ctypes.c_void_p(stream.cuda_stream)))
    # the batch: updates of random accounts below the deleted tail, fresh addresses, the tail deleted
    g = torch.Generator(device=DEV)
    g.manual_seed(3)
    kk = keys.view(n, 32)
    upd = torch.randperm(n - ndel, generator=g, device=DEV)[:nupd]
    a2, _, _ = ctx.synth_accounts(CFG, 10**9, nins)
    ins = hash_keys(ctx, a2, 20, nins)
    up_keys = torch.cat([kk[upd].reshape(-1), ins]).contiguous().cpu().numpy()
    del_keys = kk[n - ndel:].reshape(-1).contiguous().cpu().numpy()
    nup = nupd + nins
    all_keys = np.concatenate([up_keys, del_keys])
    u64 = ctypes.c_uint64
    nn, nl, nc, nm = u64(0), u64(0), u64(0), u64(0)

    def witness(hs, rl, of, cn, cb):
        return lib().kh_trie_commit_witness_host(full.h, None, up_keys.ctypes.data, nup, None, del_keys.ctypes.data, ndel,
                                                 32, 0, hs.ctypes.data, cn, rl.ctypes.data, cb, of.ctypes.data,
                                                 ctypes.byref(nn), ctypes.byref(nl), ctypes.byref(nc), None, None, 0,
                                                 ctypes.byref(nm))
    one = np.zeros(1, np.uint8)
    assert witness(one, one, np.zeros(1, np.uint64), 0, 0) == _lib.KH_ENOSPC
    wn, wb = nn.value, nl.value
    hs, rl, of = np.zeros(32 * wn, np.uint8), np.zeros(wb, np.uint8), np.zeros(wn + 1, np.uint64)
    ww, we = [], []
    for rep in range(a.warmup + a.reps):
        w, e, rc = timed(stream, lambda: witness(hs, rl, of, wn, wb))
        check(rc)
        if rep >= a.warmup:
            ww.append(w), we.append(e)
    ncol = nc.value
    wit = {hs[32 * j:32 * j + 32].tobytes(): rl[int(of[j]):int(of[j + 1])].tobytes() for j in range(wn)}
    # the yardstick: the shared proof table of the same keys
    nk = nup + ndel
    found, po = np.zeros(nk, np.uint8), np.zeros(nk + 1, np.uint64)
    pn, pl, pp = u64(0), u64(0), u64(0)

    def prove(ph, pr, pf, pi, cn, cb, cp):
        return lib().kh_trie_prove(full.h, None, all_keys.ctypes.data, 32, nk, _lib.KH_PROVE_SHARED, found.ctypes.data,
                                   ph.ctypes.data, cn, pr.ctypes.data, cb, pf.ctypes.data, pi.ctypes.data, cp,
                                   po.ctypes.data, ctypes.byref(pn), ctypes.byref(pl), ctypes.byref(pp))
    assert prove(one, one, np.zeros(1, np.uint64), np.zeros(1, np.uint32), 0, 0, 0) == _lib.KH_ENOSPC
    cn, cb, cp = pn.value, pl.value, pp.value
    ph, pr, pf, pi = np.zeros(32 * cn, np.uint8), np.zeros(cb, np.uint8), np.zeros(cn + 1, np.uint64), np.zeros(cp, np.uint32)
    pw, pe = [], []
    for rep in range(a.warmup + a.reps):
        w, e, rc = timed(stream, lambda: prove(ph, pr, pf, pi, cn, cb, cp))
        check(rc)
        if rep >= a.warmup:
            pw.append(w), pe.append(e)
    assert wn == cn + ncol
    res = {"accounts": n, "ops": nk, "upserts": nup, "deletes": ndel, "reps": a.reps, "warmup": a.warmup,
           "root": full.root.hex(), "witness_nodes": wn, "witness_bytes": wb, "n_collapse": ncol,
           "witness_wall_ms": med(ww), "witness_event_ms": med(we),
           "prove_shared_nodes": cn, "prove_shared_bytes": cb, "prove_shared_path_entries": cp,
           "prove_shared_wall_ms": med(pw), "prove_shared_event_ms": med(pe),
           "witness_over_prove_wall": round(statistics.median(ww) / statistics.median(pw), 3),
           "witness_over_prove_event": round(statistics.median(we) / statistics.median(pe), 3)}
    if not a.no_loop:
        # once: the batch over its witness, and the root-only fetch loop for the same batch
        body = b"\xf8\x44" + bytes(68)  # (any value: neither the witness nor the loop's requests depend on it)
        ups = [(up_keys[32 * i:32 * i + 32].tobytes(), body) for i in range(nup)]
        dels = [del_keys[32 * i:32 * i + 32].tobytes() for i in range(ndel)]
        want = full.root_of(ups, dels)
        t = ResidentTrie.from_witness(ctx, full.root, wit, emit=False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = t.commit(ups, dels)
        torch.cuda.synchronize()
        res["commit_over_witness_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        assert got == want and t.missing() == []
        t.close()
        t = ResidentTrie.from_witness(ctx, full.root, {full.root: wit[full.root]}, emit=False)
        refusals, fetched = 0, 1
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        while True:
            try:
                got = t.commit(ups, dels)
                break
            except _lib.MPTNodeMissingException:
                refusals += 1
                need = {h: wit[h] for _, h in t.missing()}
                fetched += len(need)
                t.fill(need)
        torch.cuda.synchronize()
        res["fetch_loop"] = {"refusals": refusals, "nodes_fetched": fetched,
                             "total_wall_ms": round((time.perf_counter() - t0) * 1e3, 1),
                             "note": "once; nodes served from a host dict, no store round trip"}
        assert got == want and fetched == wn
        t.close()
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
