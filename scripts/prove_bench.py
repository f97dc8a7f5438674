"""Merkle proofs on a resident state trie of N synthetic accounts.

  python scripts/prove_bench.py --n 1000000 [--dict] --out profiles/NAME.json

Measures, on one GPU, warm wall clock around the C ABI calls (buffers allocated once, outside,
sized by a first KH_ENOSPC call):
  - kh_trie_prove of 1, 400 and 20,000 account addresses spread over the trie, plain and with
    KH_PROVE_SHARED: median and spread of --reps calls, nodes, bytes and path entries returned;
  - kh_verify_proofs of what kh_trie_prove returned (one root, KH_HASH_KEYS);
  - with --dict, the stated baseline: the same proofs assembled on the host by walking a Python
    dict of the exported store from the root (keys hashed beforehand, outside the clock).
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--counts", default="1,400,20000")
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
    counts = [int(c) for c in a.counts.split(",")]
    addrs = addr[:a.n * 20].view(-1, 20)
    picks = {c: addrs[torch.linspace(0, a.n - 1, c, dtype=torch.float64, device=addrs.device).long()].cpu().numpy().copy()
             for c in counts}
    del addr, vals, voff, addrs
    root = np.frombuffer(t.root, np.uint8).copy()
    res = {"n_accounts": a.n, "cfg": a.cfg, "open_s": round(open_s, 3), "usage": t.usage(), "reps": a.reps}
    nn, nl, npth, need = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)

    def ms(ts):
        ts = sorted(ts)
        return {"ms_median": round(1e3 * statistics.median(ts), 3), "ms_min": round(1e3 * ts[0], 3),
                "ms_max": round(1e3 * ts[-1], 3)}

    kept = {}
    for c in counts:
        kb = picks[c]
        for shared in (False, True):
            flags = _lib.KH_PROVE_SHARED if shared else 0
            found = np.zeros(c, np.uint8)
            po = np.zeros(c + 1, np.uint64)
            rc = lib().kh_trie_prove(t.h, None, kb.ctypes.data, 20, c, flags, found.ctypes.data, None, 0, None, 0, None,
                                     None, 0, po.ctypes.data, ctypes.byref(nn), ctypes.byref(nl), ctypes.byref(npth))
            assert rc == _lib.KH_ENOSPC, rc
            cn, cb, cp = nn.value, nl.value, npth.value
            hs = np.zeros(32 * cn, np.uint8)
            rl = np.zeros(cb, np.uint8)
            of = np.zeros(cn + 1, np.uint64)
            pi = np.zeros(cp, np.uint32)

            def prove():
                t0 = time.perf_counter()
                check(lib().kh_trie_prove(t.h, None, kb.ctypes.data, 20, c, flags, found.ctypes.data, hs.ctypes.data, cn,
                                          rl.ctypes.data, cb, of.ctypes.data, pi.ctypes.data, cp, po.ctypes.data,
                                          ctypes.byref(nn), ctypes.byref(nl), ctypes.byref(npth)))
                return time.perf_counter() - t0
            for _ in range(3):
                prove()
            assert int(found.sum()) == c
            name = f"prove_{c}" + ("_shared" if shared else "")
            res[name] = dict(ms([prove() for _ in range(a.reps)]), nodes=cn, rlp_bytes=cb, path_entries=cp)
            status = np.zeros(c, np.uint8)
            vo = np.zeros(c + 1, np.uint64)
            rc = lib().kh_verify_proofs(root.ctypes.data, 1, kb.ctypes.data, 20, c, _lib.KH_HASH_KEYS, rl.ctypes.data,
                                        of.ctypes.data, cn, pi.ctypes.data, po.ctypes.data, status.ctypes.data, None, 0,
                                        vo.ctypes.data, ctypes.byref(need))
            assert rc == _lib.KH_ENOSPC, rc
            vv = np.zeros(need.value, np.uint8)

            def verify():
                t0 = time.perf_counter()
                check(lib().kh_verify_proofs(root.ctypes.data, 1, kb.ctypes.data, 20, c, _lib.KH_HASH_KEYS,
                                             rl.ctypes.data, of.ctypes.data, cn, pi.ctypes.data, po.ctypes.data,
                                             status.ctypes.data, vv.ctypes.data, vv.size, vo.ctypes.data,
                                             ctypes.byref(need)))
                return time.perf_counter() - t0
            for _ in range(3):
                verify()
            assert int((status == _lib.KH_PROOF_VALUE).sum()) == c
            res["verify" + name[5:]] = dict(ms([verify() for _ in range(a.reps)]), value_bytes=int(need.value))
            if not shared:
                kept[c] = [[rl[int(of[j]):int(of[j + 1])].tobytes() for j in pi[int(po[i]):int(po[i + 1])]]
                           for i in range(min(c, 400))]
    if a.dict:
        from oracle import oracle
        from tests import proof_ref
        store = dict(t.export_nodes(node_cap=1 << 20, rlp_cap=256 << 20))
        rootb = t.root
        for c in counts:
            hk = [oracle.kec256(picks[c][i].tobytes()) for i in range(c)]
            ds = []
            for _ in range(max(a.reps // 4, 3)):
                t0 = time.perf_counter()
                got = [proof_ref.expected_proof(store, rootb, k)[0] for k in hk]
                ds.append(time.perf_counter() - t0)
            assert got[:400] == kept[c]
            res[f"dict_{c}"] = dict(ms(ds), entries=len(store))
    t.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
