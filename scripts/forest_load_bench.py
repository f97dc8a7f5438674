"""Forest load, roots and eviction on synthetic storage tries ("Forest load and eviction").

  python scripts/forest_load_bench.py [--legs pagein,resume,evict] [--out profiles/NAME.json]

One GPU; every timed call is measured twice: host wall clock around the C ABI call and the
library's own HIP-event time (kh_stats.t_total_ms and its split).  Medians of --reps runs.
  pagein  2,000 tries of 10 slots loaded (kh_forest_load_nodes, the store already in HBM) into
          (a) an empty forest and (b) a forest already holding --resident tries of 10 slots (the
          loaded tries evicted again between runs); and the only way the library had before:
          one kh_trie_open_nodes_host call per trie, each given just that trie's own nodes.
  resume  --resume-tries tries of kh_dev_synth_storage's log-uniform sizes built by one commit,
          exported once as the store, loaded into a fresh forest: nodes/s and the split into
          store hashing + sort, rounds, anchor map.
  evict   half of --resident tries evicted, then kh_trie_compact.
  open    (not in the default legs) kh_trie_open_nodes, the store already in HBM, wall clock around
          the call, the handle freed after each: on the exported store of one trie of --slots
          slots and of a state trie of each of --open-accounts synthetic accounts.  A size whose
          open fails (out of memory) is recorded with its error.
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
    ap.add_argument("--legs", default="pagein,resume,evict")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--page-tries", type=int, default=2000)
    ap.add_argument("--slots", type=int, default=10)
    ap.add_argument("--resident", type=int, default=100_000)
    ap.add_argument("--resume-tries", type=int, default=10_000)
    ap.add_argument("--resume-reps", type=int, default=3)
    ap.add_argument("--cfg", type=int, default=4)
    ap.add_argument("--open-accounts", default="1000000,10000000")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from khipu_amd import _lib
    from khipu_amd._lib import KhStats, check, lib
    from khipu_amd.device import Ctx, ResidentForest, ResidentTrie, _ptr
    ctx = Ctx(0)
    dev = "cuda:0"
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    legs = a.legs.split(",")
    res = {"reps": a.reps}

    def random_forest(first_id, nt, slots, hash_keys=False):
        """nt tries of `slots` random 32-byte keys and 33-byte values, built by one commit."""
        n = nt * slots
        keys = torch.randint(0, 256, (n * 32 + 64,), generator=g, device=dev, dtype=torch.uint8)
        vals = torch.randint(0, 256, (n * 33 + 64,), generator=g, device=dev, dtype=torch.uint8)
        vals[0:n * 33:33] = 0xA0
        voff = torch.arange(n + 1, device=dev, dtype=torch.int64) * 33
        tid = (torch.arange(nt, device=dev, dtype=torch.int64) + first_id).repeat_interleave(slots).to(torch.int32)
        f = ResidentForest(ctx, hash_keys=hash_keys)
        commit(f, tid, keys, vals, voff, n, nt)
        return f

    def commit(f, tid, keys, vals, voff, n, nt):
        tries = np.zeros(nt + 1, np.uint32)
        roots = np.zeros(32 * (nt + 1), np.uint8)
        k = ctypes.c_uint64()
        torch.cuda.synchronize()
        check(lib().kh_forest_apply(f.h, _ptr(tid), _ptr(keys), _ptr(vals), _ptr(voff), n, None, None, 0, 32,
                                    tries.ctypes.data, roots.ctypes.data, nt + 1, ctypes.byref(k), None))

    def export_store(f, trie=None):
        """(encodings uint8, offsets uint64[n+1]) of the forest's node store, on the host."""
        encs, lens = [], []
        cur, done = f.export_cursor(), False
        node_cap, rlp_cap = 1 << 20, 256 << 20
        hs = np.zeros(32 * node_cap, np.uint8)
        rl = np.zeros(rlp_cap, np.uint8)
        of = np.zeros(node_cap + 1, np.uint64)
        nn, nl, dn = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_int(0)
        while not done:
            check(lib().kh_trie_export_nodes(f.h, _lib.KH_NO_TRIE if trie is None else trie, 0, ctypes.byref(cur),
                                             hs.ctypes.data, node_cap, rl.ctypes.data, rlp_cap, of.ctypes.data,
                                             ctypes.byref(nn), ctypes.byref(nl), ctypes.byref(dn)))
            encs.append(rl[:nl.value].copy())
            lens.append(np.diff(of[:nn.value + 1]).astype(np.uint64))
            done = bool(dn.value)
        enc = np.concatenate(encs) if encs else np.zeros(0, np.uint8)
        ln = np.concatenate(lens) if lens else np.zeros(0, np.uint64)
        off = np.zeros(len(ln) + 1, np.uint64)
        np.cumsum(ln, out=off[1:])
        return enc, off

    def to_dev(enc, off):
        e = torch.zeros(enc.size + 64, dtype=torch.uint8, device=dev)
        e[:enc.size] = torch.from_numpy(enc).to(dev)
        return e, torch.from_numpy(off.astype(np.int64)).to(dev)

    def load(f, ids, roots, d_enc, d_off, n):
        st = KhStats()
        nm = ctypes.c_uint64()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        check(lib().kh_forest_load_nodes(f.h, ids.ctypes.data, roots.ctypes.data, len(ids), _ptr(d_enc), _ptr(d_off), n,
                                         None, None, 0, ctypes.byref(nm), ctypes.byref(st)))
        return (time.perf_counter() - t0) * 1e3, st.t_total_ms, (st.t_sort_ms, st.t_branch_ms, st.t_topo_ms), st.n_levels

    def med(xs):
        return round(statistics.median(xs), 3)

    def summary(runs):
        return {"wall_ms_median": med([r[0] for r in runs]), "wall_ms_min": round(min(r[0] for r in runs), 3),
                "wall_ms_max": round(max(r[0] for r in runs), 3), "device_ms_median": med([r[1] for r in runs]),
                "store_hash_sort_ms": med([r[2][0] for r in runs]), "rounds_ms": med([r[2][1] for r in runs]),
                "map_ms": med([r[2][2] for r in runs]), "rounds": runs[0][3]}

    def id_root_arrays(roots):
        ids = np.asarray(list(roots), np.uint32)
        return ids, np.frombuffer(b"".join(roots[t] for t in roots), np.uint8).copy()

    if "pagein" in legs or "evict" in legs:
        big = random_forest(0, a.resident, a.slots)
    if "pagein" in legs:
        first = 1 << 24
        src = random_forest(first, a.page_tries, a.slots)
        roots = src.roots()
        ids, rb = id_root_arrays(roots)
        enc, off = export_store(src)
        n = len(off) - 1
        d_enc, d_off = to_dev(enc, off)
        leg = {"tries": a.page_tries, "slots": a.slots, "store_nodes": n, "store_bytes": int(enc.size)}
        runs = []
        for _ in range(a.reps + 1):  # (the first run sizes the workspaces: dropped)
            f = ResidentForest(ctx)
            runs.append(load(f, ids, rb, d_enc, d_off, n))
            assert f.roots() == roots
            f.close()
        leg["into_empty"] = summary(runs[1:])
        runs = []
        for _ in range(a.reps + 1):
            runs.append(load(big, ids, rb, d_enc, d_off, n))
            assert big.evict(list(roots)) == len(roots)
        leg["into_resident"] = dict(summary(runs[1:]), resident_tries=a.resident)
        leg["resident_over_empty"] = round(leg["into_resident"]["wall_ms_median"] / leg["into_empty"]["wall_ms_median"], 3)
        # the way before: one kh_trie_open_nodes_host per trie, each with its own nodes only
        per = [export_store(src, trie=int(t)) for t in ids]
        loops = []
        for _ in range(3):
            # (only the opens are timed; each handle is freed again at once: 2,000 live handles of
            # the host entry points would hold 2,000 private contexts)
            miss = np.zeros(32, np.uint8)
            torch.cuda.synchronize()
            spent = 0.0
            for j, (e, o) in enumerate(per):
                h = ctypes.c_void_p()
                t0 = time.perf_counter()
                check(lib().kh_trie_open_nodes_host(rb[32 * j:].ctypes.data, e.ctypes.data, o.ctypes.data, len(o) - 1,
                                                    0, miss.ctypes.data, ctypes.byref(h)))
                spent += time.perf_counter() - t0
                lib().kh_trie_free(h)
            loops.append(spent * 1e3)
        leg["open_nodes_host_loop_ms"] = [round(x, 1) for x in sorted(loops)]
        leg["loop_over_batched"] = round(statistics.median(loops) / leg["into_empty"]["wall_ms_median"], 1)
        res["pagein"] = leg
        src.close()
    if "evict" in legs:
        half = list(range(0, a.resident, 2))
        tb = np.asarray(half, np.uint32)
        n = ctypes.c_uint64()
        u0 = big.usage()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        check(lib().kh_forest_evict(big.h, tb.ctypes.data, len(half), ctypes.byref(n)))
        t1 = time.perf_counter()
        big.compact()
        t2 = time.perf_counter()
        u1 = big.usage()
        res["evict"] = {"resident_tries": a.resident, "evicted": int(n.value), "records_before": u0["records"],
                        "records_after_compact": u1["records"], "evict_ms": round((t1 - t0) * 1e3, 3),
                        "compact_ms": round((t2 - t1) * 1e3, 3)}
    if "pagein" in legs or "evict" in legs:
        big.close()
    if "resume" in legs:
        so, keys, vals, voff, seg = ctx.synth_storage(a.cfg, 0, a.resume_tries)
        nslots = seg.numel() - 16
        src = ResidentForest(ctx, hash_keys=True)
        commit(src, seg, keys, vals, voff, nslots, a.resume_tries)
        del keys, vals, voff, seg
        roots = src.roots()
        ids, rb = id_root_arrays(roots)
        t0 = time.perf_counter()
        enc, off = export_store(src)
        export_s = time.perf_counter() - t0
        recs = src.usage()["records"]
        src.close()
        n = len(off) - 1
        d_enc, d_off = to_dev(enc, off)
        runs = []
        for _ in range(a.resume_reps + 1):
            f = ResidentForest(ctx, hash_keys=True)
            runs.append(load(f, ids, rb, d_enc, d_off, n))
            assert len(f) == nslots and f.usage()["records"] == recs
            f.close()
        s = summary(runs[1:])
        res["resume"] = dict(s, tries=len(ids), slots=nslots, store_nodes=n, store_bytes=int(enc.size), records=recs,
                             export_s=round(export_s, 3), nodes_per_s=round(n / (s["wall_ms_median"] / 1e3)))
    if "open" in legs:
        def open_leg(src, root, nkeys, flags):
            enc, off = export_store(src)
            src.close()
            n = len(off) - 1
            d_enc, d_off = to_dev(enc, off)
            rb = np.frombuffer(root, np.uint8).copy()
            miss = np.zeros(32, np.uint8)
            leg = {"keys": nkeys, "store_nodes": n, "store_bytes": int(enc.size)}
            ms = []
            for _ in range(a.reps + 1):  # (the first run sizes the workspaces: dropped)
                h = ctypes.c_void_p()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                rc = lib().kh_trie_open_nodes(ctx.h, rb.ctypes.data, _ptr(d_enc), _ptr(d_off), n, flags,
                                              miss.ctypes.data, ctypes.byref(h))
                ms.append((time.perf_counter() - t0) * 1e3)
                if rc != _lib.KH_OK:
                    leg["error"] = [rc, lib().kh_last_error().decode(errors="replace")]
                    return leg
                size = ctypes.c_uint64()
                check(lib().kh_trie_size(h, ctypes.byref(size)))
                assert size.value == nkeys
                lib().kh_trie_free(h)
            leg.update(wall_ms_median=med(ms[1:]), wall_ms_min=round(min(ms[1:]), 3), wall_ms_max=round(max(ms[1:]), 3))
            return leg

        res["open"] = {}
        one = random_forest(0, 1, a.slots)
        res["open"][f"slots_{a.slots}"] = open_leg(one, one.roots()[0], a.slots, 0)
        for n in [int(x) for x in a.open_accounts.split(",") if x]:
            addr, vals, voff = ctx.synth_accounts(9, 0, n)
            t = ResidentTrie.__new__(ResidentTrie)
            t.ctx, t.dev, t.h = ctx, dev, None
            t._open(addr, 20, vals, voff, n, True, emit=False)
            del addr, vals, voff
            res["open"][f"accounts_{n}"] = open_leg(t, t.root, n, _lib.KH_HASH_KEYS)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
