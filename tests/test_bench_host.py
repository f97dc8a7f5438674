"""Host-side checks of bench.py's roofline plumbing (no GPU): the PMC traffic lookup
reads the committed per-size summary, and scripts/pmc_summary.py's --json argument is
not mistaken for the build count."""
import json
import os
import subprocess
import sys

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pmc_traffic_reads_committed_summary():
    t = bench.pmc_traffic("k_leaf_fused", 100_000_000)
    assert t is not None and t > 0
    # per launch: hbm_bytes / calls_per_build of the newest summary that has the kernel
    with open(os.path.join(ROOT, "profiles", "r1l_pmc_traffic_100000000.json")) as fh:
        row = json.load(fh)["kernels"]["k_leaf_fused"]
    assert abs(t - row["hbm_bytes"] / row["calls_per_build"]) < 1.0


def test_pmc_traffic_unknown_size_is_none():
    assert bench.pmc_traffic("k_leaf_fused", 12345) is None


def test_pmc_summary_json_arg(tmp_path):
    out = tmp_path / "t.json"
    r = subprocess.run([sys.executable, "scripts/pmc_summary.py", "no_such_tag", "--json", str(out)],
                       cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert "invalid literal" not in r.stderr
    assert r.returncode == 0, r.stderr
    with open(out) as fh:
        assert "kernels" in json.load(fh)


def test_pmc_round_order():
    """Newest summary by round number, not by file-name string order (r10a after r2a)."""
    names = ["profiles/r1l_pmc_traffic_5.json", "profiles/r10a_pmc_traffic_5.json", "profiles/r2b_pmc_traffic_5.json",
             "profiles/r2a_pmc_traffic_5.json"]
    assert sorted(names, key=bench.round_key)[-1].endswith("r10a_pmc_traffic_5.json")
    assert sorted(names, key=bench.round_key)[0].endswith("r1l_pmc_traffic_5.json")


def test_extrapolation_fit():
    """us/put = a + b*log16(n) through exact samples recovers a and b."""
    import math
    a, b = 3.0, 4.0
    samples = [(n, n * (a + b * math.log(n, 16)) * 1e-6) for n in (20000, 50000, 100000)]
    fa, fb, res = bench.fit_put_cost(samples)
    assert abs(fa - a) < 1e-6 and abs(fb - b) < 1e-6
    assert max(abs(r) for r in res) < 1e-6


def test_seq_root_hashes_keys_in_c(oracle):
    """mode 2 (keys hashed inside the C put loop) == hashing them first."""
    import numpy as np
    from khipu_amd import codec
    rnd = np.random.default_rng(5)
    addrs = [rnd.integers(0, 256, 20, dtype=np.uint8).tobytes() for _ in range(300)]
    vals = [codec.account_rlp(i, 10 ** 18 + i) for i in range(300)]
    vo = np.zeros(301, np.uint64)
    vo[1:] = np.cumsum([len(v) for v in vals])
    a = np.frombuffer(b"".join(addrs), np.uint8)
    vb = np.frombuffer(b"".join(vals), np.uint8)
    assert oracle.seq_root_packed(a, 20, vb, vo, 300, mode=2) == \
        oracle.seq_root([oracle.kec256(x) for x in addrs], vals)


def test_plain_run_has_no_extra_legs(monkeypatch):
    """Without --full the CPU legs and the host-buffer path are off; --full turns them on,
    and --no-cpu / --no-host-path still take single legs out of it."""
    def parse(*argv):
        monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
        return bench.parse()
    a = parse("--gpus", "1", "--steps", "3", "--warmup", "1")
    assert (a.steps, a.warmup, a.full, a.no_cpu, a.no_host_path, a.dump_outputs) == (3, 1, False, True, True, None)
    a = parse("--full")
    assert a.full and not a.no_cpu and not a.no_host_path and not a.no_cpu_batch
    a = parse("--full", "--no-cpu", "--dump-outputs", "d")
    assert a.full and a.no_cpu and not a.no_host_path and a.dump_outputs == "d"


def test_dump_outputs(tmp_path, monkeypatch):
    """--dump-outputs: bytes as float32, wider integers as float64, values exact; an array over
    its share of the budget becomes the same seeded sample of rows on every call."""
    import numpy as np
    r = np.random.default_rng(2)
    hh = r.integers(0, 256, (1, 32), dtype=np.uint8)
    ll = np.array([2 ** 32 - 1, 532], np.uint32)
    big = r.integers(0, 256, (1000, 32), dtype=np.uint8)
    monkeypatch.setattr(bench, "DUMP_BUDGET", 3 * 100 * 32 * 4)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"hash32": hh, "enc_len": ll, "big": big})
    got = {k: np.load(tmp_path / "a" / f"{k}.npy") for k in ("hash32", "enc_len", "big")}
    assert got["hash32"].dtype == np.float32 and (got["hash32"] == hh).all()
    assert got["enc_len"].dtype == np.float64 and (got["enc_len"] == ll).all()
    assert got["big"].dtype == np.float32 and got["big"].shape == (100, 32)
    assert sum(v.nbytes for v in got.values()) <= bench.DUMP_BUDGET
    rows = {x.tobytes() for x in big.astype(np.float32)}
    assert all(x.tobytes() in rows for x in got["big"])
    assert (np.load(tmp_path / "b" / "big.npy") == got["big"]).all()


def test_storage_ranges_balanced():
    """bench.py --workload storage: slot-balanced contiguous trie ranges cover every trie once."""
    import numpy as np
    r = np.random.default_rng(1)
    for nt, world in ((100_000, 8), (10, 16), (1, 4), (1000, 1), (5000, 3)):
        cnt = np.exp(r.uniform(0, np.log(10_001), nt)).astype(np.int64).clip(1, 10_000)
        so = np.concatenate([[0], np.cumsum(cnt)])
        b = bench.storage_ranges(so, world)
        assert b[0] == 0 and b[-1] == nt and all(b[g] <= b[g + 1] for g in range(world))
        slots = [int(so[b[g + 1]] - so[b[g]]) for g in range(world)]
        assert sum(slots) == int(so[-1])
        if nt >= 100 * world:
            assert max(slots) <= 1.02 * so[-1] / world + 10_000
