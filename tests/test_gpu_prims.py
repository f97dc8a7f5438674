"""GPU: prims.h's radix sort and exclusive scans and wave.h's helpers against plain host code,
primitive by primitive (scripts/prims_check, built by __graft_entry__.build(); its case table
is checked by tests/test_prims_plan.py).  One process per device mode; a failing case is
reported as the program's own JSON line: which primitive, which n, which bit range, the first
differing position.  The launch counts the program keeps per kernel prove that the mode ran
every kernel form it is there for: together all eight kernels of prims.h, in every tile size
and width."""
import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "scripts", "prims_check")


def _launched(mode, c):
    """The kernels a mode must have launched, as scripts/prims_check labels them: name<key or
    element width, keys per thread>, the tile sizes from the constants it was built with."""
    small, mid, big = c["RS_SMALL_ITEMS"], c["RS_ITEMS"], c["RS_BIG_ITEMS"]
    if mode in ("sort32", "sort64"):
        w = mode[4:]
        ks = [f"k_rs_hist_all<u{w},{small}>", f"k_rs_hist_all<u{w},{mid}>", f"k_rs_pass<u{w},{small}>",
              f"k_rs_pass<u{w},{mid}>"]
        return ks + ([f"k_rs_pass<u32,{big}>"] if mode == "sort32" else [])
    if mode == "scan":
        return [f"{k}<u{w}>" for k in ("k_scan_small", "k_scan_tiles", "k_scan_add_sums", "k_scan_add", "k_scan_total")
                for w in (32, 64)] + ["k_scan_small3"]
    return ["k_w_reduce", "k_w_claim", "k_w_atomic", "k_w_bscan"]


def _run(mode):
    assert os.path.exists(EXE), "scripts/prims_check is not built (__graft_entry__.build() compiles it)"
    plan = json.loads(subprocess.run([EXE, "plan"], capture_output=True, text=True, timeout=60).stdout)
    r = subprocess.run([EXE, mode], capture_output=True, text=True, timeout=120)
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert not [x for x in lines if "hip_error" in x or "error" in x], lines[-1]
    cases = [x for x in lines if "ok" in x]
    bad = [x for x in cases if x["ok"] is not True]
    assert not bad, f"{len(bad)} of {len(cases)} {mode} cases failed:\n" + "\n".join(json.dumps(x) for x in bad[:20])
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-1000:])
    assert [x["name"] for x in cases] == [x["name"] for x in plan["modes"][mode]]
    summary = lines[-1]
    assert summary["summary"] == mode and summary["cases"] == len(cases) and summary["failed"] == 0
    print(mode, "cases", len(cases), "elapsed_ms", summary["elapsed_ms"], "launches", summary["launches"])
    # every kernel form the mode is there for ran, and nothing else did (64-bit keys never take
    # the 8,192-key tiles)
    assert sorted(summary["launches"]) == sorted(_launched(mode, plan["constants"])), summary["launches"]
    return summary


@pytest.mark.parametrize("mode", ["sort32", "sort64", "scan", "wave"])
def test_prims_check(khst, mode):
    _run(mode)
