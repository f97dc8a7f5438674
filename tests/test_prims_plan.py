"""CPU: the case table of scripts/prims_check (`prims_check plan`, no HIP call) holds what
tests/test_gpu_prims.py relies on: every threshold of prims.h with the size before it, the size
itself and the one after it in the group that crosses it, every bit range the library sorts on,
the radix tile sizes the cases claim, and only a handful of cases at 4M elements.  The sizes come
from the constants the binary was built with, so a changed threshold moves the cases with it."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "scripts", "prims_check")

RANGES32 = {(0, 32), (8, 32)}
RANGES64 = {(32, 64), (40, 64), (0, 64), (0, 8), (0, 24), (0, 40)}
DISTS = {"uniform", "equal", "two_digits", "absent_digit", "sorted", "reverse", "ties16", "low_byte"}
FIXED_SORT_SIZES = {0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097}
FIXED_SCAN_SIZES = {0, 1, 2, 1023, 1024, 1025, 8191, 8192, 8193}


@pytest.fixture(scope="module")
def plan():
    if not os.path.exists(EXE):
        pytest.skip("scripts/prims_check is not built (__graft_entry__.build() compiles it)")
    r = subprocess.run([EXE, "plan"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    return json.loads(r.stdout)


def _around(x):
    return {x - 1, x, x + 1}


def test_constants_present(plan):
    c = plan["constants"]
    for name in ("RS_SMALL_N", "RS_BIG_N", "RS_ITEMS", "RS_BIG_ITEMS", "SCAN_TILE", "SCAN_SMALL_MAX",
                 "SCAN_TWO_MAX_TILES"):
        assert c[name] > 0, name
    assert set(plan["modes"]) == {"sort32", "sort64", "scan", "wave"}


@pytest.mark.parametrize("mode,ranges", [("sort32", RANGES32), ("sort64", RANGES64)])
def test_sort_sizes_ranges_and_distributions(plan, mode, ranges):
    c = plan["constants"]
    single = [x for x in plan["modes"][mode] if not x["steps"]]
    sizes = {x["n"] for x in single}
    small = FIXED_SORT_SIZES | _around(c["RS_SMALL_N"])
    assert small | _around(c["RS_BIG_N"]) <= sizes
    assert {(x["lo"], x["hi"]) for x in single} == ranges
    # every distribution, bit range and scratch form at every size up to RS_SMALL_N + 1
    have = {(x["n"], x["lo"], x["hi"], x["dist"], x["scratch"]) for x in single}
    for n in small:
        for lo, hi in ranges:
            for d in DISTS:
                for s in ("filled_ff", "hdr_zeroed"):
                    assert (n, lo, hi, d, s) in have, (n, lo, hi, d, s)
    # two distributions and both scratch forms at the 4M sizes
    big = [x for x in single if x["n"] >= c["RS_BIG_N"] - 1]
    assert len({x["dist"] for x in big}) >= 2 and {x["scratch"] for x in big} == {"filled_ff", "hdr_zeroed"}
    # scratch reuse: small, 4M, small on one scratch
    seqs = [[s["n"] for s in x["steps"]] for x in plan["modes"][mode] if x["steps"]]
    assert any(len(s) == 3 and s[0] <= c["RS_SMALL_N"] and s[1] >= c["RS_BIG_N"] and s[2] <= c["RS_SMALL_N"]
               for s in seqs), seqs


@pytest.mark.parametrize("mode", ["sort32", "sort64"])
def test_radix_items_at_the_sizes(plan, mode):
    """radix_items gives 4 keys a thread up to RS_SMALL_N, RS_ITEMS above it, and RS_BIG_ITEMS
    from RS_BIG_N for 32-bit keys only (64-bit keys stay on RS_ITEMS)."""
    c = plan["constants"]
    assert (c["RS_SMALL_ITEMS"], c["RS_ITEMS"], c["RS_BIG_ITEMS"]) == (4, 16, 32)
    assert plan["radix_items_64bit_big_ok"] is True
    seen = set()
    for x in plan["modes"][mode]:
        for n, items in [(x["n"], x["items"])] + [(s["n"], s["items"]) for s in x["steps"]]:
            want = 4 if n <= c["RS_SMALL_N"] else 32 if (n >= c["RS_BIG_N"] and mode == "sort32") else 16
            assert items == want, (x["name"], n, items)
            seen.add(items)
        if not x["steps"]:
            assert x["tiles"] == -(-x["n"] // (256 * x["items"])), x["name"]
    assert seen == ({4, 16, 32} if mode == "sort32" else {4, 16})
    at = {x["n"]: x["items"] for x in plan["modes"][mode] if not x["steps"]}
    assert (at[c["RS_SMALL_N"]], at[c["RS_SMALL_N"] + 1]) == (4, 16)
    assert (at[c["RS_BIG_N"] - 1], at[c["RS_BIG_N"]]) == ((16, 32) if mode == "sort32" else (16, 16))


def test_scan_sizes(plan):
    c = plan["constants"]
    scan = [x for x in plan["modes"]["scan"] if not x["name"].startswith("scan_small3")]
    two_max = c["SCAN_TWO_MAX_TILES"] * c["SCAN_TILE"]
    small = FIXED_SCAN_SIZES | _around(c["SCAN_TILE"]) | _around(c["SCAN_SMALL_MAX"])
    for eb in (4, 8):
        sizes = {x["n"] for x in scan if x["elem_bytes"] == eb}
        assert small | _around(two_max) <= sizes, eb
        # the nested form (small_ok = false) at every n <= SCAN_SMALL_MAX + 1, every input at those sizes
        for n in small:
            for inp in ("ones", "random20", "large"):
                for so in (True, False):
                    assert any(x["n"] == n and x["elem_bytes"] == eb and x["input"] == inp and x["small_ok"] == so
                               for x in scan), (eb, n, inp, so)
    assert {x["input"] for x in scan if x["n"] >= two_max - 1} == {"ones", "random20", "large"}
    s3 = {x["n"] for x in plan["modes"]["scan"] if x["name"].startswith("scan_small3")}
    assert s3 == {1, 1025, c["SCAN_SMALL_MAX"]}


def test_wave_cases(plan):
    names = {x["name"] for x in plan["modes"]["wave"]}
    assert {"wave_max_u32", "wave_sum_u32", "wave_sum_u64", "wave_atomic_add", "block_exclusive_scan_u32"} <= names
    assert {"wave_claim/all", "wave_claim/none", "wave_claim/one", "wave_claim/alternating",
            "wave_claim/divergent_all"} <= names


def test_few_large_cases(plan):
    """A device mode runs in seconds: at most six of its cases hold more than 2^20 elements,
    everything else 70k or fewer."""
    for mode, cases in plan["modes"].items():
        ns = [max([x["n"]] + [s["n"] for s in x.get("steps", [])]) for x in cases]
        assert sum(n > 1 << 20 for n in ns) <= 6, mode
        assert all(n > 1 << 20 or n <= 70_000 for n in ns), mode
        assert len({x["name"] for x in cases}) == len(cases), mode
