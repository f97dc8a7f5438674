"""CPU: the inputs of tests/test_gpu_levels.py are what they claim (tests/level_cases.py), so
the GPU tests cannot pass vacuously -- the target level holds exactly the stated number of
branches and therefore runs in the stated kernel, the hard children are there -- and the
generator's tries, at a size the sequential oracle and the host replay take, give one root in
the sequential oracle, the CPU batch builder and tests/emu in both link modes."""
import numpy as np
import pytest

from tests import level_cases as L
from tests.emu import emu as E

REDUCED = 300  # groups of the cases that go through the sequential oracle and the host replay


def _conditions(oracle, case, kind, depth, groups, kernel, segmented=False, sort_bits=0, full_sort=False):
    name, keys, vals, voff = case
    n = len(voff) - 1
    hist = L.level_histogram(keys)
    _, st = oracle.batch_roots(keys, (vals, voff), klen=32)
    assert st["distinct"] == st["leaves"] == n, name
    assert hist[depth] == groups, name
    assert hist.sum() == st["branches"], name
    assert L.level_kernel(hist[depth], depth, segmented) == kernel, name
    if kind == "long":
        assert st["inline"] == 0 and (L.leaf_lengths(case, depth) > 135).any(), name
    else:
        assert st["inline"] > 0, name
    # the 32-bit sort orders runs of up to TIE_RUN_MAX equal words; a longer one takes the full sort
    assert (L.max_word_run(keys, sort_bits) > L.TIE_RUN_MAX) == full_sort, name
    return hist, st


@pytest.mark.parametrize("kind,groups,kernel", L.ROWS, ids=[f"{k}-{g}" for k, g, _ in L.ROWS])
def test_row_level_conditions(oracle, kind, groups, kernel):
    depth = L.KIND_DEPTH[kind]
    hist, _ = _conditions(oracle, L.row_case(kind, groups), kind, depth, groups, kernel)
    if kind == "nested":  # the inline depth-62 branches under the slots that hold two keys
        assert hist[62] > groups
    big = np.flatnonzero(hist > L.XL_LEVEL)
    assert set(big) <= {depth, 62}, (kind, groups, hist[big])  # every other level: k_branch_xl


def test_wide_level_conditions(oracle):
    """The cluster's 8-nibble prefix is one more branch of the large depth-8 level and holds
    more than 4,096 sorted positions (k_branch_wide<6>, the SRC_POSK form); its 6,000 equal sort words exceed
    TIE_RUN_MAX, so this build alone orders its keys by the full sort."""
    case = L.wide_case()
    _conditions(oracle, case, "inline31", 8, 32769 + 1, "k_branch_fused<6>", full_sort=True)
    k = case[1].reshape(-1, 32)
    wide4 = np.array([0xC0, 0xFF, 0xEE, 0x01], np.uint8)
    assert tuple(L.WIDE_PREFIX) == tuple(int(x) for b in wide4 for x in (b >> 4, b & 15))
    under = k[(k[:, :4] == wide4).all(axis=1)]
    assert 4096 < len(under) == L.WIDE_KEYS
    # three children of the wide branch itself are leaves (one key under their nibble), whose
    # values make a 31-byte inline leaf, a 32-byte hashed one and a long one
    nib8, cnt = np.unique(under[:, 4] >> 4, return_counts=True)
    assert len(nib8) == 16 and sorted(cnt)[:4] == [1, 1, 1, sorted(cnt)[3]] and sorted(cnt)[3] > 1
    lone = [int(x) for x in L.leaf_lengths(case, 8)[-3:]]
    assert lone[:2] == [31, 32] and lone[2] > 100


@pytest.mark.parametrize("kind", ["deep", "inline31"])
def test_segmented_level_conditions(oracle, kind):
    """Cut into 64 tries by the keys' leading 6 bits, no key moves to another prefix: the level
    keeps its 32,769 branches (k_branch_fused<2>), every trie is populated, and the 26 key bits
    left in the sort word keep the runs of equal words within TIE_RUN_MAX."""
    depth = L.KIND_DEPTH[kind]
    base = L.row_case(kind, 32769)
    seg, grouped, seg_off = L.by_segment(base, L.SEG_BITS)
    assert len(seg_off) == 65 and (np.diff(seg_off.astype(np.int64)) > 0).all()
    assert np.array_equal(np.bincount(seg, minlength=64), np.diff(seg_off.astype(np.int64)))
    _conditions(oracle, grouped, kind, depth, 32769, "k_branch_fused<2>", segmented=True, sort_bits=L.SEG_BITS)
    roots, st = oracle.batch_roots(grouped[1], (grouped[2], grouped[3]), klen=32, seg_off=seg_off)
    _, st1 = oracle.batch_roots(base[1], (base[2], base[3]), klen=32)
    assert len(set(roots)) == 64 and st["inline"] > 0
    # the root and the 16 depth-1 branches give way to the 64 tries' own depth-1 roots (4 of the
    # 16 second nibbles each); everything from depth 2 down lies inside one trie
    assert st["branches"] == st1["branches"] - 17 + 64


@pytest.mark.parametrize("m", L.TILE_SIZES, ids=lambda m: f"2p21+{m - L.TOPO_TILE_MIN}")
def test_tile_threshold_level_conditions(oracle, m):
    """m distinct keys: m - 1 boundaries, one either side of TOPO_TILE_MIN and the value itself;
    the padding leaves the depth-8 level at its 40,000 branches."""
    case = L.tile_case(m)
    assert len(case[3]) - 1 == m and (m - 1 >= L.TOPO_TILE_MIN) == (m > L.TILE_SIZES[0])
    _conditions(oracle, case, "inline31", 8, 40000, "k_branch_fused<6>")


def _lists(case):
    _, keys, vals, voff = case
    n = len(voff) - 1
    vo = voff.astype(np.int64)
    return ([keys[32 * i:32 * i + 32].tobytes() for i in range(n)],
            [vals[vo[i]:vo[i + 1]].tobytes() for i in range(n)])


@pytest.fixture(scope="module", params=L.KINDS)
def reduced(request, oracle):
    """(case, sequential root, batch roots and stats) of one kind at REDUCED groups."""
    case = L.level_case(L.KIND_DEPTH[request.param], REDUCED, request.param, L.SEED)
    _, keys, vals, voff = case
    want = oracle.seq_root_packed(keys, 32, vals, voff, len(voff) - 1)
    return case, want, oracle.batch_roots(keys, (vals, voff), klen=32)


def test_generator_vs_sequential_oracle(oracle, reduced):
    case, want, (roots, st) = reduced
    assert roots[0] == want
    hist = L.level_histogram(case[1])
    kind = case[0].split("_")[0]
    assert hist[L.KIND_DEPTH[kind]] == REDUCED and hist.sum() == st["branches"]
    assert (st["inline"] > 0) == (kind != "long")


@pytest.mark.parametrize("link_mode", [0, 2], ids=["move", "positions"])
def test_generator_host_replay(oracle, reduced, link_mode):
    """tests/emu's build, both ways the early leaves reach their parents: the oracle's root and
    the batch builder's node counts (the stats the GPU tests compare)."""
    case, want, (_, bst) = reduced
    keys, vals = _lists(case)
    E.set_link_mode(link_mode)
    try:
        res, st = E.build(keys, vals)
    finally:
        E.set_link_mode(0)
    assert res[0][0] == want
    got = dict(zip(("leaves", "branches", "node_hashes", "node_perms", "inline", "extensions"), map(int, st)))
    assert got == {k: bst[k] for k in got}


def test_generator_host_replay_segmented(oracle):
    """The segmented form of the GPU test at REDUCED groups: 64 tries through the host replay's
    link slots and copy pass, each root against the sequential oracle."""
    for kind in ("deep", "inline31"):
        base = L.level_case(L.KIND_DEPTH[kind], REDUCED, kind, L.SEED)
        seg, grouped, seg_off = L.by_segment(base, L.SEG_BITS)
        keys, vals = _lists(base)
        res, _ = E.build(keys, vals, seg=seg, nseg=64)
        gk, gv = _lists(grouped)
        roots, _ = oracle.batch_roots(grouped[1], (grouped[2], grouped[3]), klen=32, seg_off=seg_off)
        for s in range(64):
            a, b = int(seg_off[s]), int(seg_off[s + 1])
            assert b > a
            assert res[s][0] == roots[s] == oracle.seq_root(gk[a:b], gv[a:b]), (kind, s)
