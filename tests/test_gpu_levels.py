"""GPU: every branch-kernel variant of the full build over inline, nested and long children.

The build picks a level's kernel by its branch count (khst.hip "5. branch levels"):
k_branch_xl up to 8,192 branches, k_branch_small up to 32,768, above that k_branch_fused<4> +
k_branch_wide<4> (depth < 8), <6> (depth >= 8) or, in a segmented build, k_branch_fused<2>
after k_leaf_move; from 2^21 boundaries the topology comes from k_topo_tile.  The inputs
(tests/level_cases.py) put an exact number of branches with inline leaves, inline branches and
extensions, 31/32-byte children or leaves over 135 bytes into one level, one branch either side
of each threshold; tests/test_level_cases.py proves on the CPU that each input has that level.
Every root and every node count is compared with the CPU batch builder (oracle/batch_root.cc),
which the same generator pins to the sequential oracle at a reduced size.
"""
import numpy as np
import pytest

from tests import level_cases as L

pytestmark = pytest.mark.gpu

STATS = (("n_leaves", "leaves"), ("n_branches", "branches"), ("n_extensions", "extensions"), ("n_inline", "inline"),
         ("n_node_hashes", "node_hashes"), ("n_node_perms", "node_perms"))


def _device_build(khst, case, seg=None, nseg=1):
    import torch
    from khipu_amd.device import Ctx
    _, keys, vals, voff = case
    n = len(voff) - 1
    dk = torch.from_numpy(keys).to("cuda:0")
    dv = torch.from_numpy(np.concatenate([vals, np.zeros(64, np.uint8)])).to("cuda:0")
    do = torch.from_numpy(voff.astype(np.int64)).to("cuda:0")
    ds = None if seg is None else torch.from_numpy(seg.astype(np.int32)).to("cuda:0")
    return Ctx(0).build(dk, 32, dv, do, n, seg=ds, nseg=nseg, hash_keys=False)


def _check(khst, oracle, case, full_sort=0):
    name, keys, vals, voff = case
    roots, bst = oracle.batch_roots(keys, (vals, voff), klen=32)
    hh, ll, _, st = _device_build(khst, case)
    got = {b: int(getattr(st, a)) for a, b in STATS}
    print(name, "device", got, "full_sort", st.full_sort, "levels", st.n_levels, "builder", bst)
    assert ll[0] >= 32 and hh[0].tobytes() == roots[0], name
    assert got == {b: bst[b] for _, b in STATS}, name
    assert st.full_sort == full_sort, name
    return st


@pytest.mark.parametrize("kind,groups,kernel", L.ROWS, ids=[f"{k}-{g}" for k, g, _ in L.ROWS])
def test_level_kernels_vs_batch_builder(khst, oracle, kind, groups, kernel):
    """One row of the table: `groups` branches at the kind's depth, which is `kernel`'s level
    (level_cases.level_kernel over level_histogram, asserted in tests/test_level_cases.py)."""
    _check(khst, oracle, L.row_case(kind, groups))


def test_wide_branch_over_inline_children(khst, oracle):
    """inline31 at 32,769 groups plus 6,000 keys with 1-byte values under one more 8-nibble
    prefix: that branch spans more than 4,096 positions of the large depth-8 level, so its wave
    leaves it to k_branch_wide<6>, beside branches with inline leaf children.  6,000 keys equal
    in their leading 32 bits are past the tie kernel's 64-key runs: the one case here whose
    keys the full sort orders (full_sort == 1, as cases.py's prefix_ties_long)."""
    _check(khst, oracle, L.wide_case(), full_sort=1)


@pytest.mark.parametrize("kind", ["deep", "inline31"])
def test_segmented_levels_vs_batch_builder(khst, oracle, kind):
    """The 32,769-group case cut into 64 tries by the keys' leading 6 bits and built with
    seg / nseg: k_leaf_move copies the early leaves' inline bodies into the child records and
    k_branch_fused<2> reads them; one root per trie and the summed node counts."""
    base = L.row_case(kind, 32769)
    seg, grouped, seg_off = L.by_segment(base, L.SEG_BITS)
    roots, bst = oracle.batch_roots(grouped[1], (grouped[2], grouped[3]), klen=32, seg_off=seg_off)
    hh, ll, _, st = _device_build(khst, base, seg=seg, nseg=64)
    got = {b: int(getattr(st, a)) for a, b in STATS}
    print(grouped[0], "device", got, "full_sort", st.full_sort, "builder", bst)
    assert (ll >= 32).all()
    assert [hh[s].tobytes() for s in range(64)] == roots
    assert got == {b: bst[b] for _, b in STATS}
    assert st.full_sort == 0


@pytest.mark.parametrize("m", L.TILE_SIZES, ids=lambda m: f"2p21+{m - L.TOPO_TILE_MIN}")
def test_tile_threshold_with_inline_leaves(khst, oracle, m):
    """inline31 at 40,000 groups padded to m keys: 2^21 - 1 boundaries (k_ansv_pd, the leaves'
    metas preset by a memset), 2^21 and 2^21 + 1 (k_topo_tile presets them per tile); in both
    forms the leaf kernel must overwrite the preset of every inline leaf."""
    st = _check(khst, oracle, L.tile_case(m))
    assert st.n_leaves == m
