"""GPU: the full build's sort paths either side of two thresholds of khst.hip's `build`, over
inputs with repeated keys and runs of equal sort words (tests/sort_cases.py; the CPU test
tests/test_sort_cases.py proves each input has them).

* `tsh = 8`: hashed unsegmented builds of n <= 2^20 radix-sort the top 24 bits of the words and
  leave every run of equal top-24 bits to the tie kernel; at 2^20 + 1 the radix sorts all 32.
* `seg_words_ok`: segmented plain builds sort 32-bit (trie id | key bits) words while
  bits_for(nseg) + CK_KEY_BITS <= 32 (nseg <= 2^20, 12 key bits left: every trie of several keys
  is an equal-word run), the 64-bit composite above; a run past TIE_RUN_MAX takes the full sort
  with its segment pass.

Roots (and n_leaves, full_sort) against oracle.batch_roots, the independent CPU batch builder.
"""
import numpy as np
import pytest

from tests import sort_cases as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("build", C.TOP24_BUILDS)
def test_top24_builds(khst, oracle, build):
    """2^20 inputs: the tie kernel orders about 31,000 runs (and drops the earlier put of 2,000
    repeated keys inside them); 2^20 + 1: the same inputs with the low byte sorted by the radix."""
    (name, keys, vals, voff), _ = C.top24_case(oracle, build)
    roots, bst = C.top24_reference(oracle, build)
    st = khst.KhStats()
    got = khst.trie_root(keys, (vals, voff), hash_keys=True, klen=20, stats=st)
    print(name, "n_leaves", st.n_leaves, "full_sort", st.full_sort, "t_sort_ms", st.t_sort_ms)
    assert got == roots[0], name
    assert st.n_leaves == bst["leaves"], name
    assert st.full_sort == 0, name


def _check_segmented(khst, oracle, case, seg_off, ref_roots, ids):
    st = khst.KhStats()
    got = C.segmented_roots(khst, case, seg_off, stats=st)
    empty = np.ones(len(seg_off) - 1, bool)
    empty[ids] = False
    # every empty trie, as one comparison
    assert (got[empty] == np.frombuffer(khst.EMPTY_TRIE_HASH, np.uint8)).all(), case[0]
    want = np.frombuffer(b"".join(ref_roots), np.uint8).reshape(-1, 32)
    bad = np.flatnonzero((got[ids] != want).any(axis=1))
    assert len(bad) == 0, (case[0], "tries", ids[bad][:10].tolist())
    return st


@pytest.mark.parametrize("over", [0, 1], ids=["S", "S+1"])
@pytest.mark.parametrize("long_run", [False, True], ids=["runs<=64", "run65"])
def test_seg_words_threshold(khst, oracle, over, long_run):
    """nseg = S: the tie kernel on segmented words (about 600 runs of 2-64 keys, 99 with a
    repeated key), and with the 65-key run the full sort with its segment pass; nseg = S + 1: the
    64-bit composite sort of the same shapes.  The CPU builder gets the non-empty tries only,
    re-indexed (sort_cases.seg_reference); the empty ones must be EMPTY_TRIE_HASH."""
    # khst.hip: `constexpr uint32_t CK_KEY_BITS = 12` and, in build(),
    # `seg_words_ok = segmented && sb + CK_KEY_BITS <= 32 && ...` with sb = bits_for(nseg):
    # S is the largest nseg that passes
    CK_KEY_BITS, WORD_BITS = 12, 32
    S = 1 << (WORD_BITS - CK_KEY_BITS)
    assert C.bits_for(S) + CK_KEY_BITS <= WORD_BITS < C.bits_for(S + 1) + CK_KEY_BITS
    assert (CK_KEY_BITS, S) == (C.CK_KEY_BITS, C.seg_words_max())
    nseg = S + over
    case, seg_off = C.seg_case(nseg, long_run)
    (roots, bst), ids = C.seg_reference(oracle, nseg, long_run)
    st = _check_segmented(khst, oracle, case, seg_off, roots, ids)
    print(case[0], "n_leaves", st.n_leaves, "full_sort", st.full_sort)
    assert st.n_leaves == bst["leaves"]
    assert st.full_sort == (1 if long_run else 0)


@pytest.mark.parametrize("nseg", C.SMALL_NSEG)
def test_small_segment_counts(khst, oracle, nseg):
    """sb of 0, 1, 2, 3, 5: the word's key bits end inside a nibble; keys that part inside the
    trailing partial nibble (the radix orders them) and only past the word (the tie kernel)."""
    case, seg_off = C.small_seg_case(nseg)
    roots, bst = oracle.batch_roots(case[1], (case[2], case[3]), klen=32, seg_off=seg_off)
    st = _check_segmented(khst, oracle, case, seg_off, roots, np.arange(nseg))
    assert st.n_leaves == bst["leaves"] and st.full_sort == 0
