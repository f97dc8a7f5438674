"""CPU: the inputs of tests/test_gpu_sort_paths.py have the runs and repeats they are there for
(tests/sort_cases.py), proven from the inputs alone, so the GPU tests cannot pass vacuously.  The
floors are conditions on the generators: a seed that misses one is changed, not the floor."""
import numpy as np
import pytest

from tests import sort_cases as C


# ---- top24 -----------------------------------------------------------------
@pytest.mark.parametrize("build", C.TOP24_BUILDS)
def test_top24_conditions(oracle, build):
    """n is 2^20 or 2^20 + 1; the keys' words are the oracle's Keccak of the keys themselves;
    at least 10,000 runs of two or more distinct keys equal in their top 24 bits, 1,000 of them
    with their low bytes out of order in input order (the tie kernel must move a word), 10 across
    a multiple of 1,024 sorted positions (the tie kernel's block), none over TIE_RUN_MAX inputs;
    with repeats, 500 runs where another key of the run lies between the two puts; and the CPU
    builder's leaf count is the number of distinct keys."""
    (name, keys, vals, voff), src = C.top24_case(oracle, build)
    pool, words = C._top24_pool(oracle)
    n = len(voff) - 1
    assert n == C.TOP24_MAX_N + (1 if build.endswith("+1") else 0)
    assert np.array_equal(keys.reshape(-1, 20), pool[src])
    # (the pool's words are the keys' hashes: spot-checked here against a second Keccak of the oracle)
    for i in (0, 1, n // 2, n - 1):
        assert int.from_bytes(oracle.kec256(keys[20 * i:20 * i + 20].tobytes())[:4], "big") == int(words[src[i]])
    ids, distinct = C.key_ids(keys, 20)
    repeats = build.startswith("repeats")
    assert n - distinct == (C.TOP24_REPEATS if repeats else 0)
    p = C.top24_properties(words[src], ids)
    print(name, "n", n, "distinct", distinct, p)
    assert p["runs"] >= 10_000
    assert p["unordered"] >= 1_000
    assert p["straddling"] >= 10
    assert p["longest"] <= C.TIE_RUN_MAX
    if repeats:
        assert p["split_repeats"] >= 500
        vo = voff.astype(np.int64)
        half = C.TOP24_REPEATS // 2
        # half of the second puts come before every other input, half after; each with a value of its own
        first, last = src[:half], src[C.TOP24_MAX_N - half:C.TOP24_MAX_N]
        base = src[half:C.TOP24_MAX_N - half]
        assert np.array_equal(base, np.arange(len(base))) and len(np.unique(np.concatenate([first, last]))) == 2 * half
        for put, orig in [(0, half + int(first[0])), (C.TOP24_MAX_N - 1, half + int(last[-1]))]:
            assert keys[20 * put:20 * put + 20].tobytes() == keys[20 * orig:20 * orig + 20].tobytes()
            assert vals[vo[put]:vo[put + 1]].tobytes() != vals[vo[orig]:vo[orig + 1]].tobytes()
    _, st = C.top24_reference(oracle, build)
    assert st["leaves"] == st["distinct"] == distinct


# ---- seg -------------------------------------------------------------------
def _seg_stats(case, seg_off):
    sb, length, distinct, with_repeat = C.seg_word_runs(case, seg_off)
    multi = distinct >= 2
    return {"sb": sb, "runs_2_64": int((multi & (length <= C.TIE_RUN_MAX)).sum()),
            "runs_over_64": int((length > C.TIE_RUN_MAX).sum()), "runs_with_repeat": with_repeat,
            "longest": int(length.max())}


def test_seg_words_threshold_is_the_rule():
    S = C.seg_words_max()
    assert C.bits_for(S) + C.CK_KEY_BITS <= 32 < C.bits_for(S + 1) + C.CK_KEY_BITS
    assert S == 1 << 20


@pytest.mark.parametrize("over", [0, 1], ids=["S", "S+1"])
@pytest.mark.parametrize("long_run", [False, True], ids=["runs<=64", "run65"])
def test_seg_conditions(oracle, over, long_run):
    nseg = C.seg_words_max() + over
    case, seg_off = C.seg_case(nseg, long_run)
    name, keys, vals, voff = case
    n = len(voff) - 1
    cnt = np.diff(seg_off.astype(np.int64))
    assert len(seg_off) == nseg + 1 and int(seg_off[-1]) == n == len(keys) // 32
    assert cnt[0] > 0 and cnt[-1] > 0
    assert 2300 <= (cnt > 0).sum() <= 2700 and 25_000 <= n <= 35_000
    s = _seg_stats(case, seg_off)
    print(name, "n", n, "non-empty", int((cnt > 0).sum()), s)
    assert s["sb"] == 20 + over
    # the words path is the one taken at S: 12 key bits left, and few keys per trie
    assert (s["sb"] + C.CK_KEY_BITS <= 32) == (over == 0)
    assert n // nseg <= 1 << (32 - s["sb"] - 2)
    assert s["runs_2_64"] >= 500
    assert s["runs_over_64"] == (1 if long_run else 0) and s["longest"] == (65 if long_run else 64)
    assert s["runs_with_repeat"] >= 20
    k = keys.reshape(-1, 32)
    so = seg_off.astype(np.int64)
    # two adjacent tries hold the same key with different values
    vo = voff.astype(np.int64)
    twins = 0
    for t in np.flatnonzero((cnt[:-1] > 0) & (cnt[1:] > 0)):
        a = {k[i].tobytes(): vals[vo[i]:vo[i + 1]].tobytes() for i in range(so[t], so[t + 1])}
        b = {k[i].tobytes(): vals[vo[i]:vo[i + 1]].tobytes() for i in range(so[t + 1], so[t + 2])}
        twins += any(key in a and a[key] != b[key] for key in b)
    assert twins >= 1
    # a repeated key's two puts are not adjacent in the input
    apart = 0
    for t in np.flatnonzero(cnt >= 3):
        rows = [k[i].tobytes() for i in range(so[t], so[t + 1])]
        apart += rows[0] == rows[-1]
    assert apart >= 20
    # a trie of 200 keys over random leading bits; tries whose keys share 12 bits and part at nibbles 3, 4, 17, 63
    assert (cnt == 200).sum() == 1
    t = int(np.flatnonzero(cnt == 200)[0])
    assert len(np.unique(k[so[t]:so[t + 1], :2].copy().view(">u2") >> 4)) > 150
    parts = set()
    for t in np.flatnonzero((cnt >= 9) & (cnt <= 65))[:50]:  # (the random tries hold up to 8 keys)
        rows = np.unique(k[so[t]:so[t + 1]], axis=0)
        nib = np.stack([rows >> 4, rows & 15], axis=2).reshape(len(rows), 64)
        assert (nib[:, :3] == nib[0, :3]).all()
        for i in range(len(rows) - 1):  # sorted rows: where neighbours part
            parts.add(int(np.argmax(nib[i] != nib[i + 1])))
    assert parts == {3, 4, 17, 63}
    # the CPU builder over the non-empty tries keeps every distinct (trie, key)
    (_, st), ids = C.seg_reference(oracle, nseg, long_run)
    assert len(ids) == (cnt > 0).sum()
    assert st["leaves"] == st["distinct"] == len({(int(t), k[i].tobytes()) for t in ids for i in range(so[t], so[t + 1])})


@pytest.mark.parametrize("nseg", C.SMALL_NSEG)
def test_small_seg_conditions(oracle, nseg):
    """The word's key bits end inside a nibble (sb of 1, 2, 3, 5; at sb = 0 at a nibble's end):
    a trie's keys are equal on every whole nibble of the word, part (a) inside the trailing
    partial nibble's word bits and (b) only past the word -- equal-word runs for the tie kernel."""
    case, seg_off = C.small_seg_case(nseg)
    name, keys, vals, voff = case
    sb = C.bits_for(nseg)
    assert sb == {1: 0, 2: 1, 3: 2, 5: 3, 17: 5}[nseg]
    kb = 32 - sb
    whole, part = kb // 4, kb % 4
    k = keys.reshape(-1, 32)
    nib = np.stack([k >> 4, k & 15], axis=2).reshape(len(k), 64)
    so = seg_off.astype(np.int64)
    s = _seg_stats(case, seg_off)
    print(name, "n", len(k), s)
    assert (np.diff(so) > 0).all()
    for t in range(nseg):
        rows = nib[so[t]:so[t + 1]]
        assert (rows[:, :whole] == rows[0, :whole]).all()
        inside = rows[:, whole] >> (4 - part) if part else np.zeros(len(rows), np.uint8)
        assert len(np.unique(inside)) == 1 << part  # (a)
        for a in np.unique(inside):  # (b): equal in the word, distinct past it
            grp = rows[inside == a]
            assert len(grp) >= 4 and len(np.unique(grp, axis=0)) == len(grp)
            differ = np.flatnonzero((grp != grp[0]).any(axis=0))
            assert set(differ) <= {whole, 8, 9, 40, 63} and {40, 63} <= set(differ)
    assert s["runs_2_64"] == nseg << part and s["runs_over_64"] == 0
    roots, st = oracle.batch_roots(keys, (vals, voff), klen=32, seg_off=seg_off)
    assert st["leaves"] == len(k) and len(set(roots)) == nseg
