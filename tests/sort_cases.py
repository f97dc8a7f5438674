"""Seeded numpy inputs that put the full build's sort paths (khst.hip: `sort_dedup`, `build`)
on both sides of two thresholds no other test stands at, with repeated keys and runs of equal
sort words where hashed or random keys never put them.

top24   hashed 20-byte keys, unsegmented, n = 2^20 and 2^20 + 1.  Up to 2^20 keys the radix
        sorts the top 24 bits of the 32-bit words only (`tsh = 8`) and the tie kernel orders every
        run of equal top-24 bits by the whole key; one key more and the radix sorts all 32 bits.
        About n^2 / 2^25 = 32,000 such runs exist at this size; 2,000 keys inside them are put
        twice, half of the second puts before every other input and half after.
seg     raw 32-byte keys in `nseg` tries, nseg = S (the most tries whose id leaves CK_KEY_BITS = 12
        key bits in a 32-bit word: 2^20) and S + 1 (the 64-bit composite sort), about 2,500 of
        them non-empty; and nseg of 1, 2, 3, 5, 17, whose words end inside a nibble.

A case is (name, keys_u8[n*klen], vals_u8, voff_u64[n+1]) plus, for seg, seg_off_u64[nseg+1].
tests/test_sort_cases.py proves on the CPU that each input has the runs it is there for;
tests/test_gpu_sort_paths.py builds them on the device.
"""
import functools

import numpy as np

SEED = 11

# ---- khst.hip: `constexpr uint32_t CK_KEY_BITS = 12`, `bits_for` (host.h), `TIE_RUN_MAX = 64`, the tie
# kernel's block of TF_ITEMS * BS = 1,024 sorted positions, and `n <= (1ull << 20) ? 8u : 0u`
CK_KEY_BITS = 12
TIE_RUN_MAX = 64
TIE_BLOCK = 1024
TOP24_MAX_N = 1 << 20


def bits_for(nseg):
    b = 0
    while (1 << b) < nseg:
        b += 1
    return b


def seg_words_max():
    """S: the largest nseg with bits_for(nseg) + CK_KEY_BITS <= 32 (khst.hip `seg_words_ok`)."""
    return 1 << (32 - CK_KEY_BITS)


def _values(rng, n, lens=(1, 33, 70, 90)):
    ln = rng.choice(lens, n).astype(np.uint64)
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum(ln)
    return rng.integers(1, 256, int(off[-1]) + 8, dtype=np.uint8), off


def key_ids(keys, klen):
    """An id per input, equal for equal keys (uint32[n]), and the number of distinct keys."""
    k = np.ascontiguousarray(keys, np.uint8).reshape(-1, klen)
    pad = np.zeros((len(k), -klen % 8), np.uint8)
    cols = np.concatenate([k, pad], axis=1).view(">u8")
    order = np.lexsort([cols[:, j] for j in range(cols.shape[1] - 1, -1, -1)])
    s = cols[order]
    new = np.concatenate([[True], (s[1:] != s[:-1]).any(axis=1)])
    ids = np.empty(len(k), np.uint32)
    ids[order] = (np.cumsum(new) - 1).astype(np.uint32)
    return ids, int(new.sum())


# ---------------------------------------------------------------------------
# top24
# ---------------------------------------------------------------------------
TOP24_REPEATS = 2000
TOP24_BUILDS = ("distinct_2p20", "distinct_2p20+1", "repeats_2p20", "repeats_2p20+1")


def hashed_words(oracle, keys20):
    """The leading 32 bits of kec256 of each 20-byte key (uint32[n]), by the oracle's Keccak."""
    n = len(keys20)
    raw = np.ascontiguousarray(keys20, np.uint8).tobytes()
    out = np.empty(n, np.uint32)
    kec = oracle.batch_kec256
    for i in range(n):
        out[i] = int.from_bytes(kec(raw[20 * i:20 * i + 20])[:4], "big")
    return out


@functools.lru_cache(maxsize=1)
def _top24_pool(oracle):
    """2^20 + 1 distinct random addresses and their words: the first 2^20 - R are the base, the
    next R pad the repeat-free build, the last one is the key past 2^20."""
    rng = np.random.default_rng([SEED, 24])
    n = TOP24_MAX_N + 1
    pool = rng.integers(0, 256, (n + 64, 20), dtype=np.uint8)
    ids, distinct = key_ids(pool, 20)
    assert distinct == n + 64  # (160-bit random keys)
    pool = pool[:n]
    return pool, hashed_words(oracle, pool)


@functools.lru_cache(maxsize=4)
def top24_case(oracle, build):
    """(case, src): src[i] is the pool index of input i (pool and words from _top24_pool)."""
    pool, words = _top24_pool(oracle)
    nb = TOP24_MAX_N - TOP24_REPEATS
    rng = np.random.default_rng([SEED, 25])
    if build.startswith("distinct"):
        src = np.arange(TOP24_MAX_N)
    else:  # keys of the base that share their top 24 bits with another key of it, put twice
        top = words[:nb] >> 8
        u, cnt = np.unique(top, return_counts=True)
        in_run = np.flatnonzero(np.isin(top, u[cnt >= 2]))
        rep = rng.choice(in_run, TOP24_REPEATS, replace=False)
        half = TOP24_REPEATS // 2
        src = np.concatenate([rep[:half], np.arange(nb), rep[half:]])
    if build.endswith("+1"):
        src = np.concatenate([src, [TOP24_MAX_N]])
    vals, voff = _values(np.random.default_rng([SEED, 26, TOP24_BUILDS.index(build)]), len(src))
    keys = np.ascontiguousarray(pool[src]).reshape(-1)
    return ("top24_" + build, keys, vals, voff), src


def word_runs(words, ids, shift):
    """The runs of inputs equal in `words >> shift`, in the order the stable radix leaves them
    (word bits, input position): (order, run start positions, run lengths, distinct keys per run)."""
    top = words >> np.uint32(shift) if shift else words
    order = np.argsort(top, kind="stable")
    st = top[order]
    brk = np.flatnonzero(np.concatenate([[True], st[1:] != st[:-1], [True]]))
    start, length = brk[:-1], np.diff(brk)
    run_of = np.repeat(np.arange(len(start)), length)
    pair = np.unique(run_of.astype(np.int64) << 32 | ids[order].astype(np.int64))
    distinct = np.bincount(pair >> 32, minlength=len(start))
    return order, start, length, distinct


def top24_properties(words, ids):
    """What the tie kernel meets in a tsh = 8 build of these inputs (see tests/test_sort_cases.py)."""
    order, start, length, distinct = word_runs(words, ids, 8)
    multi = distinct >= 2
    run_of = np.repeat(np.arange(len(start)), length)
    low = (words[order] & np.uint32(0xFF)).astype(np.int64)
    desc = np.zeros(len(order), bool)
    desc[1:] = (low[1:] < low[:-1]) & (run_of[1:] == run_of[:-1])
    unordered = np.bincount(run_of[desc], minlength=len(start)) > 0
    straddle = (start // TIE_BLOCK) != ((start + length - 1) // TIE_BLOCK)
    # runs with a key put twice and another key of the run between the two puts (input order is
    # the run's order): the two puts are not neighbours in the run
    split = 0
    sid = ids[order]
    for r in np.flatnonzero(multi & (length > distinct)):
        run = sid[start[r]:start[r] + length[r]].tolist()
        split += any(run.index(k) + 1 < len(run) - 1 - run[::-1].index(k) for k in set(run) if run.count(k) > 1)
    return {"runs": int(multi.sum()), "unordered": int((multi & unordered).sum()),
            "straddling": int((multi & straddle).sum()), "split_repeats": split, "longest": int(length.max())}


# ---------------------------------------------------------------------------
# seg
# ---------------------------------------------------------------------------
def _pack_nibbles(nib):
    return ((nib[:, 0::2] << 4) | nib[:, 1::2]).astype(np.uint8)


def _shared12(rng, c):
    """c keys equal to one random key except at nibbles 3, 4, 17 and 63: groups of four part at
    nibbles 3 (and, past 16 groups, 4); inside a group the second key parts at nibble 17, the
    third from the second at nibble 63 only, the fourth at nibble 4."""
    nib = np.tile(rng.integers(0, 16, 64, dtype=np.uint8), (c, 1))
    j = np.arange(c)
    g, m = j // 4, j % 4
    nib[:, 3] = g % 16
    nib[:, 4] = (g // 16) + 8 * (m == 3)
    nib[:, 17] = np.where((m == 1) | (m == 2), nib[:, 17] ^ 5, nib[:, 17])
    nib[:, 63] = np.where(m == 2, nib[:, 63] ^ 9, nib[:, 63])
    return _pack_nibbles(nib)[rng.permutation(c)]


def _assemble(name, tries, nseg, rng):
    """tries: {trie id: uint8[c, 32] keys in input order} -> (case, seg_off)."""
    ids = sorted(tries)
    keys = np.concatenate([tries[t] for t in ids])
    counts = np.zeros(nseg, np.int64)
    counts[ids] = [len(tries[t]) for t in ids]
    seg_off = np.zeros(nseg + 1, np.uint64)
    seg_off[1:] = np.cumsum(counts)
    vals, voff = _values(rng, len(keys), lens=(1, 1, 33, 70))
    return (name, np.ascontiguousarray(keys).reshape(-1), vals, voff), seg_off


@functools.lru_cache(maxsize=4)
def seg_case(nseg, long_run=False):
    """About 2,500 non-empty tries among nseg (see the module docstring and the issue's list):
    trie 0 and trie nseg - 1; two adjacent tries holding the same key; 600 tries of 2-64 keys
    that share their leading 12 bits (100 of them with their first key put again at the end, so
    the two puts are not adjacent); a trie of 200 random keys; the rest of 1-8 random keys.
    long_run: one more trie whose 65 keys share their leading 12 bits (past the tie kernel)."""
    rng = np.random.default_rng([SEED, 32, nseg, int(long_run)])
    pick = np.unique(np.concatenate([[0, nseg - 1], rng.integers(1, nseg - 1, 2600)]))
    mid = pick[1:-1]
    mid = mid[rng.permutation(len(mid))]
    tries = {}
    for t in (0, nseg - 1):
        tries[int(t)] = _shared12(rng, 9)
    twin = int(mid[0])
    tries[twin] = _shared12(rng, 5)
    tries[twin + 1] = tries[twin][[2, 0, 4]].copy()  # the same keys next door, other values
    rest = [int(t) for t in mid[1:] if int(t) not in (twin, twin + 1)]
    if long_run:
        tries[rest.pop()] = _shared12(rng, TIE_RUN_MAX + 1)
    tries[rest.pop()] = rng.integers(0, 256, (200, 32), dtype=np.uint8)
    for i in range(600):
        k = _shared12(rng, int(rng.integers(2, TIE_RUN_MAX + 1 - (1 if i < 100 else 0))))
        if i < 100 and len(k) >= 3:
            k = np.concatenate([k, k[:1]])  # first key again, after every other key of the trie
        tries[rest.pop()] = k
    for t in rest[:1850]:
        tries[t] = rng.integers(0, 256, (int(rng.integers(1, 9)), 32), dtype=np.uint8)
    name = f"seg_n{nseg}" + ("_run65" if long_run else "")
    return _assemble(name, tries, nseg, rng)


SMALL_NSEG = (1, 2, 3, 5, 17)


@functools.lru_cache(maxsize=8)
def small_seg_case(nseg):
    """nseg tries whose keys equal the trie's base key on every whole nibble of the sort word
    (32 - bits_for(nseg) key bits): (a) one key per value of the word's trailing partial nibble's
    bits inside the word, and under each of them (b) keys that part only past the word -- in the
    rest of that nibble, or at nibbles 8, 9, 40 or 63."""
    sb = bits_for(nseg)
    kb = 32 - sb
    whole, part = kb // 4, kb % 4
    rng = np.random.default_rng([SEED, 33, nseg])
    tries = {}
    for t in range(nseg):
        base = rng.integers(0, 16, 64, dtype=np.uint8)
        rows = []
        for a in range(1 << part):  # (a): the partial nibble's bits inside the word
            hi = (a << (4 - part)) if part else int(base[whole])
            lows = range(1 << (4 - part)) if part else [0]
            for low in lows:  # (b): its bits past the word
                r = base.copy()
                r[whole] = hi | low if part else hi
                rows.append(r)
            for pos in (8, 9, 40, 63):  # (b): later nibbles
                if pos <= whole:
                    continue
                r = base.copy()
                r[whole] = hi
                r[pos] ^= 7
                rows.append(r)
        k = _pack_nibbles(np.array(rows, np.uint8))
        tries[t] = k[rng.permutation(len(k))]
    return _assemble(f"seg_small_n{nseg}", tries, nseg, rng)


def seg_word_runs(case, seg_off):
    """Equal-word runs of a segmented input: the same trie and the same leading 32 - sb key bits.
    Returns (sb, lengths of the runs in inputs, distinct keys per run, runs holding a repeated key)."""
    _, keys, _, voff = case
    nseg = len(seg_off) - 1
    sb = bits_for(nseg)
    k = keys.reshape(-1, 32)
    seg = np.repeat(np.arange(nseg, dtype=np.uint64), np.diff(seg_off.astype(np.int64)))
    lead = k[:, :4].copy().view(">u4").reshape(-1).astype(np.uint64)
    word = (seg << np.uint64(32)) | (lead >> np.uint64(sb) << np.uint64(sb))  # (segment, leading 32 - sb key bits)
    ids, _ = key_ids(keys, 32)
    order = np.argsort(word, kind="stable")
    w = word[order]
    brk = np.flatnonzero(np.concatenate([[True], w[1:] != w[:-1], [True]]))
    start, length = brk[:-1], np.diff(brk)
    run_of = np.repeat(np.arange(len(start)), length)
    pair = np.unique(run_of.astype(np.int64) << 32 | ids[order].astype(np.int64))
    distinct = np.bincount(pair >> 32, minlength=len(start))
    return sb, length, distinct, int(((length > distinct) & (distinct >= 2)).sum())


def nonempty_only(case, seg_off):
    """The non-empty tries re-indexed 0.. (for the CPU builder): (their ids, seg_off over them)."""
    cnt = np.diff(seg_off.astype(np.int64))
    ids = np.flatnonzero(cnt > 0)
    so = np.zeros(len(ids) + 1, np.uint64)
    so[1:] = np.cumsum(cnt[ids])
    return ids, so


@functools.lru_cache(maxsize=4)
def top24_reference(oracle, build):
    """(roots, stats) of the CPU batch builder for a top24 build (computed once a process)."""
    (_, keys, vals, voff), _ = top24_case(oracle, build)
    return oracle.batch_roots(keys, (vals, voff), klen=20, hash_keys=True)


@functools.lru_cache(maxsize=4)
def seg_reference(oracle, nseg, long_run=False):
    """((roots, stats), ids): the CPU batch builder over the non-empty tries only, re-indexed (a
    million empty segments are no work for it, but a million Python root objects are); ids are
    their trie ids in the full build."""
    case, seg_off = seg_case(nseg, long_run)
    ids, so = nonempty_only(case, seg_off)
    return oracle.batch_roots(case[1], (case[2], case[3]), klen=32, seg_off=so), ids


def segmented_roots(khst, case, seg_off, stats=None):
    """kh_trie_roots_segmented over numpy buffers: uint8[nseg, 32] roots (khipu_amd.trie_roots
    takes a Python list of tries; a million of them is not one)."""
    import ctypes
    from khipu_amd._lib import check
    _, keys, vals, voff = case
    nseg = len(seg_off) - 1
    out = np.zeros((nseg, 32), np.uint8)
    st = stats if stats is not None else khst.KhStats()
    so = np.ascontiguousarray(seg_off, np.uint64)
    vo = np.ascontiguousarray(voff, np.uint64)
    check(khst.lib().kh_trie_roots_segmented(keys.ctypes.data, 32, vals.ctypes.data, vo.ctypes.data, so.ctypes.data,
                                             nseg, 0, out.ctypes.data, ctypes.byref(st)))
    return out
