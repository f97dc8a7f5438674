"""Seeded numpy inputs that put a chosen number of branches with chosen kinds of children
into one trie level, so that each of the full build's branch kernels meets inline leaves,
inline branches and extensions, long leaves and the 31/32-byte inline rule, not only
32-byte hashes (tests/cases.py holds the same node shapes at sizes that all fit k_branch_xl).

A case is (name, keys_u8[n*32], vals_u8, voff_u64[n+1]): raw 32-byte keys in shuffled input
order, the values packed back to back (8 spare bytes after the last).  tests/test_level_cases.py
checks on the CPU that every case has the level it claims; tests/test_gpu_levels.py runs them
through the device build.
"""
import functools

import numpy as np

from khipu_amd import codec

# The full build picks a branch kernel per level by the level's branch count.  These mirror
# khipu_amd/csrc/khst.hip: `#define KH_XL_LEVEL 8192` / `constexpr uint32_t XL_LEVEL`,
# `constexpr uint32_t SMALL_LEVEL = 32768`, `constexpr uint64_t TOPO_TILE_MIN = 1u << 21`
# (boundaries between distinct sorted keys, i.e. keys - 1), and `TIE_RUN_MAX = 64` (the longest
# run of keys equal in their leading 32 bits that the 32-bit sort orders without the full sort).
XL_LEVEL = 8192
SMALL_LEVEL = 32768
TOPO_TILE_MIN = 1 << 21
TIE_RUN_MAX = 64

KINDS = ("long", "inline31", "deep", "nested")
KIND_DEPTH = {"long": 5, "inline31": 8, "deep": 62, "nested": 60}
CHILD_COUNTS = (2, 3, 6, 7, 16)
LONG_LENS = (1, 33, 55, 56, 100, 136, 255, 256, 300, 1000)


def level_kernel(count, depth, segmented=False):
    """The kernel a level of `count` branches at `depth` runs in (khst.hip, "5. branch
    levels"), for a root-only build of fixed-length keys sorted on 32-bit words."""
    if count <= XL_LEVEL:
        return "k_branch_xl"
    if count <= SMALL_LEVEL:
        return "k_branch_small"
    if segmented:
        return "k_branch_fused<2>"
    return "k_branch_fused<4>" if depth < 8 else "k_branch_fused<6>"


def _pack_nibbles(nib):
    return ((nib[:, 0::2] << 4) | nib[:, 1::2]).astype(np.uint8)


def _account_pool(rng, k=256):
    """k account bodies (codec.account_rlp: 70-odd bytes) as (blob, offsets)."""
    items = [codec.account_rlp(int(rng.integers(0, 1 << 16)), int(rng.integers(0, 10 ** 18)) * 10 ** 4)
             for _ in range(k)]
    off = np.zeros(k + 1, np.int64)
    off[1:] = np.cumsum([len(x) for x in items])
    return np.frombuffer(b"".join(items), np.uint8), off


def _one_byte_or_account(rng, n, p_small, p_big):
    """Per key a 1-byte value < 0x80 (p_small), a 1-byte value >= 0x80 (p_big) or an account
    body (the rest): (vals, voff)."""
    blob, poff = _account_pool(rng)
    u = rng.random(n)
    acct = u >= p_small + p_big
    pick = rng.integers(0, len(poff) - 1, n)
    lens = np.where(acct, poff[pick + 1] - poff[pick], 1).astype(np.int64)
    voff = np.zeros(n + 1, np.int64)
    voff[1:] = np.cumsum(lens)
    total = int(voff[-1])
    vals = np.zeros(total + 8, np.uint8)
    src = np.where(acct, poff[pick], 0)
    vals[:total] = blob[np.repeat(src - voff[:-1], lens) + np.arange(total)]
    one = np.where(u < p_small, rng.integers(1, 0x80, n), rng.integers(0x80, 0x100, n)).astype(np.uint8)
    vals[voff[:-1][~acct]] = one[~acct]
    return vals, voff.astype(np.uint64)


def _distinct_prefixes(rng, groups, depth):
    got = np.zeros((0, depth), np.uint8)
    while len(got) < groups:
        more = rng.integers(0, 16, (groups + groups // 4 + 16, depth), dtype=np.uint8)
        got = np.unique(np.concatenate([got, more]), axis=0)
    return got[rng.permutation(len(got))[:groups]]


def level_case(depth, groups, kind, seed):
    """`groups` distinct random prefixes of `depth` nibbles, under each of them c keys (c per
    group from CHILD_COUNTS) whose nibble at `depth` is distinct and whose other nibbles are
    random: exactly `groups` branches at depth `depth`, every other branch above them on the
    prefixes' own trie.  Kinds:

    long      values of LONG_LENS bytes mixed per key (leaves over 135 B: the long-leaf path);
    inline31  depth 8: a 1-byte value < 0x80 (31-byte leaf, inline), a 1-byte value >= 0x80
              (32 bytes, hashed) or an account body, mixed inside each branch;
    deep      depth 62: 1-byte values, seven in eight < 0x80 (3-byte leaves, else 4): inline
              branches of 18-31 bytes under hashed extensions, hashed ones from 32 bytes
              (six 3-byte children make 30 bytes, seven 32);
    nested    depth 60: a child slot holds a leaf or two keys that share nibbles 60 and 61 -- an
              inline 1-nibble extension over an inline depth-62 branch inside the depth-60 branch.
    """
    assert kind in KINDS and 0 < depth <= 62
    rng = np.random.default_rng([seed, depth, groups, KINDS.index(kind)])
    pre = _distinct_prefixes(rng, groups, depth)
    c = rng.choice(CHILD_COUNTS, groups)
    slot = rng.permuted(np.tile(np.arange(16, dtype=np.uint8), (groups, 1)), axis=1)
    used = np.arange(16)[None, :] < c[:, None]
    gid = np.repeat(np.arange(groups), c)
    child = slot[used]  # row-major: group by group, as gid
    if kind == "nested":
        assert depth <= 60
        twin = rng.random(len(gid)) < 0.5
        gid = np.concatenate([gid, gid[twin]])
        child = np.concatenate([child, child[twin]])
    n = len(gid)
    nib = rng.integers(0, 16, (n, 64), dtype=np.uint8)
    nib[:, :depth] = pre[gid]
    nib[:, depth] = child
    if kind == "nested":
        first = np.flatnonzero(twin)
        second = np.arange(n - len(first), n)
        nib[second, :depth + 2] = nib[first, :depth + 2]
        nib[second, depth + 2] = (nib[first, depth + 2] + rng.integers(1, 16, len(first))) & 15
    if kind == "long":
        lens = rng.choice(LONG_LENS, n).astype(np.int64)
        voff = np.zeros(n + 1, np.uint64)
        voff[1:] = np.cumsum(lens)
        vals = rng.integers(0, 256, int(voff[-1]) + 8, dtype=np.uint8)
    elif kind == "inline31":
        vals, voff = _one_byte_or_account(rng, n, 0.4, 0.3)
    else:
        vals, voff = _one_byte_or_account(rng, n, 0.875, 0.125)
    order = rng.permutation(n)
    keys = _pack_nibbles(nib)[order]
    vals, voff = _reorder_values(vals, voff, order)
    return f"{kind}_d{depth}_g{groups}_s{seed}", np.ascontiguousarray(keys).reshape(-1), vals, voff


def _reorder_values(vals, voff, order):
    """The packed values of keys taken in `order`."""
    vo = voff.astype(np.int64)
    lens = np.diff(vo)[order]
    new = np.zeros(len(order) + 1, np.int64)
    new[1:] = np.cumsum(lens)
    total = int(new[-1])
    out = np.zeros(total + 8, np.uint8)
    out[:total] = vals[np.repeat(vo[:-1][order] - new[:-1], lens) + np.arange(total)]
    return out, new.astype(np.uint64)


def _concat(a, b, name):
    """Case a followed by the keys and values of b."""
    na = len(a[3]) - 1
    ta, tb = int(a[3][-1]), int(b[3][-1])
    vals = np.concatenate([a[2][:ta], b[2][:tb], np.zeros(8, np.uint8)])
    voff = np.concatenate([a[3], b[3][1:] + a[3][-1]]).astype(np.uint64)
    assert len(voff) == na + len(b[3])
    return name, np.concatenate([a[1], b[1]]), vals, voff


def _words(keys):
    """The keys as n x 4 big-endian 64-bit words (numeric order == key order)."""
    return np.ascontiguousarray(keys, dtype=np.uint8).reshape(-1, 32).view(">u8").astype(np.uint64)


def _sorted_words(keys):
    w = _words(keys)
    return w[np.lexsort((w[:, 3], w[:, 2], w[:, 1], w[:, 0]))]


def _lcp_nibbles(w):
    """Common leading nibbles of adjacent rows of sorted words (64 for equal keys)."""
    x = w[1:] ^ w[:-1]
    nz = x != 0
    wi = np.argmax(nz, axis=1)
    v = x[np.arange(len(x)), wi]
    lz = np.zeros(len(x), np.int64)
    found = np.zeros(len(x), bool)
    for k in range(16):
        hit = ~found & (((v >> np.uint64(60 - 4 * k)) & np.uint64(15)) != 0)
        lz[hit] = k
        found |= hit
    return np.where(nz.any(axis=1), wi * 16 + lz, 64)


def level_histogram(keys):
    """Branches per depth (int64[64]) of the trie of the distinct keys.  A branch at depth d is a
    d-nibble prefix at which two keys part: the boundaries between adjacent sorted keys whose
    common prefix is d nibbles, counted once per distinct prefix -- two such boundaries belong to
    one branch exactly when no boundary between them is shallower than d."""
    lcp = _lcp_nibbles(_sorted_words(keys))
    lcp = lcp[lcp < 64]
    hist = np.zeros(64, np.int64)
    for d in np.unique(lcp):
        sub = lcp[lcp <= d]
        hist[d] = int(((sub == d) & (np.concatenate([[-1], sub[:-1]]) != d)).sum())
    return hist


def max_word_run(keys, seg_bits=0):
    """The longest run of (distinct) keys equal in the 32-bit word the device sorts: the leading
    32 key bits, or (segmented by the keys' own leading `seg_bits` bits) the leading 32 - seg_bits
    key bits under the segment id."""
    word = _sorted_words(keys)[:, 0] >> np.uint64(32 + seg_bits)
    brk = np.flatnonzero(np.concatenate([[True], word[1:] != word[:-1], [True]]))
    return int(np.diff(brk).max())


def pad_to(case, m, seed, keep_depth=None):
    """`case` followed by uniformly random keys, with values of one byte < 0x80 or account
    bodies, up to exactly m keys (distinct: tests/test_level_cases.py checks it).  With
    keep_depth, random keys that share their first keep_depth nibbles with any other key are
    drawn again, so the branch count of that level stays the case's."""
    name, keys, vals, voff = case
    rng = np.random.default_rng([seed, m])
    need = m - (len(voff) - 1)
    assert need >= 0 and (keep_depth is None or keep_depth <= 16)
    sh = np.uint64(64 - 4 * (keep_depth or 16))
    top_have = np.unique(_words(keys)[:, 0] >> sh)
    pad = np.zeros((0, 4), np.uint64)
    while len(pad) < need:
        more = _words(rng.integers(0, 256, ((need - len(pad)) * 9 // 8 + 16, 32), dtype=np.uint8))
        pad = np.concatenate([pad, more])
        if keep_depth is not None:
            top = pad[:, 0] >> sh
            u, cnt = np.unique(top, return_counts=True)
            pad = pad[~np.isin(top, np.union1d(top_have, u[cnt > 1]))]
    pad = pad[:need]
    pk = pad.astype(">u8").view(np.uint8).reshape(-1)
    pv, po = _one_byte_or_account(rng, need, 0.3, 0.0)
    return _concat(case, (None, pk, pv, po), f"{name}_pad{m}")


def cluster(nibbles, count, seed, lone=0):
    """`count` keys under one prefix (a list of nibbles), 1-byte values.  The last `lone` (up to
    3) of them stand alone under a next nibble of their own, so they are leaf children of the
    prefix's branch itself: the first with a value < 0x80, the second >= 0x80, the third with an
    account body; the others share the remaining next nibbles at random."""
    rng = np.random.default_rng([seed, count])
    d = len(nibbles)
    nib = rng.integers(0, 16, (count, 64), dtype=np.uint8)
    nib[:, :d] = np.asarray(nibbles, np.uint8)
    nib[:, d] = rng.integers(0, 16 - lone, count)
    nib[count - lone:, d] = np.arange(16 - lone, 16)
    keys = _pack_nibbles(nib)
    vals, voff = _one_byte_or_account(rng, count - lone, 0.7, 0.3)
    body = codec.account_rlp(1, 10 ** 18)
    tail = [b"\x05", b"\x85", body][:lone]
    case = f"cluster{count}", keys.reshape(-1), vals, voff
    if lone:
        lv = np.frombuffer(b"".join(tail) + b"\0" * 8, np.uint8)
        lo = np.concatenate([[0], np.cumsum([len(x) for x in tail])]).astype(np.uint64)
        case = _concat((case[0], keys[:count - lone].reshape(-1), vals, voff),
                       (None, keys[count - lone:].reshape(-1), lv, lo), case[0])
    return case


def by_segment(case, seg_bits):
    """The case cut into 2**seg_bits tries by the keys' leading bits: (seg uint32[n] in input
    order; the case regrouped by segment with seg_off uint64[nseg+1] for the CPU builders)."""
    name, keys, vals, voff = case
    k = keys.reshape(-1, 32)
    seg = (k[:, 0] >> (8 - seg_bits)).astype(np.uint32)
    order = np.argsort(seg, kind="stable")
    gv, go = _reorder_values(vals, voff, order)
    seg_off = np.searchsorted(seg[order], np.arange((1 << seg_bits) + 1)).astype(np.uint64)
    return seg, (name + f"_seg{1 << seg_bits}", np.ascontiguousarray(k[order]).reshape(-1), gv, go), seg_off


def leaf_lengths(case, depth):
    """Encoded length of every leaf hanging off a depth-`depth` branch (RLP list of the
    hex-prefix path of the 63 - depth nibbles left and the value)."""
    _, _, vals, voff = case
    vo = voff.astype(np.int64)
    vlen = np.diff(vo)
    v0 = vals[vo[:-1]]

    def rlp_str_len(ln, first):
        big = np.where(ln < 256, 2, 3)  # (lengths here stay under 65,536)
        return np.where((ln == 1) & (first < 0x80), 1, np.where(ln < 56, 1 + ln, big + ln))

    hp = (63 - depth) // 2 + 1  # flag nibble (+ pad) and the path; its first byte is 0x20 or 0x3n
    payload = rlp_str_len(np.int64(hp), 0x20) + rlp_str_len(vlen, v0)
    return np.where(payload < 56, 1, np.where(payload < 256, 2, 3)) + payload


# ---- the cases of tests/test_gpu_levels.py (tests/test_level_cases.py checks each of them)

ROWS = [  # (kind, groups, the kernel the depth-KIND_DEPTH[kind] level runs in)
    ("long", 8192, "k_branch_xl"), ("long", 8193, "k_branch_small"), ("long", 32768, "k_branch_small"),
    ("long", 32769, "k_branch_fused<4>"), ("long", 40000, "k_branch_fused<4>"),
    ("inline31", 8193, "k_branch_small"), ("inline31", 32768, "k_branch_small"),
    ("inline31", 32769, "k_branch_fused<6>"), ("inline31", 40000, "k_branch_fused<6>"),
    ("deep", 8193, "k_branch_small"), ("deep", 32769, "k_branch_fused<6>"),
    ("nested", 8193, "k_branch_small"), ("nested", 32769, "k_branch_fused<6>"),
]
SEED = 7
WIDE_PREFIX = (0xC, 0x0, 0xF, 0xF, 0xE, 0xE, 0x0, 0x1)
WIDE_KEYS = 6000
SEG_BITS = 6
TILE_SIZES = (TOPO_TILE_MIN, TOPO_TILE_MIN + 1, TOPO_TILE_MIN + 2)  # keys: boundaries + 1


@functools.lru_cache(maxsize=2)
def row_case(kind, groups):
    return level_case(KIND_DEPTH[kind], groups, kind, SEED)


def wide_case():
    """inline31 at 32,769 groups plus 6,000 keys under one more 8-nibble prefix: that prefix's
    branch sits in the large depth-8 level and spans more than 4,096 sorted positions; three
    of its children are leaves (31 bytes inline, 32 bytes hashed, an account), the others
    branches."""
    base = row_case("inline31", 32769)
    wide4 = _pack_nibbles(np.array([WIDE_PREFIX], np.uint8))[0]
    assert not (base[1].reshape(-1, 32)[:, :4] == wide4).all(axis=1).any()
    return _concat(base, cluster(WIDE_PREFIX, WIDE_KEYS, SEED, lone=3), base[0] + "_wide")


def tile_case(m):
    return pad_to(row_case("inline31", 40000), m, SEED, keep_depth=8)
