"""Ranges for the range-scan tests (tests/test_range_ref.py pins their conditions with the oracle
alone; tests/test_range_host.py and tests/test_gpu_range.py run them).  No GPU, no library."""
import random

from tests import fuzz_cases as F

ZERO, FF = b"\x00" * 32, b"\xff" * 32
MAXES = [1, 2, 3, 7, 50, 1000]
HOST_MAXES = [1, 2, 3, 15, 16, 17, 63, 64, 65, 257]


def _rk(r):
    return bytes(r.getrandbits(8) for _ in range(32))


def _step(k, d):
    """The key d above (below) k as a 256-bit number, clamped."""
    return min(max(int.from_bytes(k, "big") + d, 0), (1 << 256) - 1).to_bytes(32, "big")


def _point(r, keys):
    if keys and r.random() < 0.6:
        return _step(r.choice(keys), r.choice([-1, 0, 0, 1]))
    return _rk(r)


def random_ranges(r, keys, n=200):
    """n ranges (origin or None, limit or None, max_entries) over a trie holding `keys`: ends at,
    next to and between present keys, open ends, single keys, and a few with origin > limit."""
    keys = sorted(keys)
    out = []
    for _ in range(n):
        x = r.random()
        if x < 0.25:
            o, l = _point(r, keys), None
        elif x < 0.5:
            o, l = sorted([_point(r, keys), _point(r, keys)])
        elif x < 0.65:
            o, l = None, _point(r, keys)
        elif x < 0.8:
            k = _point(r, keys)
            o, l = (k, k) if r.random() < 0.5 else (_step(k, -1), _step(k, 1))
        elif x < 0.9:
            o, l = _rk(r), _rk(r)
        else:
            o, l = None, None
        out.append((o, l, r.choice(MAXES)))
    return out


def dense_case(seed=7, nkeys=160, npick=4):
    """(keys, vals, Keys, ranges): fuzz_cases' dense keys (branches only at the 17 split depths,
    every extension a gap between two of them) and, for npick keys, an origin and a limit one
    nibble either side of the key at each split depth."""
    r = random.Random(seed)
    K = F.Keys(r)
    keys = set()
    while len(keys) < nkeys:
        keys.add(K.key(r) if not keys or r.random() < 0.5 else K.sibling(r, r.choice(sorted(keys))))
    keys = sorted(keys)
    vals = [F.value(r) for _ in keys]
    ranges = []
    for k in r.sample(keys, npick):
        for p in K.P:
            for d in (-1, 1):
                n = F.nibbles(k)
                if not 0 <= n[p] + d <= 15:
                    continue
                n[p] += d
                b = F.from_nibbles(n)
                ranges.append((b, None, p))
                ranges.append((None, b, p))
                ranges.append((min(b, k), max(b, k), p))
    return keys, vals, K, ranges
