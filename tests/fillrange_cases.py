"""Shapes for the range-fill tests (tests/test_fillrange_ref.py pins them on the CPU,
tests/test_fillrange_host.py replays the span test, tests/test_gpu_fillrange.py runs them).  No
GPU, no library: pages are cut from the sorted content and carry the nodes of
tests/proof_ref.expected_proof for their two boundary keys, as a serving handle's range_proof does.

crafted() is the smallest state in which every path of a fill can go wrong:
  - every key starts with the byte a5: the root node is an extension;
  - groups sharing 62 and 63 nibbles, with 1-byte values (embedded leaves, and depth-62/63
    branches short enough to be embedded themselves) and with 40-byte values (hashed leaves under a
    depth-63 branch: a re-delivered one must stay a leaf);
  - EXT_GROUP: keys alone under a5 77 that share the 8 nibbles a5 77 77 77, so an extension sits
    below the top branch; EXT_ORIGIN diverges inside that extension's path, below all of its keys,
    so its proof ends at the extension and leaves a stub whose missing node is known to be a branch.
"""
import random

from tests import proof_ref as P

ZERO, FF = b"\x00" * 32, b"\xff" * 32
EXT_PREFIX = bytes.fromhex("a5777777")
EXT_ORIGIN = bytes.fromhex("a5777770") + b"\x00" * 28
PAGES = (7, 64)


def crafted(seed=2024, n=300):
    r = random.Random(seed)
    items = {}

    def rnd_val():
        return bytes(r.getrandbits(8) for _ in range(r.choice((33, 40, 70))))

    while len(items) < n - 40:
        k = b"\xa5" + bytes(r.getrandbits(8) for _ in range(31))
        if k[1] != 0x77:
            items[k] = rnd_val()
    for _ in range(6):  # the extension group
        items[EXT_PREFIX + bytes(r.getrandbits(8) for _ in range(28))] = rnd_val()
    for j in range(4):  # 63 shared nibbles: the last nibble differs
        base = b"\xa5" + bytes([0x10 + j]) + bytes(r.getrandbits(8) for _ in range(29))
        for x in (0x31, 0x37, 0x3c):
            items[base + bytes([x])] = bytes([1 + j]) if j < 2 else rnd_val()
    for j in range(4):  # 62 shared nibbles: the last byte's high nibble differs
        base = b"\xa5" + bytes([0x90 + j]) + bytes(r.getrandbits(8) for _ in range(29))
        for x in (0x10, 0x25, 0xe0):
            items[base + bytes([x])] = bytes([0x7f - j]) if j < 2 else rnd_val()
    return sorted(items.items())


def step(k, d=1):
    """The key d above k (k + 1: where a sync continues after its last key)."""
    return ((int.from_bytes(k, "big") + d) % (1 << 256)).to_bytes(32, "big")


def page(items, nodes, root, origin, max_entries):
    """The honest page for (origin, max_entries): (keys, vals, proof encodings, more)."""
    inr = [(k, v) for k, v in items if k >= origin]
    cut = inr[:max_entries]
    keys, vals = [k for k, _ in cut], [v for _, v in cut]
    proof = P.expected_proof(nodes, root, origin)[0] + P.expected_proof(nodes, root, keys[-1] if keys else FF)[0]
    return keys, vals, proof, len(inr) > len(cut)


def walk_origins(items, size, first=ZERO):
    """The origins of a sync from `first` in pages of `size`: each continues at the last key + 1."""
    out, o = [], first
    while True:
        inr = [k for k, _ in items if k >= o]
        out.append(o)
        if len(inr) <= size:
            return out
        o = step(inr[size - 1])


def mutations(r, items, origin, keys, vals, j):
    """[(kind, keys, vals, expected status)] of a page tampered with at its entry j, 0 < j < m - 1, a
    key the receiving handle does not hold yet (a fill vouches for the handle: it cannot see that a
    key it already held was left out).  BAD_ORDER is 1, BAD_ROOT 4."""
    present = {k for k, _ in items}
    v = bytearray(vals[j])
    v[r.randrange(len(v))] ^= 1 << r.randrange(8)
    out = [
        ("drop_middle", keys[:j] + keys[j + 1:], vals[:j] + vals[j + 1:], 4),
        ("flip_value", keys, vals[:j] + [bytes(v)] + vals[j + 1:], 4),
        ("swap", keys[:j] + [keys[j + 1], keys[j]] + keys[j + 2:], vals[:j] + [vals[j + 1], vals[j]] + vals[j + 2:], 1),
        ("empty_value", keys, vals[:j] + [b""] + vals[j + 1:], 1),
    ]
    mid = step(keys[j])
    if mid < keys[j + 1] and mid not in present:
        out.append(("invent", keys[:j + 1] + [mid] + keys[j + 1:], vals[:j + 1] + [b"\x05" * 33] + vals[j + 1:], 4))
    if origin != ZERO:
        out.append(("below_origin", [step(origin, -1)] + keys, [b"\x01"] + vals, 1))
    return out
