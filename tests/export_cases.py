"""Inputs shared by the node-export tests (tests/test_export_host.py on the CPU,
tests/test_gpu_export.py on the device)."""
import random


def embedded_case(seed=77):
    """40 keys in 10 groups of 4 that share 62 nibbles, pairs of them 63, with 1-byte values: the
    depth-64 leaves (3 B) embed in their depth-63 branches (22 B), which embed in the depth-62
    branch above them."""
    r = random.Random(seed)
    keys, vals = [], []
    for _ in range(10):
        base = bytearray(r.getrandbits(8) for _ in range(32))
        hi = r.sample(range(16), 2)
        for h in hi:
            for lo in r.sample(range(16), 2):
                b = bytearray(base)
                b[31] = (h << 4) | lo
                keys.append(bytes(b))
                vals.append(bytes([r.randrange(1, 0x80)]))
    return keys, vals


def _items(enc):
    """Top-level items of an RLP list: [(is_list, payload_offset, payload_len)]."""
    def head(p):
        b = enc[p]
        if b < 0x80:
            return False, p, 1
        if b < 0xB8:
            return False, p + 1, b - 0x80
        if b < 0xC0:
            nb = b - 0xB7
            return False, p + 1 + nb, int.from_bytes(enc[p + 1:p + 1 + nb], "big")
        if b < 0xF8:
            return True, p + 1, b - 0xC0
        nb = b - 0xF7
        return True, p + 1 + nb, int.from_bytes(enc[p + 1:p + 1 + nb], "big")
    is_list, p, n = head(0)
    assert is_list and p + n == len(enc)
    out, end = [], p + n
    while p < end:
        l, q, m = head(p)
        out.append((l, q, m))
        p = q + m
    return out


def holds_embedded_child(nodes):
    """Does any branch or extension of {hash: encoding} hold a list item (an embedded node) as a child?"""
    for enc in nodes.values():
        it = _items(enc)
        if len(it) == 17 and any(l for l, _, _ in it[:16]):
            return True
        if len(it) == 2 and it[1][0]:
            return True
    return False
