"""Inputs shared by the proof tests (tests/test_proof_ref.py and tests/test_prove_host.py on the
CPU, tests/test_gpu_prove.py on the device)."""
import random

from tests import cases as C


def ext_case(seed=91, n=50, shared=10):
    """n keys sharing their first `shared` nibbles (an extension at the root), account values;
    returns (keys, vals, queries): queries leave the shared path at nibbles 1, 5 and 9."""
    r = random.Random(seed)
    base = C._rk(r)
    keys = []
    for _ in range(n):
        k = bytearray(C._rk(r))
        k[:shared // 2] = base[:shared // 2]
        keys.append(bytes(k))
    vals = [C.account_value(r) for _ in keys]
    queries = []
    for nib in (1, 5, 9):
        q = bytearray(keys[nib])
        q[nib >> 1] ^= 0x10 if nib % 2 == 0 else 0x01
        queries.append(bytes(q))
    return keys, vals, queries


def near_misses(r, present, count=8):
    """Keys sharing 60-63 nibbles with a present key and differing at the next one."""
    out = []
    for i in range(count):
        k = bytearray(r.choice(present))
        nib = 60 + i % 4
        k[nib >> 1] ^= (0x10 if nib % 2 == 0 else 0x01) << r.randrange(4)
        for j in range(nib + 1, 64):  # (the rest random)
            k[j >> 1] ^= r.randrange(16) << (4 if j % 2 == 0 else 0)
        out.append(bytes(k))
    return out


def vb_case(small):
    """The construction of test_gpu_export.py::test_export_value_only_branch: (keys, vals, blocks,
    (k1, k2, k3)); a re-put of k1 under a depth-63 branch makes khipu's value-only branch."""
    r = random.Random(64 if small else 63)
    val = (lambda: bytes([r.randrange(1, 0x80)])) if small else (lambda: C.account_value(r))

    def pair():
        k1 = bytearray(C._rk(r))
        k2 = bytearray(k1)
        k2[31] ^= 0x01
        return bytes(k1), bytes(k2)
    k1, k2 = pair()
    k3 = bytearray(k1)
    k3[31] = (k3[31] & 0x0F) | (((k3[31] >> 4) ^ 0x3) << 4)
    k3 = bytes(k3)
    q1, q2 = pair()
    others = [C._rk(r) for _ in range(300)]
    ks = others + [k1, k2, q1, q2]
    vs = [val() for _ in ks]
    blocks = [([(k1, val()), (others[0], val()), (q1, val())], []),
              ([(k1, val())], [others[1]]),
              ([(others[3], val())], [k2]),
              ([(k3, val())], []),
              ([(k1, val()), (q1, val())], [others[4]]),
              ([], [k3])]
    return ks, vs, blocks, (k1, k2, k3)


def malformed_nodes():
    """(name, encoding): each not a well-formed trie node on the walk of key 0x11 * 32, as a
    single-node proof under root kec256(encoding)."""
    def s(b):
        return bytes([0x80 + len(b)]) + b if len(b) != 1 or b[0] >= 0x80 else b

    def lst(items):
        p = b"".join(items)
        return (bytes([0xC0 + len(p)]) if len(p) < 56 else bytes([0xF8, len(p)]) if len(p) < 256
                else bytes([0xF9, len(p) >> 8, len(p) & 255])) + p
    empty = b"\x80"
    h = s(b"\x77" * 32)
    out = [("byte_string", s(b"\x05" * 40)),
           ("empty_list", b"\xc0"),
           ("three_items", lst([s(b"\x20" + b"\x11" * 32), s(b"ab"), s(b"cd")])),
           ("child_31_bytes", lst([empty, s(b"\x33" * 31)] + [empty] * 15)),
           ("long_prefix_past_end", b"\xf9\x40\x00" + b"\x80" * 40),
           ("hp_flag_4", lst([s(b"\x40" + b"\x11" * 32), s(b"value" * 8)])),
           ("ext_65_nibbles", lst([s(b"\x11" + b"\x11" * 32), h])),
           ("leaf_past_nibble_64", lst([s(b"\x31" + b"\x11" * 32), s(b"value" * 8)]))]
    # a 17-item list whose child list (slot 15) claims 8 bytes where its parent has 3 left
    items = [empty] * 15 + [b"\xc8\x01\x02", empty]
    out.append(("child_list_overruns", lst(items)))
    return out
