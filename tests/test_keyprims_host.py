"""CPU: the anchor key primitives of khipu_amd/csrc/forest.h -- prefix_word, prefix_eq, anchor_tag,
set_nibble -- run on the host by tests/keyprims_host/keyprims_check.cc (a stand-alone program) and
compared with a plain nibble-list reference for every depth 0..64: the cases at the 16-nibble words
(d == 16 q, d == 16 q + 16, d inside a word) that a resident anchor meets only with dense keys.  The
program runs twice: built plain, and built with AddressSanitizer and UBSan."""
import os
import random
import subprocess

import pytest

from tests import hostprog

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "keyprims_host", "keyprims_check.cc")
M64 = (1 << 64) - 1


def nibbles(key):
    return [x for b in key for x in (b >> 4, b & 15)]


def from_nibbles(n):
    return bytes((n[2 * i] << 4) | n[2 * i + 1] for i in range(32))


def lcp(a, b):
    na, nb = nibbles(a), nibbles(b)
    return next((i for i in range(64) if na[i] != nb[i]), 64)


def ref_prefix(key, d):
    """The key with every nibble from d on zeroed."""
    n = nibbles(key)
    return from_nibbles(n[:d] + [0] * (64 - d))


def _fmix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def ref_tag(t, d, key):
    """forest.h anchor_tag over the zero-extended prefix (its four words little-endian)."""
    p = ref_prefix(key, d)
    h = _fmix64(((t << 8) ^ d ^ 0x9E3779B97F4A7C15) & M64)
    for q in range(4):
        w = int.from_bytes(p[8 * q:8 * q + 8], "little")
        h = _fmix64(h ^ w ^ ((0x632BE59BD9B4E019 * (q + 1)) & M64))
    return h | 2


def _inputs():
    r = random.Random(64)
    a = bytes(r.getrandbits(8) for _ in range(32))
    zero, ff = b"\x00" * 32, b"\xff" * 32
    flipped = []
    for i in range(64):  # a key that differs from a at nibble i only: nibble d - 1, d and d + 1 of every d
        n = nibbles(a)
        n[i] ^= r.randrange(1, 16)
        flipped.append(from_nibbles(n))
    keys = [(0, a), (0, zero), (0, ff), (70000, a), (0xFFFFFFFF, zero), (1, ff)] + [(0, k) for k in flipped[::7]]
    pairs = [(a, k) for k in flipped] + [(k, a) for k in flipped[::5]] + [(a, a), (zero, ff), (zero, zero), (ff, ff)]
    for i in range(64):  # all-0 against a key whose only set nibble is i; all-f against its complement
        n = [0] * 64
        n[i] = 1 + i % 15
        pairs.append((zero, from_nibbles(n)))
        pairs.append((ff, from_nibbles([15 - x for x in n])))
    return keys, pairs, [a, zero, ff]


def _build(tmp, sanitize):
    if sanitize:
        return hostprog.compile_prog(SRC, tmp / "keyprims_check_san")
    return hostprog.compile_prog(SRC, tmp / "keyprims_check", ["-O2", "-std=c++17"])


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "sanitized"])
def out(request, tmp_path_factory):
    keys, pairs, sets = _inputs()
    text = "".join(f"K {t} {k.hex()}\n" for t, k in keys) + "".join(f"P {a.hex()} {b.hex()}\n" for a, b in pairs)
    text += "".join(f"S {k.hex()}\n" for k in sets)
    exe = _build(tmp_path_factory.mktemp("keyprims"), request.param)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]  # (a sanitizer report ends the program with a non-zero status)
    rows = [ln.split() for ln in r.stdout.split("\n") if ln]
    return dict(K=[x for x in rows if x[0] == "K"], P=[x for x in rows if x[0] == "P"], S=[x for x in rows if x[0] == "S"])


def test_prefix_word_and_tag(out):
    keys, _, _ = _inputs()
    assert len(out["K"]) == 65 * len(keys)
    tags = {}
    for x in out["K"]:
        i, d = int(x[1]), int(x[2])
        t, k = keys[i]
        assert "".join(x[3:7]) == ref_prefix(k, d).hex(), ("prefix_word", i, d)
        assert int(x[7], 16) == ref_tag(t, d, k), ("anchor_tag", i, d)
        tags[(i, d)] = int(x[7], 16)
    assert all(g >= 2 for g in tags.values())  # 0 and 1 mark empty slots and tombstones
    # the depth is part of the tag: a key whose nibble d is 0 has equal prefixes at d and d + 1
    for d in range(64):
        assert tags[(1, d)] != tags[(1, d + 1)], d
    # and so is the trie id
    assert all(tags[(0, d)] != tags[(3, d)] for d in range(65))


def test_prefix_eq_holds_exactly_up_to_the_common_prefix(out):
    _, pairs, _ = _inputs()
    assert len(out["P"]) == len(pairs)
    for x in out["P"]:
        a, b = pairs[int(x[1])]
        l = lcp(a, b)
        assert x[2] == "".join("1" if d <= l else "0" for d in range(65)), (a.hex(), b.hex(), l)


def test_set_nibble(out):
    _, _, sets = _inputs()
    assert len(out["S"]) == 64 * 16 * len(sets)
    for x in out["S"]:
        k, i, v = sets[int(x[1])], int(x[2]), int(x[3])
        n = nibbles(k)
        n[i] = v
        assert x[4] == from_nibbles(n).hex(), (x[1], i, v)
