"""CPU: the order check and the count / fill boundary walk of khipu_amd/csrc/rangeverify.h
replayed on the host under AddressSanitizer and UBSan.  tests/rangeverify_host/rangeverify_check.cc
(a stand-alone program) runs every range of a case as ONE call over a shared node set, as
rangeverify_kernels.hip does up to the element build, into arrays of exactly the scanned sizes.
The kept lists, statuses, `more` and missing hashes must equal tests/rangeverify_ref.py's; a range
the plan leaves to the build is finished with the reference's builder over the program's kept list."""
import random
import subprocess

import pytest

from tests import cases as C
from tests import export_cases, hostprog, proof_cases
from tests import proof_ref as P
from tests import range_cases as RC
from tests import rangeverify_cases as VC
from tests import rangeverify_ref as VR
from tests.hostprog import hexs as _hex
from tests.hostprog import unhexs as _unhex

prog = hostprog.prog_fixture("rangeverify")


def _run(prog, tmp_path, nodes, ranges):
    """nodes: encodings; ranges: [(root, origin, keys, vals, proved)] -> per range
    (status, more, missing, inbuild, [(prefix nibbles, reference, side)])"""
    lines = [f"N {e.hex()}" for e in nodes]
    for root, origin, keys, vals, proved in ranges:
        ent = "".join(f" {k.hex()} {_hex(v)}" for k, v in zip(keys, vals))
        lines.append(f"R {root.hex()} {origin.hex()} {proved} {len(keys)}{ent}")
    p = tmp_path / "in.txt"
    p.write_text("\n".join(lines) + "\n")
    r = subprocess.run([prog, str(p)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])  # (a sanitizer report ends it with a non-zero status)
    out = [ln.split() for ln in r.stdout.split("\n")[:-1]]
    assert len(out) == len(ranges)
    ans = []
    for s, x in enumerate(out):
        assert x[0] == "A" and int(x[1]) == s
        n = int(x[6])
        kept = [(P.nibbles(bytes.fromhex(x[8 + 4 * j]))[:int(x[7 + 4 * j])], _unhex(x[9 + 4 * j]), int(x[10 + 4 * j]) - 1)
                for j in range(n)]
        assert all(not any(P.nibbles(bytes.fromhex(x[8 + 4 * j]))[int(x[7 + 4 * j]):]) for j in range(n))
        ans.append((int(x[2]), x[3] == "1", _unhex(x[4]) if x[4] != "-" else None, x[5] == "1", kept))
    return ans


def _check(prog, tmp_path, nodes, ranges, tag):
    """Every range against the reference; returns how many kept lists were compared and the statuses seen."""
    store = {P.kec(e): e for e in nodes}
    compared, seen = 0, set()
    for (root, origin, keys, vals, proved), (st, more, missing, inb, kept) in zip(ranges, _run(prog, tmp_path, nodes,
                                                                                              ranges)):
        want = VR.verify(store, root, origin, keys, vals, proved)
        if inb:
            assert st == VR.OK
            st = VR.OK if VR.rebuilt_root(keys, vals, kept) == root else VR.BAD_ROOT
            if proved:
                wst, _, _, wkept = VR.boundary_walk(store, root, origin, keys[-1] if keys else origin)
                assert wst == VR.OK and sorted(kept) == sorted(wkept), (tag, origin.hex(), len(keys))
                compared += 1
        assert st == want[0], (tag, origin.hex(), len(keys), st, want)
        if want[0] in (VR.OK, VR.INCOMPLETE):
            assert more == want[1], (tag, origin.hex(), len(keys))
        assert missing == want[2], (tag, origin.hex())
        seen.add(st)
    return compared, seen


def _flip(k, nib, d=1):
    n = P.nibbles(k)
    n[nib] = (n[nib] + d) % 16
    return bytes((n[2 * i] << 4) | n[2 * i + 1] for i in range(32))


def _ranges(o, origins, maxes):
    """Honest responses for every (origin, max_entries), the same without their entries, and a few
    tampers of each, all over the union of their nodes."""
    import random as _r
    from tests import range_ref as RR
    nodes, root = o.reachable(), o.root_hash()
    items = RR.content(nodes, root)
    r = _r.Random(17)
    encs, ranges = [], []
    for origin in origins:
        for mx in maxes:
            x = VC.response(items, nodes, root, origin, mx)
            encs += x["nodes"]
            ranges.append((root, origin, x["keys"], x["vals"], 1))
            ranges.append((root, origin, [], [], 1))
            for kind, t, proved, _ in VC.tampers(r, x, items, nodes, root):
                if not kind.startswith("withhold"):
                    encs += t["nodes"]
                    ranges.append((root, t["origin"], t["keys"], t["vals"], proved))
    return encs, ranges


def _two_keys(split):
    """Two keys that part at nibble `split`, and origins below both, between, on the second and
    above both -- each leaving the trie at a leaf, inside the extension above the branch (split > 0)
    and at an empty slot of the branch."""
    r = random.Random(40 + split)
    a = bytearray(C._rk(r))
    a[split >> 1] = 0x55
    a = bytes(a)
    b = _flip(a, split, 4)  # nibble 5 -> 9
    lo, hi = sorted([a, b])
    origins = [RC.ZERO, RC._step(lo, -1), lo, RC._step(lo, 1), RC._step(hi, -1), hi, RC._step(hi, 1), RC.FF]
    origins += [_flip(lo, split, -2), _flip(lo, split, 2), _flip(lo, split, 7)]            # empty slots: below, between, above
    origins += [_flip(lo, 63), _flip(hi, 63, -1), _flip(lo, split + 1), _flip(hi, split + 1, -1)]  # at a leaf
    if split:
        origins += [_flip(lo, 0, -1), _flip(lo, 0), _flip(lo, split - 1, -1), _flip(lo, split - 1)]  # leaves the extension
    return [lo, hi], [b"\x01" * 40, C.account_value(r)], origins


CASES = ["one_key", "two_keys_0", "two_keys_1", "two_keys_10", "two_keys_62", "random300", "embedded", "extension",
         "dense"]


@pytest.mark.parametrize("name", CASES)
def test_host_walks_match_the_reference(prog, tmp_path, oracle, name):
    r = random.Random(6)
    maxes = RC.HOST_MAXES
    if name == "one_key":
        ks, vs = [C._rk(r)], [b"\x07" * 40]
        origins = [RC.ZERO, RC._step(ks[0], -1), ks[0], RC._step(ks[0], 1), RC.FF, _flip(ks[0], 0), _flip(ks[0], 0, -1)]
    elif name.startswith("two_keys"):
        ks, vs, origins = _two_keys(int(name.split("_")[2]))
        maxes = [1, 2, 3]
    elif name == "random300":
        ks = [C._rk(r) for _ in range(300)]
        vs = [C.storage_value(r) if i % 3 else C.account_value(r) for i, _ in enumerate(ks)]
        origins = [RC._point(r, ks) for _ in range(12)] + [RC.ZERO, RC.FF]
    elif name == "embedded":
        ks, vs = export_cases.embedded_case()
        origins = [RC._point(r, ks) for _ in range(12)] + [RC.ZERO]
    elif name == "extension":
        ks, vs, qs = proof_cases.ext_case()
        origins = list(qs) + [RC._point(r, ks) for _ in range(8)] + [RC.ZERO, RC.FF]
    else:
        ks, vs, _, dense = RC.dense_case()
        origins = [a for a, b, _ in dense if b is None]
        maxes = [1, 3, 17]
    o = hostprog.trie(oracle, ks, vs)
    encs, ranges = _ranges(o, origins, maxes)
    compared, seen = _check(prog, tmp_path, encs, ranges, name)
    assert compared >= len(origins) and VR.OK in seen and VR.BAD_ROOT in seen
    if len(ks) > 1:
        assert {VR.BAD_ORDER, VR.INCOMPLETE} <= seen


def test_host_malformed_nodes_and_missing(prog, tmp_path, oracle):
    key = b"\x11" * 32
    ranges, encs = [], []
    for _, enc in proof_cases.malformed_nodes():
        encs.append(enc)
        ranges += [(P.kec(enc), key, [], [], 1), (P.kec(enc), key, [key], [b"v"], 1), (P.kec(enc), RC.ZERO, [key], [b"v"], 1)]
    got = _run(prog, tmp_path, encs, ranges)
    assert all(g[:4] == (VR.BAD_NODE, False, None, False) for g in got), got
    # a withheld node on each path, alone in its call; the empty trie; a root that is not there
    r = random.Random(8)
    ks = sorted(C._rk(r) for _ in range(120))
    vs = [C.account_value(r) for _ in ks]
    o = hostprog.trie(oracle, ks, vs)
    nodes, root = o.reachable(), o.root_hash()
    items = list(zip(ks, vs))
    n = 0
    for origin in (ks[30], RC._step(ks[60], 1)):
        x = VC.response(items, nodes, root, origin, 7)
        for kind, t, proved, exp in VC.tampers(r, x, items, nodes, root):
            if kind.startswith("withhold"):
                c, seen = _check(prog, tmp_path, t["nodes"], [(root, t["origin"], t["keys"], t["vals"], 1)], kind)
                assert seen == {VR.MISSING}
                n += 1
    assert n == 4
    E = P.EMPTY_ROOT
    _, seen = _check(prog, tmp_path, [], [(E, RC.ZERO, [], [], 1), (E, RC.ZERO, [], [], 0), (E, key, [], [], 1),
                                          (E, RC.ZERO, [key], [b"v"], 1), (E, RC.ZERO, [key], [b"v"], 0),
                                          (b"\x07" * 32, RC.ZERO, [], [], 1), (b"\x07" * 32, RC.ZERO, [], [], 0)], "empty")
    assert seen == {VR.OK, VR.BAD_ROOT, VR.MISSING}


def test_host_unproved_and_value_only_branch(prog, tmp_path, oracle):
    """Whole tries with proved = 0 beside proved ranges in one call, and the value-only branch: a
    boundary path that ends at it drops it like a leaf."""
    r = random.Random(9)
    ranges, encs = [], []
    for n in (1, 2, 17, 300):
        ks = sorted(C._rk(r) for _ in range(n))
        vs = [C.storage_value(r) for _ in ks]
        root = hostprog.trie(oracle, ks, vs).root_hash()
        ranges += [(root, RC.ZERO, ks, vs, 0), (root, RC.ZERO, ks[1:], vs[1:], 0)]
    o, _ = hostprog.vb_trie(oracle)
    from tests import range_ref as RR
    nodes, root = o.reachable(), o.root_hash()
    items = RR.content(nodes, root)
    ks0, _, blocks, _ = proof_cases.vb_case(False)
    for vbk in (blocks[0][0][0][0], ks0[-2]):
        at = [k for k, _ in items].index(vbk)
        for origin, mx in ((items[at - 2][0], 5), (RC.ZERO, at + 1), (vbk, 2), (RC._step(vbk, 1), 2), (items[at - 3][0], 2)):
            x = VC.response(items, nodes, root, origin, mx)
            encs += x["nodes"]
            ranges.append((root, origin, x["keys"], x["vals"], 1))
    compared, seen = _check(prog, tmp_path, encs, ranges, "vb")
    assert compared == 10 and seen == {VR.OK, VR.BAD_ROOT}
