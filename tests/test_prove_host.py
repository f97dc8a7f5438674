"""CPU: the proof walks of khipu_amd/csrc/prove.h replayed on the host under AddressSanitizer
and UBSan.  tests/prove_host/prove_check.cc (a stand-alone program) builds a trie's records
bottom-up, runs the count walk and the fill walk into arrays of exactly the counted size, encodes
every hit through export.h and feeds proofs -- its own, and mutated and malformed ones from its
input file -- to the verify walk.  The proofs must equal tests/proof_ref.expected_proof bit for
bit and the statuses tests/proof_ref.check_proof."""
import random
import subprocess

import pytest

from tests import cases as C
from tests import export_cases, hostprog, proof_cases
from tests import proof_ref as P
from tests.hostprog import hexs as _hex
from tests.hostprog import unhexs as _unhex


prog = hostprog.prog_fixture("prove")


def _run(prog, tmp_path, puts=(), queries=(), verifies=()):
    """verifies: [(root, key, [enc], idx or None)] -> (root, [(found, status, value, proof)], [(status, value)])"""
    lines = [f"P {k.hex()} {_hex(v)}" for k, v in puts] + [f"Q {k.hex()}" for k in queries]
    for root, key, encs, idx in verifies:
        lines.append(" ".join(["V", root.hex(), key.hex(), str(len(encs))] + [_hex(e) for e in encs]
                              + ([str(idx)] if idx is not None else [])))
    p = tmp_path / "in.txt"
    p.write_text("\n".join(lines) + "\n")
    r = subprocess.run([prog, str(p)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]  # (a sanitizer report ends the program with a non-zero status)
    out = [ln.split() for ln in r.stdout.split("\n")[:-1]]
    root = bytes.fromhex(out[0][1])
    q = [(x[1] == "1", int(x[2]), _unhex(x[3]), [_unhex(e) for e in x[5:5 + int(x[4])]]) for x in out if x[0] == "Q"]
    v = [(int(x[1]), _unhex(x[2])) for x in out if x[0] == "V"]
    assert len(q) == len(queries) and len(v) == len(verifies)
    return root, q, v


def _cases():
    r = random.Random(5)
    one = ([C._rk(r)], [b"\x07" * 40])
    ks = [C._rk(r) for _ in range(300)]
    rnd = (ks, [C.storage_value(r) if i % 3 else C.account_value(r) for i, _ in enumerate(ks)])
    ek, ev, eq = proof_cases.ext_case()
    return {"one_key": one + ([],), "random300": rnd + ([],), "embedded": export_cases.embedded_case() + ([],),
            "extension": (ek, ev, eq)}


@pytest.mark.parametrize("name", ["one_key", "random300", "embedded", "extension"])
def test_host_proofs_match_the_checker(prog, tmp_path, oracle, name):
    keys, vals, extra = _cases()[name]
    r = random.Random(17)
    o = oracle.Trie()
    for k, v in zip(keys, vals):
        o.put(k, v)
    have = set(keys)
    queries = list(keys[:120]) + list(extra) + [C._rk(r) for _ in range(20)]
    queries += [k for k in proof_cases.near_misses(r, keys, 16) if k not in have]
    root, got, _ = _run(prog, tmp_path, zip(keys, vals), queries)
    assert root == o.root_hash()
    nodes = o.reachable()
    for k, (found, status, value, proof) in zip(queries, got):
        want, val = P.expected_proof(nodes, root, k)
        assert proof == want, (name, k.hex())
        assert found == (o.get(k) is not None)
        assert (status, value if status == P.VALUE else None) == P.check_proof(root, k, proof) == \
            ((P.VALUE, val) if val is not None else (P.ABSENT, None)), (name, k.hex())
    if name == "embedded":  # a depth-64 leaf: its proof ends at the last hashed ancestor
        assert all(len(export_cases._items(p[-1])) == 17 for _, _, _, p in got[:40])


def test_host_empty_trie(prog, tmp_path):
    root, got, ver = _run(prog, tmp_path, [], [b"\x01" * 32], [(P.EMPTY_ROOT, b"\x01" * 32, [], None),
                                                             (b"\x02" * 32, b"\x01" * 32, [], None)])
    assert root == P.EMPTY_ROOT and got == [(False, P.ABSENT, b"", [])]
    assert [s for s, _ in ver] == [P.ABSENT, P.SHORT]


def test_host_malformed_nodes_are_bad_nodes(prog, tmp_path):
    key = b"\x11" * 32
    bad = proof_cases.malformed_nodes()
    ver = [(P.kec(enc), key, [enc], None) for _, enc in bad]
    leaf = bytes([0xF8, 34 + 41, 0xA1, 0x20]) + key + bytes([0xA8]) + b"\x09" * 40  # a valid single-leaf trie
    ver.append((P.kec(leaf), key, [leaf], None))
    ver.append((P.kec(leaf), key, [leaf], 1))  # a path index equal to n_nodes
    _, _, got = _run(prog, tmp_path, verifies=ver)
    for (name, _), (status, _) in zip(bad, got):
        assert status == P.BAD_NODE, name
    assert got[-2] == (P.VALUE, b"\x09" * 40) and got[-1][0] == P.BAD_NODE


def test_host_mutated_proofs_match_the_checker(prog, tmp_path, oracle):
    r = random.Random(23)
    keys = [C._rk(r) for _ in range(300)]
    o = oracle.Trie()
    for k in keys:
        o.put(k, C.storage_value(r) if r.random() < 0.5 else C.account_value(r))
    root, nodes = o.root_hash(), o.reachable()
    ver = []
    for m in range(300):
        key = r.choice(keys) if m % 3 else C._rk(r)
        proof = list(P.expected_proof(nodes, root, key)[0])
        op = m % 4
        if op == 0:
            j = r.randrange(len(proof))
            proof[j] = C.mutate(r, proof[j])
        elif op == 1:
            del proof[r.randrange(len(proof))]
        elif op == 2 and len(proof) > 1:
            a, b = r.sample(range(len(proof)), 2)
            proof[a], proof[b] = proof[b], proof[a]
        else:
            kb = bytearray(key)
            kb[r.randrange(32)] ^= 1 << r.randrange(8)
            key = bytes(kb)
        ver.append((root, key, proof, None))
    _, _, got = _run(prog, tmp_path, verifies=ver)
    seen = set()
    for (rt, key, proof, _), (status, value) in zip(ver, got):
        want = P.check_proof(rt, key, proof)
        assert (status, value if status == P.VALUE else None) == want, (key.hex(), [e.hex() for e in proof])
        seen.add(status)
    assert {P.ABSENT, P.BAD_HASH, P.SHORT}.issubset(seen), seen
