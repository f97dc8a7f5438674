"""CPU: the proof tests' own checker (tests/proof_ref.py) checked against the oracle trie, so the
yardstick of tests/test_prove_host.py and tests/test_gpu_prove.py is trusted: over every commit
scenario, embedded nodes, extensions and a value-only branch, check_proof(expected_proof(...))
gives VALUE with oracle.Trie.get's value for present keys and ABSENT for absent ones."""
import random

import pytest

from tests import cases as C
from tests import export_cases, proof_cases
from tests import proof_ref as P


def _check(o, present, absent):
    root = o.root_hash()
    nodes = o.reachable() if root != P.EMPTY_ROOT else {}
    for k in present:
        proof, val = P.expected_proof(nodes, root, k)
        assert val == o.get(k) and val is not None, k.hex()
        assert P.check_proof(root, k, proof) == (P.VALUE, val), k.hex()
        assert all(len(e) >= 32 for e in proof[1:])  # only the root may be shorter than a hash
    for k in absent:
        assert o.get(k) is None
        proof, val = P.expected_proof(nodes, root, k)
        assert val is None
        assert P.check_proof(root, k, proof) == (P.ABSENT, None), k.hex()


@pytest.mark.parametrize("i", range(len(C.commit_scenarios())), ids=[s[0] for s in C.commit_scenarios()])
def test_checker_over_commit_scenarios(oracle, i):
    name, ks, vs, batches = C.commit_scenarios()[i]
    r = random.Random(i)
    o = oracle.Trie()
    live = {}
    for k, v in zip(ks, vs):
        o.put(k, v)
        live[k] = v
    gone = []
    for b in range(len(batches) + 1):
        if b:
            for k, v in batches[b - 1][0]:
                o.put(k, v)
                live[k] = v
            for k in batches[b - 1][1]:
                o.remove(k)
                live.pop(k, None)
                gone.append(k)
        present = r.sample(list(live), min(len(live), 60))
        absent = [C._rk(r) for _ in range(20)] + [k for k in gone if k not in live]
        if present:
            absent += [k for k in proof_cases.near_misses(r, present) if k not in live]
        _check(o, present, absent)


def test_checker_embedded_extension_and_value_only_branch(oracle):
    ks, vs = export_cases.embedded_case()
    o = oracle.Trie()
    for k, v in zip(ks, vs):
        o.put(k, v)
    assert export_cases.holds_embedded_child(o.reachable())
    r = random.Random(3)
    _check(o, ks, [k for k in proof_cases.near_misses(r, ks, 16) if k not in set(ks)])
    proof, _ = P.expected_proof(o.reachable(), o.root_hash(), ks[0])
    assert len(export_cases._items(proof[-1])) == 17  # the depth-64 leaf is embedded: the proof ends at a branch
    # extensions, and keys that leave them
    ks, vs, queries = proof_cases.ext_case()
    o = oracle.Trie()
    for k, v in zip(ks, vs):
        o.put(k, v)
    _check(o, ks, queries)
    for q in queries:  # the extension is listed, nothing below it
        assert len(P.expected_proof(o.reachable(), o.root_hash(), q)[0]) == 1
    # the value-only branch, hashed and embedded
    for small in (False, True):
        ks, vs, blocks, (k1, k2, k3) = proof_cases.vb_case(small)
        o = oracle.Trie()
        for k, v in zip(ks, vs):
            o.put(k, v)
        for ups, dels in blocks:
            for k, v in ups:
                o.put(k, v)
            for k in dels:
                o.remove(k)
            kk = [k1, k2, k3]
            _check(o, [k for k in kk if o.get(k) is not None], [k for k in kk if o.get(k) is None])


def test_checker_statuses_on_tampered_proofs(oracle):
    r = random.Random(9)
    ks = [C._rk(r) for _ in range(300)]
    o = oracle.Trie()
    for k in ks:
        o.put(k, C.account_value(r))
    root, nodes = o.root_hash(), o.reachable()
    proof, val = P.expected_proof(nodes, root, ks[0])
    assert len(proof) >= 3
    bad = list(proof)
    bad[1] = bad[1][:5] + bytes([bad[1][5] ^ 1]) + bad[1][6:]
    assert P.check_proof(root, ks[0], bad)[0] == P.BAD_HASH
    assert P.check_proof(b"\x01" * 32, ks[0], proof)[0] == P.BAD_HASH
    assert P.check_proof(root, ks[0], proof[:-1])[0] == P.SHORT
    assert P.check_proof(root, ks[0], proof + [proof[0]])[0] == P.EXTRA
    assert P.check_proof(root, ks[0], []) == (P.SHORT, None)
    assert P.check_proof(P.EMPTY_ROOT, ks[0], []) == (P.ABSENT, None)
    for name, enc in proof_cases.malformed_nodes():
        assert P.check_proof(P.kec(enc), b"\x11" * 32, [enc]) == (P.BAD_NODE, None), name
