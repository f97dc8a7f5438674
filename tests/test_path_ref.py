"""CPU: the nodes-by-path reference (tests/path_ref.py) checks itself against the oracle's
reachable() node sets, and the query generator (tests/path_cases.py) yields every kind of query on
the inputs chosen for it."""
import random

import pytest

from tests import cases as C
from tests import export_cases, hostprog, path_cases, path_ref, proof_cases, proof_ref


def _fold(o, ups, dels):
    for k, v in ups:
        o.put(k, v)
    for k in dels:
        o.remove(k)


def _check_state(o):
    root = o.root_hash()
    nodes = o.reachable() if root != path_ref.EMPTY_ROOT else {}
    sp = path_ref.stored_paths(nodes, root)
    # every hash of reachable() is found, and exactly at the paths stored_paths gives
    assert {h for _, h in sp} == set(nodes)
    for path, h in sp:
        assert path_ref.node_at(nodes, root, path) == (1, nodes[h])
        assert proof_ref.kec(nodes[h]) == h
    # no other kind of query finds a node, and nothing is unknown on a whole set
    q = path_cases.queries(nodes, root, seed=len(nodes))
    at = {p for p, _ in sp}
    for kind, p in path_cases.flat(q):
        f, enc = path_ref.node_at(nodes, root, p)
        assert f == (1 if p in at else 0), (kind, p)
        if kind in ("empty_slot", "inside_ext", "below_leaf", "embedded", "mismatch"):
            assert f == 0, (kind, p)


@pytest.mark.parametrize("i", range(len(C.commit_scenarios())), ids=[s[0] for s in C.commit_scenarios()])
def test_reference_on_commit_scenarios(oracle, i):
    name, ks, vs, batches = C.commit_scenarios()[i]
    o = hostprog.trie(oracle, ks, vs)
    _check_state(o)
    for ups, dels in batches:
        _fold(o, ups, dels)
        _check_state(o)


def test_absent_hash_is_unknown(oracle):
    r = random.Random(5)
    ks = [C._rk(r) for _ in range(300)]
    o = hostprog.trie(oracle, ks, [C.account_value(r) for _ in ks])
    root, nodes = o.root_hash(), o.reachable()
    sp = path_ref.stored_paths(nodes, root)
    path, h = max(sp, key=lambda x: len(x[0]))
    part = {k: v for k, v in nodes.items() if k != h}
    assert path_ref.node_at(part, root, path) == (2, None)
    assert path_ref.node_at(part, root, path + (0,)) == (2, None)
    assert path_ref.node_at(part, root, path[:-1]) == (1, nodes[dict((p, x) for p, x in sp)[path[:-1]]])


def test_kinds_occur(oracle):
    """The kinds the device tests rely on are present in the inputs chosen for them."""
    ks, vs = export_cases.embedded_case()
    o = hostprog.trie(oracle, ks, vs)
    assert path_cases.queries(o.reachable(), o.root_hash())["embedded"]
    ks, vs, _ = proof_cases.ext_case()
    o = hostprog.trie(oracle, ks, vs)
    q = path_cases.queries(o.reachable(), o.root_hash())
    assert q["inside_ext"] and q["mismatch"]
    o, _ = hostprog.vb_trie(oracle)
    assert any(len(p) == 64 for p in path_cases.queries(o.reachable(), o.root_hash())["stored"])
    r = random.Random(300)
    ks = [C._rk(r) for _ in range(300)]
    o = hostprog.trie(oracle, ks, [C.account_value(r) for _ in ks])
    q = path_cases.queries(o.reachable(), o.root_hash())
    assert q["empty_slot"] and q["below_leaf"]


def test_compact_paths():
    """snap's wire form of a partial path (khipu_amd/codec.py)."""
    from khipu_amd import codec
    assert codec.path_to_compact([]) == b"\x00"
    assert codec.path_to_compact([1]) == b"\x11"
    assert codec.path_to_compact([1, 2]) == b"\x00\x12"
    assert codec.path_to_compact([1, 2, 3]) == b"\x11\x23"
    r = random.Random(9)
    for n in list(range(65)) * 2:
        p = [r.randrange(16) for _ in range(n)]
        b = codec.path_to_compact(p)
        assert codec.path_from_compact(b) == p and len(b) == 1 + n // 2
        assert codec.path32_to_nibbles(codec.nibbles_to_path32(p), n) == p
    for bad in (b"", b"\x20\x12", b"\x01", b"\x00" * 34):
        with pytest.raises(ValueError):
            codec.path_from_compact(bad)
