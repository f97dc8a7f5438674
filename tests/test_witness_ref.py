"""CPU: tests/witness_ref.expected (the commit witness from the node encodings and the key sets)
against hand cases with known answers, and bounded on the commit scenarios and the dense-key
sequences: it holds every path node of the op keys (fuzz_cases.path_set) and nothing the reference's
walk and fix could not load (partial_cases.fetchable)."""
import pytest

from tests import cases as C
from tests import fuzz_cases as F
from tests import partial_cases as P
from tests import witness_cases as WC
from tests import witness_ref
from tests import writeback as W
from tests.hostprog import trie


@pytest.mark.parametrize("case", WC.hand_cases(), ids=lambda c: c[0])
def test_hand_cases(oracle, case):
    name, ks, vs, ups, dels, cover, ncol = case
    o = trie(oracle, ks, vs)
    nodes, root = o.reachable(), o.root_hash()
    got, n = witness_ref.expected(nodes, root, ks, [k for k, _ in ups], dels)
    assert got == WC.want(nodes, root, cover), name
    assert n == ncol, name


def test_hand_case_shapes(oracle):
    """The fixtures are what their names say: the embedded case is one stored node, the sibling of
    the branch and extension cases is a branch resp. an extension referred to by hash."""
    by = {c[0]: c for c in WC.hand_cases()}
    _, ks, vs, *_ = by["embedded_sibling"]
    assert len(trie(oracle, ks, vs).reachable()) == 1
    for name, kind in (("sibling_branch", 17), ("sibling_extension", 2)):
        _, ks, vs, *_ = by[name]
        o = trie(oracle, ks, vs)
        nodes, root = o.reachable(), o.root_hash()
        sib = P.path_hashes(nodes, root, WC.B)[0][1]
        _, it = witness_ref.proof_ref.list_items(nodes[sib], 0, len(nodes[sib]))
        assert len(it) == kind and sib in P.hash_children(nodes[root])
        assert len(P.path_hashes(nodes, root, WC.B)[0]) == (3 if kind == 17 else 4)


def _bounded(nodes, root, live, ups, dels, tag):
    keys = [k for k, _ in ups] + list(dels)
    got, n = witness_ref.expected(nodes, root, live, [k for k, _ in ups], dels)
    paths = F.path_set(nodes, root, keys)
    assert got >= paths, tag
    assert got <= P.fetchable(nodes, root, keys), tag
    assert n == len(got - paths), tag
    return n


@pytest.mark.parametrize("sc", C.commit_scenarios(), ids=lambda s: s[0])
def test_bounds_on_commit_scenarios(oracle, sc):
    name, ks, vs, batches = sc
    o = trie(oracle, ks, vs)
    live = set(ks)
    total = 0
    for i, (ups, dels) in enumerate(batches):
        total += _bounded(W.reachable(o), o.root_hash(), live, ups, dels, (name, i))
        for k, v in ups:
            o.put(k, v)
        for k in dels:
            o.remove(k)
        live = (live | {k for k, _ in ups}) - set(dels)
    if name in ("storage", "to_empty", "large_batch"):
        assert total > 0, name  # (deletes that collapse branches onto untouched, hashed siblings)


@pytest.mark.parametrize("seed", F.TRIE_SEEDS[:3])
def test_bounds_on_dense_key_sequences(oracle, seed):
    pre, ncommit = None, 0
    for i, step, m in F.trie_run(seed, oracle, nsteps=30):
        if step["op"] == "commit" and not step["refused"]:
            nodes, root, live = pre
            _bounded(nodes, root, live, step["ups"], step["dels"], (seed, i))
            ncommit += 1
        pre = (dict(W.reachable(m.t)), m.root(), set(m.live))
    assert ncommit >= 3
