"""CPU: the model of the range-fill tests (tests/fillrange_ref.py) against the oracle and against
the range-verification reference (tests/rangeverify_ref.py), over the shapes of
tests/fillrange_cases.py.  A sync walked by the model from a root-only handle ends holding exactly
oracle.Trie.reachable(); every page it accepts the range verifier accepts too; every tampered page
is rejected by both."""
import random

import pytest

from tests import fillrange_cases as FC
from tests import fillrange_ref as F
from tests import proof_ref as P
from tests import rangeverify_ref as RV


@pytest.fixture(scope="module")
def state(oracle):
    items = FC.crafted()
    o = oracle.Trie()
    for k, v in items:
        o.put(k, v)
    return items, o.reachable(), o.root_hash()


def test_crafted_shapes(state):
    items, nodes, root = state
    assert F._decode(nodes[root])[0] == "ext"  # an extension at the root
    keys = [k for k, _ in items]
    lcp = [next(i for i in range(65) if i == 64 or P.nibbles(a)[i] != P.nibbles(b)[i]) for a, b in zip(keys, keys[1:])]
    assert 62 in lcp and 63 in lcp
    # embedded leaves: a stored node that holds a list item
    assert any(any(it[0] for it in P.list_items(e, 0, len(e))[1]) for e in nodes.values())
    # the origin inside the extension: its proof ends at the extension, whose branch becomes a stub
    held = F.fill_nodes(nodes, root, {root}, P.expected_proof(nodes, root, FC.EXT_ORIGIN)[0])
    ext = [(p, h) for p, h in F.stubs(nodes, root, held) if p == P.nibbles(FC.EXT_PREFIX)]
    assert len(ext) == 1 and F._decode(nodes[ext[0][1]])[0] == "branch"
    assert F.inside(ext[0][0], P.nibbles(FC.EXT_ORIGIN), P.nibbles(FC.FF))
    assert not F.inside(ext[0][0], P.nibbles(FC.step(FC.EXT_PREFIX + b"\x00" * 28)), P.nibbles(FC.FF))


@pytest.mark.parametrize("size", FC.PAGES)
def test_a_walk_ends_with_the_whole_trie_and_agrees_with_the_verifier(state, size):
    items, nodes, root = state
    r = random.Random(size)
    held, n_keys, tampered = {root}, 0, 0
    origins = FC.walk_origins(items, size, FC.EXT_ORIGIN) + FC.walk_origins(items, size)
    for origin in origins:
        keys, vals, proof, _ = FC.page(items, nodes, root, origin, size)
        pn = {P.kec(e): e for e in proof}
        held = F.fill_nodes(nodes, root, held, proof)
        fresh = [j for j in range(1, len(keys) - 1) if F._walk_key(nodes, root, held, P.nibbles(keys[j]))[0] == "stub"]
        if fresh:
            for kind, mk, mv, want in FC.mutations(r, items, origin, keys, vals, r.choice(fresh)):
                assert F.fill_range(nodes, root, held, origin, mk, mv).status == want, kind
                assert RV.verify(pn, root, origin, mk, mv)[0] == want, kind
                tampered += 1
        res = F.fill_range(nodes, root, held, origin, keys, vals)
        assert res.status == F.OK and RV.verify(pn, root, origin, keys, vals)[0] == RV.OK
        assert res.n_keys == F.keys_held(nodes, root, res.held) - F.keys_held(nodes, root, held)
        assert res.n_stubs == len(F.stubs(nodes, root, held)) - len(F.stubs(nodes, root, res.held))
        # the same page again: nothing left to gain
        again = F.fill_range(nodes, root, res.held, origin, keys, vals)
        assert (again.status, again.n_keys, again.n_stubs) == (F.OK, 0, 0)
        held, n_keys = res.held, n_keys + res.n_keys
    # (the boundary proofs bring their own leaves: the fills gain the rest)
    assert held == set(nodes) and F.stubs(nodes, root, held) == []
    assert 0 < n_keys <= len(items) == F.keys_held(nodes, root, held)
    assert tampered >= 20


def test_refusals_of_the_model(state):
    items, nodes, root = state
    keys, vals, proof, _ = FC.page(items, nodes, root, FC.ZERO, 64)
    # without the proof the entries run into the root-only handle's stub, which is not inside
    res = F.fill_range(nodes, root, {root}, FC.ZERO, keys, vals)
    assert res.status == F.MISSING and len(res.missing) == 1 and res.held == {root}
    held = F.fill_nodes(nodes, root, {root}, proof)
    # no entries, stubs at or after the origin; none past the last key's successor of a whole trie
    assert F.fill_range(nodes, root, held, FC.ZERO, [], []).status == F.INCOMPLETE
    assert F.fill_range(nodes, root, set(nodes), FC.step(items[-1][0]), [], []).status == F.OK
    # every key of one inside stub left out
    ins = [p for p, _ in F.stubs(nodes, root, held) if F.inside(p, [0] * 64, P.nibbles(keys[-1]))]
    gone = [k for k in keys if P.nibbles(k)[:len(ins[0])] == ins[0]]
    assert gone and len(gone) < len(keys)
    kept = [(k, v) for k, v in zip(keys, vals) if k not in gone]
    assert F.fill_range(nodes, root, held, FC.ZERO, [k for k, _ in kept], [v for _, v in kept]).status == F.BAD_ROOT
    assert F.whole(root, [k for k, _ in items], [v for _, v in items]) == F.OK
    assert F.whole(root, [k for k, _ in items[1:]], [v for _, v in items[1:]]) == F.BAD_ROOT
