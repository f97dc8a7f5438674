"""CPU: the range-verification reference (tests/rangeverify_ref.py) on every state of
cases.commit_scenarios() -- every honest response of tests/rangeverify_cases.py is OK with the
`more` of range_ref.Snapshot, every tamper gets the status the contract assigns to its kind -- and
the conditions of the generators, so the host and device tests that run them cannot pass emptily."""
import random

import pytest

from tests import cases as C
from tests import proof_cases
from tests import proof_ref as P
from tests import range_cases as RC
from tests import range_ref as RR
from tests import rangeverify_cases as VC
from tests import rangeverify_ref as VR

SCEN = C.commit_scenarios()


def _nodes(o):
    return o.reachable() if o.root_hash() != P.EMPTY_ROOT else {}


def states(oracle, i):
    """(batch index, node store, root, content) after the open and after every batch of scenario i."""
    _, ks, vs, batches = SCEN[i]
    o = oracle.Trie()
    for k, v in zip(ks, vs):
        o.put(k, v)
    yield 0, _nodes(o), o.root_hash(), RR.content(_nodes(o), o.root_hash())
    for b, (ups, dels) in enumerate(batches):
        for k, v in ups:
            o.put(k, v)
        for k in dels:
            o.remove(k)
        yield b + 1, _nodes(o), o.root_hash(), RR.content(_nodes(o), o.root_hash())


def _store(encs):
    return {P.kec(e): e for e in encs}


def _verify(root, resp, proved=1):
    return VR.verify(_store(resp["nodes"]), root, resp["origin"], resp["keys"], resp["vals"], proved)


@pytest.mark.parametrize("i", range(len(SCEN)), ids=[s[0] for s in SCEN])
def test_honest_and_tampered_responses(oracle, i):
    kinds = set()
    for b, nodes, root, items in states(oracle, i):
        snap = RR.Snapshot(nodes, root)
        r = VC.seed(i, b)
        resps = VC.responses(r, items, nodes, root)
        assert len(resps) == VC.N_RESPONSES
        for resp in resps:
            page = snap.expected_range(resp["origin"], None, max(len(resp["keys"]), 1))
            if resp["keys"]:
                assert page[1] == resp["keys"] and page[3] == resp["more"]
            assert _verify(root, resp) == (VR.OK, resp["more"], None), (SCEN[i][0], b, resp["origin"].hex())
            for kind, t, proved, (st, more, missing) in VC.tampers(r, resp, items, nodes, root):
                got = _verify(root, t, proved)
                assert got[0] == st, (SCEN[i][0], b, kind, got)
                assert more is None or got[1] == more, (SCEN[i][0], b, kind)
                assert missing is None or got[2] == missing, (SCEN[i][0], b, kind)
                kinds.add(kind)
        # the whole content unproved is OK; minus one entry it is not
        ks, vs = [k for k, _ in items], [v for _, v in items]
        assert VR.verify({}, root, None, ks, vs, 0) == (VR.OK, False, None)
        if items:
            j = r.randrange(len(items))
            assert VR.verify({}, root, None, ks[:j] + ks[j + 1:], vs[:j] + vs[j + 1:], 0)[0] == VR.BAD_ROOT
    if SCEN[i][0] in ("accounts", "storage", "deep"):
        assert len(kinds) == 13, sorted(kinds)


@pytest.mark.parametrize("i", range(len(SCEN)), ids=[s[0] for s in SCEN])
def test_responses_keep_subtrees_on_both_sides(oracle, i):
    """On every state of at least 8 entries, at least 8 of the 40 responses have an entry, more = 1
    and a key below origin all at once (the minimum over the scenarios is 10 of 40)."""
    for b, nodes, root, items in states(oracle, i):
        if len(items) < 8:
            continue
        resps = VC.responses(VC.seed(i, b), items, nodes, root)
        assert sum(1 for x in resps if VC.busy(x, items)) >= 8, (SCEN[i][0], b)


def test_empty_trie():
    assert VR.verify({}, P.EMPTY_ROOT, None, [], [], 1) == (VR.OK, False, None)
    assert VR.verify({}, P.EMPTY_ROOT, None, [], [], 0) == (VR.OK, False, None)
    assert VR.verify({}, P.EMPTY_ROOT, b"\x55" * 32, [], [], 1) == (VR.OK, False, None)
    assert VR.verify({}, P.EMPTY_ROOT, None, [b"\x01" * 32], [b"v"], 1)[0] == VR.BAD_ROOT
    assert VR.verify({}, P.EMPTY_ROOT, None, [b"\x01" * 32], [b"v"], 0)[0] == VR.BAD_ROOT
    # a root that is not in the node set
    assert VR.verify({}, b"\x07" * 32, None, [], [], 1) == (VR.MISSING, False, b"\x07" * 32)
    assert VR.verify({}, b"\x07" * 32, None, [], [], 0)[0] == VR.BAD_ROOT


def test_no_entries_with_keys_after_origin_is_incomplete(oracle):
    r = random.Random(3)
    ks = sorted(C._rk(r) for _ in range(50))
    vs = [C.account_value(r) for _ in ks]
    o = oracle.Trie()
    for k, v in zip(ks, vs):
        o.put(k, v)
    nodes, root = o.reachable(), o.root_hash()
    for origin in (RC.ZERO, ks[10], RC._step(ks[10], 1), ks[-2]):
        resp = VC.response(list(zip(ks, vs)), nodes, root, origin, 1000)
        assert _verify(root, resp) == (VR.OK, False, None)
        assert _verify(root, dict(resp, keys=[], vals=[])) == (VR.INCOMPLETE, True, None)
    # the only key left is origin itself: nothing lies above it, and the rebuild misses its leaf
    resp = VC.response(list(zip(ks, vs)), nodes, root, ks[-1], 1000)
    assert _verify(root, resp) == (VR.OK, False, None)
    assert _verify(root, dict(resp, keys=[], vals=[])) == (VR.BAD_ROOT, False, None)
    resp = VC.response(list(zip(ks, vs)), nodes, root, RC._step(ks[-1], 1), 5)
    assert resp["keys"] == [] and _verify(root, resp) == (VR.OK, False, None)


def test_value_only_branch_limit(oracle):
    """A range whose inside holds khipu's value-only branch cannot be expressed by entries:
    BAD_ROOT; a range that ends below it is OK."""
    ks, vs, blocks, (k1, k2, k3) = proof_cases.vb_case(False)
    o = oracle.Trie()
    for k, v in zip(ks, vs):
        o.put(k, v)
    for k, v in blocks[0][0]:
        o.put(k, v)
    nodes, root = o.reachable(), o.root_hash()
    items = RR.content(nodes, root)
    keys = [k for k, _ in items]
    at = keys.index(min(k1, ks[-2]))  # (blocks[0] re-puts k1 and q1 = ks[-2]: two value-only branches)
    k1 = keys[at]
    assert at > 3
    around = VC.response(items, nodes, root, keys[at - 2], 5)
    assert k1 in around["keys"] and _verify(root, around)[0] == VR.BAD_ROOT
    below = VC.response(items, nodes, root, RC.ZERO, at - 1)
    assert k1 not in below["keys"] and _verify(root, below) == (VR.OK, True, None)
    # (ending ON the value-only branch's key: the range is inclusive, so it is inside as well)
    upto = VC.response(items, nodes, root, RC.ZERO, at + 1)
    assert upto["keys"][-1] == k1 and _verify(root, upto)[0] == VR.BAD_ROOT


def test_dense_origins_cover_every_split_depth(oracle):
    keys, vals, K, ranges = RC.dense_case()
    o = oracle.Trie()
    for k, v in zip(keys, vals):
        o.put(k, v)
    nodes, root = o.reachable(), o.root_hash()
    items = sorted(zip(keys, vals))
    origins = [(o_, p) for o_, l_, p in ranges if l_ is None]
    assert {p for _, p in origins} == set(K.P) and len(K.P) == 17
    for origin, _ in origins:
        for mx in (1, 3, 1000):
            resp = VC.response(items, nodes, root, origin, mx)
            assert _verify(root, resp) == (VR.OK, resp["more"], None)
