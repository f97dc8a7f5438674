"""CPU: the range-scan reference (tests/range_ref.py) pinned against oracle.Trie.get over every
key ever put, on every state of cases.commit_scenarios(); and the conditions of the generators in
tests/range_cases.py checked with the oracle alone, so the host and device tests that run them
cannot pass emptily."""
import random

import pytest

from tests import cases as C
from tests import export_cases, proof_cases
from tests import proof_ref as P
from tests import range_cases as RC
from tests import range_ref as RR

SCEN = C.commit_scenarios()


def _nodes(o):
    return o.reachable() if o.root_hash() != P.EMPTY_ROOT else {}


def _states(oracle, i):
    """(batch index, oracle trie, every key put so far) after the open and after every batch."""
    _, ks, vs, batches = SCEN[i]
    o = oracle.Trie()
    ever = set(ks)
    for k, v in zip(ks, vs):
        o.put(k, v)
    yield 0, o, ever
    for b, (ups, dels) in enumerate(batches):
        for k, v in ups:
            o.put(k, v)
            ever.add(k)
        for k in dels:
            o.remove(k)
        yield b + 1, o, ever


@pytest.mark.parametrize("i", range(len(SCEN)), ids=[s[0] for s in SCEN])
def test_walk_is_the_oracles_content(oracle, i):
    r = random.Random(500 + i)
    for b, o, ever in _states(oracle, i):
        nodes, root = _nodes(o), o.root_hash()
        want = sorted((k, o.get(k)) for k in ever if o.get(k) is not None)
        assert RR.content(nodes, root) == want, (SCEN[i][0], b)
        # paging by next with a small val_cap ends at the same content
        got, origin = [], None
        for _ in range(len(want) + 2):
            page = RR.expected_range(nodes, root, origin, None, 37, 4000)
            assert page[0] == "page"
            got += list(zip(page[1], page[2]))
            if not page[3]:
                break
            origin = page[4]
        assert got == want, (SCEN[i][0], b)
        # a range is the slice of the content between its ends; the kept walk answers the same
        snap = RR.Snapshot(nodes, root)
        for o_, l_, mx in RC.random_ranges(r, [k for k, _ in want], 40):
            lo, hi = o_ or RC.ZERO, l_ or RC.FF
            inr = [(k, v) for k, v in want if lo <= k <= hi]
            page = RR.expected_range(nodes, root, o_, l_, mx)
            cap = r.choice([0, 1, 50, 200, 1 << 20])
            assert snap.expected_range(o_, l_, mx) == page
            assert snap.expected_range(o_, l_, mx, cap) == RR.expected_range(nodes, root, o_, l_, mx, cap)
            assert page[:3] == ("page", [k for k, _ in inr[:mx]], [v for _, v in inr[:mx]])
            assert page[3] == (len(inr) > mx) and page[4] == (inr[mx][0] if len(inr) > mx else None)


@pytest.mark.parametrize("i", range(len(SCEN)), ids=[s[0] for s in SCEN])
def test_random_ranges_hit_and_page(oracle, i):
    """The 200 ranges a state gets in tests/test_gpu_range.py: on a state of at least 8 entries at
    least a third return an entry and at least a tenth return `more` (a state of fewer entries
    cannot page a max_entries of 7 or more, and an empty one returns nothing)."""
    checked = 0
    for b, o, _ in _states(oracle, i):
        nodes, root = _nodes(o), o.root_hash()
        live = [k for k, _ in RR.content(nodes, root)]
        if len(live) < 8:
            continue
        pages = [RR.expected_range(nodes, root, o_, l_, mx)
                 for o_, l_, mx in RC.random_ranges(random.Random(1000 * i + b), live)]
        assert sum(1 for p in pages if p[1]) * 3 >= len(pages), (SCEN[i][0], b)
        assert sum(1 for p in pages if p[3]) * 10 >= len(pages), (SCEN[i][0], b)
        checked += 1
    assert checked or SCEN[i][0] in ("single", "recut_opened_branch")


def test_dense_ranges_cover_every_split_depth(oracle):
    keys, vals, K, ranges = RC.dense_case()
    o = oracle.Trie()
    for k, v in zip(keys, vals):
        o.put(k, v)
    assert len(K.P) == 17 and {p for _, _, p in ranges} == set(K.P)
    nodes, root = o.reachable(), o.root_hash()
    assert RR.content(nodes, root) == sorted(zip(keys, vals))
    pages = [RR.expected_range(nodes, root, o_, l_, 3) for o_, l_, _ in ranges]
    assert sum(1 for p in pages if p[1]) * 3 >= len(pages)
    assert sum(1 for p in pages if p[3]) * 10 >= len(pages)
    # the shapes of the other host cases are what their names say
    ek, ev = export_cases.embedded_case()
    e = oracle.Trie()
    for k, v in zip(ek, ev):
        e.put(k, v)
    assert export_cases.holds_embedded_child(e.reachable())
    assert RR.content(e.reachable(), e.root_hash()) == sorted(zip(ek, ev))


def test_value_only_branch_is_read_like_any_node(oracle):
    ks, vs, blocks, (k1, k2, k3) = proof_cases.vb_case(False)
    o = oracle.Trie()
    for k, v in zip(ks, vs):
        o.put(k, v)
    for k, v in blocks[0][0]:
        o.put(k, v)
    want = dict(zip(ks, vs))
    want.update(blocks[0][0])
    assert RR.content(o.reachable(), o.root_hash()) == sorted(want.items())
    assert RR.expected_range(o.reachable(), o.root_hash(), k1, k1, 1)[:4] == ("page", [k1], [want[k1]], False)


def test_missing_subtrees_are_one_thing_at_their_lowest_key(oracle):
    r = random.Random(9)
    ks = sorted(C._rk(r) for _ in range(300))
    vs = [C.account_value(r) for _ in ks]
    o = oracle.Trie()
    for k, v in zip(ks, vs):
        o.put(k, v)
    nodes, root = o.reachable(), o.root_hash()
    path, _ = P.expected_proof(nodes, root, ks[150])
    gone = P.kec(path[1])  # the depth-1 subtree holding ks[150]
    part = {h: e for h, e in nodes.items() if h != gone}
    things = list(RR.walk(part, root))
    miss = [t for t in things if t[0] == "missing"]
    assert len(miss) == 1 and miss[0][1] == gone and miss[0][2] == P.nibbles(ks[150])[:1]
    at = things.index(miss[0])
    assert [t[1] for t in things[:at]] == ks[:at] and at > 3
    # refused when the stub is among the first max_entries + 1 things, served when it is past them
    assert RR.expected_range(part, root, None, None, at) == ("missing", gone)
    assert RR.expected_range(part, root, None, None, at - 1) == ("page", ks[:at - 1], vs[:at - 1], True, ks[at - 1])
    assert RR.expected_range(part, root, ks[150], None, 1) == ("missing", gone)
    # a range that ends below the missing subtree's prefix does not meet it
    assert RR.expected_range(part, root, None, ks[at - 1], 1000) == ("page", ks[:at], vs[:at], False, None)
