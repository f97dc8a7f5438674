"""CPU: the reference of the batched trie diff (tests/diffs_ref.py) held to the single-pair reference,
and the conditions of the batches of tests/diffs_cases.py held with the reference alone, for the very
batches tests/test_gpu_diffs.py runs.  The state pairs are the commit scenarios' state pairs that
tests/test_diff_ref.py uses, grouped into forests, and the 60-trie forest against itself after a
block."""
import pytest

from tests import diff_ref as DR
from tests import diffs_cases as BC
from tests import diffs_ref as BR


@pytest.fixture(scope="module")
def states(oracle):
    return BC.scenario_states(oracle)


def _stitched(a, b, same, reqs, mx, cap):
    """expected_diffs from single-pair expected_diff answers alone: each request asked with what is
    left of the two budgets, in order, until one is cut."""
    nq = len(reqs)
    pages = [[] for _ in range(nq)]
    left, room = mx, cap
    for q, (ta, tb, o, l) in enumerate(reqs):
        tb = ta if tb is None else tb
        if same and ta == tb:
            continue
        na, ra = a.get(ta, BR.EMPTY)
        nb, rb = b.get(tb, BR.EMPTY)
        if left == 0:  # the budget ended exactly at the end of a request: the next difference cuts
            one = DR.expected_diff(na, ra, nb, rb, o, l, 1, 1 << 40)
            if one[1]:
                return ("pages", pages, q, one[1][0][0])
            continue
        one = DR.expected_diff(na, ra, nb, rb, o, l, left, room)
        if one[0] == "nospc":
            if left == mx and room == cap and not any(pages):
                return one
            first = DR.expected_diff(na, ra, nb, rb, o, l, 1, 1 << 40)
            return ("pages", pages, q, first[1][0][0])
        assert one[0] == "page"
        _, ents, more, nxt = one
        pages[q] = ents
        left -= len(ents)
        room -= sum(len(v) for _, _, v in ents)
        if more:
            return ("pages", pages, q, nxt)
    return ("pages", pages, nq, None)


@pytest.mark.parametrize("name", sorted(BC.RUNS))
def test_batches_cut_in_every_way(oracle, states, name):
    a, b, same, pairs = BC.state_pair(oracle, name, states)
    diffs = BC.full_diffs(a, b, same, pairs)
    batches = BC.batches_for(name, diffs, same)
    complete = inside = at_first = by_cap = after_empty = 0
    nqs, shapes = set(), set()
    for reqs, mx, cap in batches:
        nq = len(reqs)
        nqs.add(nq)
        seen = set()
        for q, (ta, tb, o, l) in enumerate(reqs):
            tb_ = ta if tb is None else tb
            if ta not in a and tb_ not in b:
                shapes.add("neither")
            elif not (same and ta == tb_) and ((ta in a) != (tb_ in b)):
                shapes.add("one_sided")
            if o is not None and l is not None and o > l:
                shapes.add("reversed")
            if (same and ta == tb_) or (ta in a and tb_ in b and a[ta][1] == b[tb_][1]):
                shapes.add(("identical", "front" if q == 0 else "end" if q == nq - 1 else "middle"))
            if (ta, tb_) in seen and diffs.get((ta, tb_)):
                shapes.add("repeated")
            seen.add((ta, tb_))
        if any(o is None and l is None for _, _, o, l in reqs) and any(o is not None or l is not None
                                                                       for _, _, o, l in reqs):
            shapes.add("mixed")
        want = BR.expected_diffs(a, b, reqs, mx, cap, same)
        assert want == _stitched(a, b, same, reqs, mx, cap), (name, nq, mx, cap)
        assert want[0] == "pages", want[0]  # (full stores, and a cap no smaller than the first value)
        _, pages, n_done, nxt = want
        returned = sum(len(p) for p in pages)
        assert returned <= mx and sum(len(v) for p in pages for _, _, v in p) <= cap
        assert all(not pages[q] for q in range(n_done + 1, nq))
        if n_done == nq:
            complete += 1
            assert nxt is None
            continue
        assert nxt is not None and (not pages[n_done] or pages[n_done][-1][0] < nxt)
        if pages[n_done]:
            inside += 1
        else:
            at_first += 1
        if returned < mx:
            by_cap += 1
        if n_done and not pages[n_done - 1]:
            after_empty += 1
    n = len(batches)
    assert nqs == set(BC.NQS)
    assert shapes >= {"neither", "one_sided", "reversed", "repeated", "mixed", ("identical", "front"),
                      ("identical", "middle"), ("identical", "end")}, shapes
    assert 5 * complete >= n and 5 * inside >= n, (complete, inside, n)
    assert at_first >= 1 and by_cap >= 1 and after_empty >= 1, (at_first, by_cap, after_empty)


def test_one_request_is_the_single_reference(oracle, states):
    """nq = 1 equals diff_ref.expected_diff, the refusals included; a store that lacks a node names
    the hash and the request, and only when it is among the first max_entries + 1 things."""
    sts = states[0]
    (na, ra), (nb, rb) = sts[0], sts[1]
    full = [(t[1], t[2], t[3]) for t in DR.walk_diff(na, ra, nb, rb)]
    assert len(full) >= 3
    first = next(len(v) for _, _, v in full if v)
    for mx in (1, 2, len(full), len(full) + 1):
        for cap in (1 << 20, first, first - 1, 0):
            for o in (None, full[1][0]):
                one = DR.expected_diff(na, ra, nb, rb, o, None, mx, cap)
                got = BR.expected_diffs({1: sts[0]}, {1: sts[1]}, [(1, None, o, None)], mx, cap)
                if one[0] == "nospc":
                    assert got == one
                    continue
                _, ents, more, nxt = one
                assert got == ("pages", [ents], 0 if more else 1, nxt), (mx, cap)
    only_a = next(h for h in na if h not in nb and h != ra)
    part = {h: e for h, e in na.items() if h != only_a}
    one = DR.expected_diff(part, ra, nb, rb)
    assert one == ("missing", only_a)
    sa, sb = {1: (part, ra), 2: sts[0]}, {1: sts[1], 2: sts[2 % len(sts)]}
    two = [(t[1], t[2], t[3]) for t in DR.walk_diff(*sa[2], *sb[2])]
    assert two
    assert BR.expected_diffs(sa, sb, [(2, None, None, None), (1, None, None, None)], 1000) == ("missing", only_a, 1)
    got = BR.expected_diffs(sa, sb, [(2, None, None, None), (1, None, None, None)], max(len(two) - 1, 1))
    assert got[0] == "pages" or len(two) == 1
