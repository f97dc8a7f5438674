"""CPU: the conditions of the batched range-scan cases (tests/ranges_cases.py), held with the
reference alone (tests/ranges_ref.py over the oracle's nodes), for the very batches
tests/test_gpu_ranges.py runs; and expected_ranges with one request equal to
range_ref.expected_range."""
import random

import pytest

from tests import range_cases as RC
from tests import range_ref as RR
from tests import ranges_cases as BC
from tests import ranges_ref as BR


def _content(tries):
    return {t: RR.content(nodes, root) for t, (nodes, root) in tries.items()}


@pytest.mark.parametrize("name", sorted(BC.RUNS))
def test_batches_cut_in_every_way(oracle, name):
    tries = BC.state(oracle, name)
    content = _content(tries)
    batches = BC.batches_for(name, content)
    complete = inside = at_first = by_cap = after_empty = 0
    nqs, shapes = set(), set()
    for reqs, mx, cap in batches:
        nq = len(reqs)
        nqs.add(nq)
        for q, (t, o, l) in enumerate(reqs):
            if t == BC.UNHELD:
                shapes.add("unheld")
            if o is not None and l is not None and o > l:
                shapes.add("reversed")
            if t in BC.EMPTY_IDS:
                shapes.add(("empty", "front" if q == 0 else "end" if q == nq - 1 else "middle"))
            if q and reqs[q - 1][0] == t and t in content and content[t]:
                shapes.add("repeated")
        if any(o is None and l is None for _, o, l in reqs) and any(o is not None or l is not None for _, o, l in reqs):
            shapes.add("mixed")
        want = BR.expected_ranges(tries, reqs, mx, cap)
        assert want[0] == "pages", want[0]  # (full stores, and a cap no smaller than the first value)
        _, pages, n_done, nxt = want
        returned = sum(len(ks) for ks, _ in pages)
        assert returned <= mx and sum(len(v) for _, vs in pages for v in vs) <= cap
        assert all(not pages[q][0] for q in range(n_done + 1, nq))
        if n_done == nq:
            complete += 1
            assert nxt is None
            continue
        assert nxt is not None and (not pages[n_done][0] or pages[n_done][0][-1] < nxt)
        if pages[n_done][0]:
            inside += 1
        else:
            at_first += 1
        if returned < mx:
            by_cap += 1
        if n_done and not pages[n_done - 1][0]:
            after_empty += 1
    n = len(batches)
    assert nqs == set(BC.NQS)
    assert shapes >= {"unheld", "reversed", "repeated", "mixed", ("empty", "front"), ("empty", "middle"),
                      ("empty", "end")}, shapes
    assert 5 * complete >= n and 5 * inside >= n, (complete, inside, n)
    assert at_first >= 1 and by_cap >= 1 and after_empty >= 1, (at_first, by_cap, after_empty)


def test_one_request_is_the_single_reference(oracle):
    tries = BC.state(oracle, "big")
    nodes, root = tries[5]
    keys = [k for k, _ in RR.content(nodes, root)]
    r = random.Random(9)
    first = len(RR.content(nodes, root)[0][1])
    for a, b, mx in RC.random_ranges(r, keys, 60):
        for cap in (1 << 20, 300, first - 1):
            one = RR.expected_range(nodes, root, a, b, mx, cap)
            got = BR.expected_ranges(tries, [(5, a, b)], mx, cap)
            if one[0] == "nospc":
                assert got == one
                continue
            _, ks, vs, more, nxt = one
            assert got == ("pages", [(ks, vs)], 0 if more else 1, nxt), (a, b, mx, cap)
    # a store that lacks a node: the refusal names the hash and the request
    k = keys[len(keys) // 2]
    from tests import proof_ref as P
    wit = {root: nodes[root]}
    wit.update({P.kec(e): e for e in P.expected_proof(nodes, root, k)[0]})
    part = {5: (wit, root), 6: tries[6]}
    one = RR.expected_range(wit, root, None, None, 50)
    assert one[0] == "missing"
    assert BR.expected_ranges(part, [(6, None, None), (5, None, None)], 50) == ("missing", one[1], 1)
    assert BR.expected_ranges(part, [(6, None, None), (5, None, None)], 5)[0] == "pages"
