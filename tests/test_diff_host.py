"""CPU: the trie diff of khipu_amd/csrc/diff.h replayed on the host under AddressSanitizer and UBSan.
tests/diff_host/diff_check.cc (a stand-alone program) builds the records of two tries bottom-up and
runs the rounds as range_kernels.hip does -- the root pair, select with the skip test in 16 lanes an
item, scan, a 16-lane fill into a frontier cut at max_entries + 2 items, lengths, fit, write into
outputs of exactly the scanned sizes.  Every answer must equal tests/diff_ref.expected_diff over the
oracle's nodes; the same inputs with the cut at max_entries + 1, and with the skip test made after
the cut, must disagree somewhere, so the inputs can see both."""
import random
import subprocess

import pytest

from tests import cases as C
from tests import diff_cases as DC
from tests import diff_ref as DR
from tests import hostprog
from tests.hostprog import hexs as _hex
from tests.hostprog import unhexs as _unhex

SHAPES = DC.shapes()
BIG = 1 << 30

prog = hostprog.prog_fixture("diff")


def _run(prog, tmp_path, puts_a, puts_b, queries, slack=2, late=0, tag=""):
    """puts: [(key, value, makes a value-only branch)]; queries: [(origin, limit, max_entries, val_cap)]
    -> (root a, root b, [answer in the form of diff_ref.expected_diff], [(rounds, visited)])"""
    lines = [f"{'B' if vb else 'P'}A {k.hex()} {_hex(v)}" for k, v, vb in puts_a]
    lines += [f"{'B' if vb else 'P'}B {k.hex()} {_hex(v)}" for k, v, vb in puts_b]
    lines += [f"D {(o or DC.ZERO).hex()} {(l or DC.FF).hex()} {mx} {cap} {slack} {late}" for o, l, mx, cap in queries]
    p = tmp_path / f"in{tag}_{slack}_{late}.txt"
    p.write_text("\n".join(lines) + "\n")
    r = subprocess.run([prog, str(p)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]  # (a sanitizer report ends the program with a non-zero status)
    out = [ln.split() for ln in r.stdout.split("\n")[:-1]]
    assert out[0][0] == "T"
    ans, cost = [], []
    for x in out[1:]:
        assert x[0] == "A"
        if x[1] == "page":
            k = int(x[2])
            ents = [(bytes.fromhex(x[7 + 3 * i]), int(x[8 + 3 * i]), _unhex(x[9 + 3 * i])) for i in range(k)]
            ans.append(("page", ents, x[3] == "1", _unhex(x[4]) if x[3] == "1" else None))
            cost.append((int(x[5]), int(x[6])))
        elif x[1] == "nospc":
            ans.append(("nospc", int(x[2])))
        else:
            ans.append(("missing", bytes.fromhex(x[2])))
    assert len(ans) == len(queries)
    return bytes.fromhex(out[0][1]), bytes.fromhex(out[0][2]), ans, cost


def _oracle(oracle, puts):
    """The oracle's trie of the puts; a put marked as leaving a value-only branch is made again once
    every key is in (its 63-nibble sibling with it)."""
    o = oracle.Trie()
    for k, v, _ in puts:
        o.put(k, v)
    for k, v, vb in puts:
        if vb:
            o.put(k, v)
    return DC.snap(o)


def _queries(r, diffs):
    return [(None, None, mx, BIG) for mx in DC.HOST_MAXES] + DC.queries(r, diffs)


@pytest.mark.parametrize("s", range(len(SHAPES)), ids=[s[0] for s in SHAPES])
def test_host_diffs_match_the_reference(prog, tmp_path, oracle, s):
    name, pa, pb = SHAPES[s]
    r = random.Random(s)
    for swap, (xa, xb) in enumerate(((pa, pb), (pb, pa))):
        (na, ra), (nb, rb) = _oracle(oracle, xa), _oracle(oracle, xb)
        diffs = DR.content_diff(na, ra, nb, rb)
        assert diffs, name
        q = _queries(r, diffs)
        got_a, got_b, got, cost = _run(prog, tmp_path, xa, xb, q, tag=swap)
        assert (got_a, got_b) == (ra, rb)
        for x, g in zip(q, got):
            assert g == DR.expected_diff(na, ra, nb, rb, *x), (name, swap, x[0] and x[0].hex(), x[1] and x[1].hex(), x[2:])
        assert max(c[0] for c in cost) <= 67
    if name == "vb_against_leaf":
        assert [(d[1], d[2]) for d in diffs] == [(3, pa[0][1])]  # equal values, and still a difference


def test_host_identical_tries_take_no_round(prog, tmp_path, oracle):
    _, pa, _ = next(s for s in SHAPES if s[0] == "random300_changed_7")
    _, _, got, cost = _run(prog, tmp_path, pa, pa, [(None, None, 5, 100)])
    assert got == [("page", [], False, None)] and cost == [(0, 0)]
    _, _, got, cost = _run(prog, tmp_path, [], [], [(None, None, 5, 100)])
    assert got == [("page", [], False, None)] and cost == [(0, 0)]
    _, _, got, _ = _run(prog, tmp_path, pa, [], [(DC.FF, DC.ZERO, 5, 100)])  # origin > limit
    assert got == [("page", [], False, None)]


def test_host_skipping_follows_the_changed_paths(prog, tmp_path, oracle):
    """300 keys, 1 changed: the items the walk selects are far fewer than those of the two full
    scans (each side against the empty trie)."""
    _, pa, pb = next(s for s in SHAPES if s[0] == "random300_changed_1")
    q = [(None, None, 1000, BIG)]
    visited = [_run(prog, tmp_path, x, y, q, tag=i)[3][0][1] for i, (x, y) in enumerate(((pa, pb), (pa, []), ([], pb)))]
    assert 0 < visited[0] < 40 and visited[1] > 300 and visited[2] > 300


def test_host_val_cap(prog, tmp_path, oracle):
    """val_cap at exactly a page's bytes, one less, the first non-empty value, one less than it, and 0."""
    _, pa, pb = next(s for s in SHAPES if s[0] == "random300_changed_150")
    (na, ra), (nb, rb) = _oracle(oracle, pa), _oracle(oracle, pb)
    full = DR.expected_diff(na, ra, nb, rb, None, None, 64)
    origin = next(k for k, kind, v in full[1] if kind != 1)  # (the first difference that carries a value)
    full = DR.expected_diff(na, ra, nb, rb, origin, None, 64)
    total, first = sum(len(v) for _, _, v in full[1]), len(full[1][0][2])
    assert first > 0
    q = [(origin, None, 64, cap) for cap in (total, total - 1, first, first - 1, 0)]
    _, _, got, _ = _run(prog, tmp_path, pa, pb, q)
    assert got == [DR.expected_diff(na, ra, nb, rb, *x) for x in q]
    assert len(got[0][1]) == 64 and len(got[1][1]) < 64 and got[1][2]
    assert got[3] == got[4] == ("nospc", first)
    # a first difference of kind 1 carries no value: it fits a val_cap of 0
    _, _, got, _ = _run(prog, tmp_path, pa, [], [(None, None, 3, 0)], tag="k1")
    assert got[0][0] == "page" and [e[1:] for e in got[0][1]] == [(1, b"")] * 3


def test_a_cut_at_max_entries_plus_one_is_seen(prog, tmp_path, oracle):
    """The same inputs through a frontier cut at max_entries + 1 items: an origin just past a key
    leaves that key's item on origin's path, empty, in the place of the item `more` and `next` come
    from -- at least one answer is wrong."""
    _, pa, pb = next(s for s in SHAPES if s[0] == "random300_changed_150")
    (na, ra), (nb, rb) = _oracle(oracle, pa), _oracle(oracle, pb)
    diffs = DR.content_diff(na, ra, nb, rb)
    q = [(DC.RC._step(k, 1), None, mx, BIG) for k, _, _ in diffs[:40] for mx in (1, 2, 3)]
    want = [DR.expected_diff(na, ra, nb, rb, *x) for x in q]
    assert _run(prog, tmp_path, pa, pb, q)[2] == want
    _, _, got, _ = _run(prog, tmp_path, pa, pb, q, slack=1)
    assert sum(1 for w, g in zip(want, got) if w != g) >= 1


def test_the_skip_test_after_the_cut_is_seen(prog, tmp_path, oracle):
    """A branch pair of 16 children of which only the last differs, asked at small budgets over
    several such pairs: with the skip test made after the cut the 15 equal children fill the frontier
    and the difference is lost; made before it, every answer is right."""
    wrong = 0
    for seed in range(4):
        pa, pb = DC.sixteen_children_one_differs(seed)
        (na, ra), (nb, rb) = _oracle(oracle, pa), _oracle(oracle, pb)
        q = [(None, None, mx, BIG) for mx in (1, 2, 3, 7, 13, 14, 15)]
        want = [DR.expected_diff(na, ra, nb, rb, *x) for x in q]
        assert all(w[0] == "page" and len(w[1]) == 1 for w in want)
        assert _run(prog, tmp_path, pa, pb, q, tag=seed)[2] == want
        got = _run(prog, tmp_path, pa, pb, q, late=1, tag=seed)[2]
        wrong += sum(1 for w, g in zip(want, got) if w != g)
    assert wrong >= 4
