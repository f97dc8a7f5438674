"""CPU: the reference of the trie-diff tests (tests/diff_ref.py) held to itself and to the oracle.
Over every ordered pair of states (i, j), |i - j| <= 3, of every scenario: the lockstep walk with the
skip rule equals the merge of the two full contents; the result applied to the oracle's trie i gives
root j (the pairs where khipu's value-only branch prevents that are named and counted, not skipped);
the pages, cuts and val_cap rules of expected_diff equal the same rules over the merged list; and the
inputs show every kind, a skipped subtree, a split and the value-only-branch kind."""
import random

import pytest

from tests import diff_cases as DC
from tests import diff_ref as DR

SCEN = DC.scenarios()


@pytest.fixture(scope="module")
def world(oracle):
    """Per scenario: its states [(nodes, root)] and their full contents."""
    out = {}
    for s in SCEN:
        st = DC.states(oracle, s)
        out[s[0]] = (st, [DR.content(n, r) for n, r in st])
    return out


def _merge(ca, cb):
    a = {k: (v, vb) for k, v, vb in ca}
    b = {k: (v, vb) for k, v, vb in cb}
    out = []
    for k in sorted(set(a) | set(b)):
        if k not in b:
            out.append((k, DR.ONLY_A, b""))
        elif k not in a:
            out.append((k, DR.ONLY_B, b[k][0]))
        elif a[k] != b[k]:
            out.append((k, DR.CHANGED, b[k][0]))
    return out


@pytest.mark.parametrize("s", range(len(SCEN)), ids=[s[0] for s in SCEN])
def test_walk_equals_content(world, s):
    st, cont = world[SCEN[s][0]]
    for i, j in DC.pairs(len(st)):
        things = list(DR.walk_diff(*st[i], *st[j]))
        assert all(t[0] == "diff" for t in things)
        got = [(t[1], t[2], t[3]) for t in things]
        assert got == _merge(cont[i], cont[j]), (SCEN[s][0], i, j)
        assert (got == []) == (st[i][1] == st[j][1])


def test_content_diff_is_the_merge(world):
    st, cont = world["storage"]
    assert DR.content_diff(*st[0], *st[2]) == _merge(cont[0], cont[2]) != []


def test_the_inputs_show_every_case(world):
    """Each kind, a skipped subtree (the walk decodes fewer nodes than the two stores hold), a split
    and the value-only-branch kind occur."""
    kinds, skipped, splits, vb, fewer = set(), 0, 0, 0, 0
    for s in SCEN:
        st, _ = world[s[0]]
        for i, j in DC.pairs(len(st)):
            stats = {}
            kinds |= {t[2] for t in DR.walk_diff(*st[i], *st[j], stats=stats)}
            skipped += stats.get("skipped", 0)
            splits += stats.get("splits", 0)
            vb += stats.get("vb", 0)
            fewer += i != j and stats.get("decoded", 0) < len(st[i][0]) + len(st[j][0])
    assert kinds == {1, 2, 3} and skipped and splits and vb and fewer


def test_applying_the_diff_gives_the_other_root(oracle, world):
    """put(upserts) then remove(deletes) on the oracle's trie i gives root j.  khipu's value-only
    branch depends on history (a re-put while a 63-nibble sibling is still there makes one, a put on
    one never makes the leaf again), so a pair may miss the root only by WHICH keys sit in value-only
    branches, every key and value being right; those pairs are named and counted, and the leaf ->
    value-only branch direction must still come out right."""
    missed, vb_made = [], 0
    for s in SCEN:
        st, cont = world[s[0]]
        for i, j in DC.pairs(len(st)):
            d = _merge(cont[i], cont[j])
            if not d:
                continue
            o = DC.oracle_at(oracle, s, i)
            want_vb = {k for k, _, vb in cont[j] if vb}
            try:
                DC.fold(o, [(k, v) for k, kind, v in d if kind != DR.ONLY_A], [k for k, kind, _ in d if kind == DR.ONLY_A])
                ok = o.root_hash() == st[j][1]
                got = DR.content(*DC.snap(o))
            except oracle.OracleError:  # (removing a value-only branch's key throws in khipu)
                ok, got = False, None
            if not ok:
                # the keys and values came out right; only which keys sit in value-only branches differs
                assert got is None or ([(k, v) for k, v, _ in got] == [(k, v) for k, v, _ in cont[j]] and
                                       {k for k, _, vb in got if vb} != want_vb), (s[0], i, j)
                missed.append((s[0], i, j))
            elif want_vb and not any(vb for _, _, vb in cont[i]):
                vb_made += 1
    print("pairs whose value-only branches the apply cannot reproduce:", len(missed), missed)
    assert vb_made >= 1
    assert ("vb_equal_value", 1, 0) in missed  # (a put on a value-only branch never makes the leaf again)
    assert len(missed) < len([1 for s in SCEN for _ in DC.pairs(len(world[s[0]][0]))]) // 4


def test_expected_diff_pages_and_cuts(world):
    """expected_diff (walk, max_entries + 1 things, fit) equals the same rules over the merged list,
    on the constructed origins, limits, budgets and val_cap edges; paging by next reaches the end."""
    r = random.Random(9)
    shapes = set()
    for name in ("storage", "deep", "value_only_branch", "to_empty"):
        st, cont = world[name]
        for i, j in [(0, 1), (2, 0), (1, len(st) - 1)]:
            d = _merge(cont[i], cont[j])
            for o, l, mx, cap in DC.queries(r, d):
                got = DR.expected_diff(*st[i], *st[j], o, l, mx, cap)
                assert got == DC.expected_from_content(d, o, l, mx, cap), (name, i, j, o, l, mx, cap)
                shapes.add((got[0], got[0] == "page" and got[2]))
            for chunk in (1, 7):
                out, origin = [], None
                while True:
                    g = DR.expected_diff(*st[i], *st[j], origin, None, chunk)
                    out += g[1]
                    if not g[2]:
                        break
                    origin = g[3]
                assert out == d
    assert shapes == {("page", True), ("page", False), ("nospc", False)}


def test_missing_nodes_are_named_only_when_not_skipped():
    """Two partial stores that lack the same subtree diff completely; one that lacks a changed
    subtree names its hash."""
    # (built from full stores of a small pair by dropping nodes: see tests/test_gpu_diff.py for the device)
    from oracle import oracle as O
    r = random.Random(4)
    ks = sorted(DC.C._rk(r) for _ in range(120))
    vs = [DC.C.account_value(r) for _ in ks]
    a, b = O.Trie(), O.Trie()
    for k, v in zip(ks, vs):
        a.put(k, v)
        b.put(k, v)
    b.put(ks[3], b"\x05" * 9)
    na, ra = DC.snap(a)
    nb, rb = DC.snap(b)
    full = [t for t in DR.walk_diff(na, ra, nb, rb)]
    assert [t[1:] for t in full] == [(ks[3], 3, b"\x05" * 9)]
    shared = set(na) & set(nb)
    drop = next(h for h in shared if h != ra)
    pa = {h: e for h, e in na.items() if h != drop}
    pb = {h: e for h, e in nb.items() if h != drop}
    assert list(DR.walk_diff(pa, ra, pb, rb)) == full
    assert list(DR.walk_diff(pa, ra, nb, rb)) == full  # (skipped by its reference: never resolved)
    only_a = next(h for h in na if h not in nb and h != ra)
    pa = {h: e for h, e in na.items() if h != only_a}
    assert ("missing", only_a) in list(DR.walk_diff(pa, ra, nb, rb))
    assert DR.expected_diff(pa, ra, nb, rb) == ("missing", only_a)
