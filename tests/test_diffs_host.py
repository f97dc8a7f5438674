"""CPU: the batched trie diff of khipu_amd/csrc/diff.h replayed on the host under AddressSanitizer
and UBSan.  tests/diffs_host/diffs_check.cc (a stand-alone program) builds the records of several
tries a side bottom-up into one store a side and runs the rounds as range_kernels.hip's k_diffs_* do
-- one df_request a request, then select with the skip test in 16 lanes an item, each item against
its own request's range, scan, a 16-lane fill into a segmented frontier cut at exactly
max_entries + 2 * nq items, lengths, fit, write into outputs of exactly the scanned sizes; every
planned place is filled exactly once.  Every answer must equal tests/diffs_ref.expected_diffs over
the oracle's nodes; with the cut one item smaller an input built to need the full cut must come out
wrong, and so must inputs through a skip test made after the cut.

Tries: every shape of tests/diff_cases.shapes() under an id of its own (side a of the shape on side
a, side b on side b), a twin (the same 300 keys on both sides), an id only side a holds and one only
side b holds."""
import random
import subprocess

import pytest

from tests import diff_cases as DC
from tests import diffs_ref as BR
from tests import hostprog
from tests.hostprog import hexs as _hex
from tests.hostprog import unhexs as _unhex
from tests.test_diff_host import _oracle

NQS = [1, 2, 3, 16, 17]
MAXES = [1, 2, 15, 16, 17, 255, 256, 257]  # either side of the fill's 16 items a block and the count's 256
BIG = 1 << 30
UNHELD = 999
SHAPES = DC.shapes()
TWIN, ONLY_A, ONLY_B = 5000, 70000, 1 << 31

prog = hostprog.prog_fixture("diffs")


def _run(prog, tmp_path, side_a, side_b, batches, less=0, late=0, same=0, tag=""):
    """side_a, side_b: {id: puts [(key, value, makes a value-only branch)]}; batches: [(requests [(id of
    a, id of b, origin, limit)], max_entries, val_cap)]
    -> ({("a" | "b", id): root}, [answer in the form of expected_diffs], [(rounds, visited)])"""
    lines = []
    for side, tries in (("A", side_a), ("B", side_b)):
        for t, puts in tries.items():
            lines.append(f"T{side} {t}")
            lines += [f"{'B' if vb else 'P'} {k.hex()} {_hex(v)}" for k, v, vb in puts]
    for reqs, mx, cap in batches:
        lines.append(f"Q {mx} {cap} {less} {late} {same}")
        lines += [f"R {ta} {ta if tb is None else tb} {(o or DC.ZERO).hex()} {(l or DC.FF).hex()}" for ta, tb, o, l in reqs]
    p = tmp_path / f"in{tag}_{less}_{late}_{same}.txt"
    p.write_text("\n".join(lines) + "\n")
    r = subprocess.run([prog, str(p)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])  # (a sanitizer report ends the program non-zero)
    out = [ln.split() for ln in r.stdout.split("\n")[:-1]]
    roots = {(x[1], int(x[2])): bytes.fromhex(x[3]) for x in out if x[0] == "T"}
    ans, cost = [], []
    for (reqs, _, _), x in zip(batches, [x for x in out if x[0] == "A"]):
        nq = len(reqs)
        if x[1] == "pages":
            k, n_done = int(x[2]), int(x[3])
            eo = [int(e) for e in x[7:8 + nq]]
            ents = x[8 + nq:]
            assert len(ents) == 3 * k and eo[0] == 0 and eo[nq] == k and eo == sorted(eo)
            d = [(bytes.fromhex(ents[3 * i]), int(ents[3 * i + 1]), _unhex(ents[3 * i + 2])) for i in range(k)]
            ans.append(("pages", [d[eo[q]:eo[q + 1]] for q in range(nq)], n_done, _unhex(x[4]) if n_done < nq else None))
            cost.append((int(x[5]), int(x[6])))
        elif x[1] == "nospc":
            ans.append(("nospc", int(x[2])))
            cost.append(None)
        else:
            ans.append(("missing", bytes.fromhex(x[2]), int(x[3])))
            cost.append(None)
    assert len(ans) == len(batches)
    return roots, ans, cost


@pytest.fixture(scope="module")
def world(oracle):
    """(puts of side a {id: puts}, of side b, the oracle's stores of side a {id: (nodes, root)}, of side
    b, {id: the keys that differ})"""
    pa, pb = {}, {}
    for s, (name, xa, xb) in enumerate(SHAPES):
        pa[s + 1], pb[s + 1] = xa, xb
    three = next(s for s in SHAPES if s[0] == "random300_changed_7")
    pa[TWIN] = pb[TWIN] = three[1]
    pa[ONLY_A] = three[2][:40]
    pb[ONLY_B] = three[1][:25]
    sa = {t: _oracle(oracle, p) for t, p in pa.items() if p}
    sb = {t: _oracle(oracle, p) for t, p in pb.items() if p}
    keys = {}
    for t in set(pa) | set(pb):
        na, ra = sa.get(t, BR.EMPTY)
        nb, rb = sb.get(t, BR.EMPTY)
        keys[t] = [x[1] for x in BR.DR.walk_diff(na, ra, nb, rb)]
    return pa, pb, sa, sb, keys


def _batches(world, seed):
    _, _, _, _, keys = world
    r = random.Random(seed)
    ids = sorted(keys)
    big = [t for t in ids if len(keys[t]) >= 100]
    out = []
    for nq in NQS:
        for mx in MAXES:
            for rep in range(3):
                reqs = []
                for _ in range(nq):
                    x = r.random()
                    t = UNHELD if x < 0.06 else reqs[-1][0] if (reqs and x < 0.2) else r.choice(big) if x < 0.4 else r.choice(ids)
                    u = None if r.random() < 0.7 else r.choice(ids)  # (a crossed pair now and then)
                    ks = keys.get(t, []) if u is None else []
                    o, l, _ = DC.RC.random_ranges(r, ks, 1)[0]
                    if r.random() < 0.35:
                        o = l = None
                    reqs.append((t, u, o, l))
                out.append((reqs, mx, BIG))
    return out


def test_host_batches_match_the_reference(prog, tmp_path, world):
    pa, pb, sa, sb, _ = world
    batches = _batches(world, 1)
    roots, got, cost = _run(prog, tmp_path, pa, pb, batches)
    assert roots == {**{("a", t): sa.get(t, BR.EMPTY)[1] for t in pa}, **{("b", t): sb.get(t, BR.EMPTY)[1] for t in pb}}
    for (reqs, mx, cap), g in zip(batches, got):
        assert g == BR.expected_diffs(sa, sb, reqs, mx, cap), (len(reqs), mx)
    assert max(c[0] for c in cost) <= 68
    cut = [g for g in got if g[2] < len(g[1])]
    assert len(cut) >= 20 and len(got) - len(cut) >= 20
    assert any(not g[1][g[2]] for g in cut) and any(g[1][g[2]] for g in cut)
    assert {k for g in got for p in g[1] for _, k, _ in p} == {1, 2, 3}


def test_host_one_handle_on_both_sides(prog, tmp_path, world):
    """Side b is side a's store: a request naming one id twice is empty, two ids of the store differ."""
    pa, _, sa, _, _ = world
    ids = sorted(sa)
    r = random.Random(3)
    batches = [([(r.choice(ids), r.choice(ids + [None]), None, None) for _ in range(nq)], mx, BIG)
               for nq in (1, 3, 17) for mx in (2, 16, 257)]
    _, got, _ = _run(prog, tmp_path, pa, {}, batches, same=1)
    for (reqs, mx, cap), g in zip(batches, got):
        assert g == BR.expected_diffs(sa, sa, reqs, mx, cap, same=True), (len(reqs), mx)
    assert any(any(g[1]) for g in got)


def test_host_val_cap(prog, tmp_path, world):
    """val_cap at exactly the bytes of the whole answer, one less, the first request's bytes, one
    less, the first value, one less than it, and 0."""
    pa, pb, sa, sb, _ = world
    t = next(s + 1 for s, x in enumerate(SHAPES) if x[0] == "random300_changed_150")
    u = next(s + 1 for s, x in enumerate(SHAPES) if x[0] == "random300_changed_7")
    full = BR.expected_diffs(sa, sb, [(u, None, None, None)], 1000)[1][0]
    origin = next(k for k, kind, v in full if kind != 1)  # (the first difference that carries a value)
    reqs = [(u, None, origin, None), (TWIN, None, None, None), (t, None, None, None), (ONLY_B, None, None, None)]
    n0 = len(BR.expected_diffs(sa, sb, reqs[:1], 1000)[1][0])
    mx = n0 + 30
    whole = BR.expected_diffs(sa, sb, reqs, mx)
    vals = [v for p in whole[1] for _, _, v in p]
    assert len(vals) == mx and whole[2] == 2
    total, first, head = sum(len(v) for v in vals), len(vals[0]), sum(len(v) for v in vals[:n0])
    assert first > 0
    batches = [(reqs, mx, cap) for cap in (total, total - 1, head, head - 1, first, first - 1, 0)]
    _, got, _ = _run(prog, tmp_path, pa, pb, batches)
    assert got == [BR.expected_diffs(sa, sb, *b) for b in batches]
    n = [sum(len(p) for p in g[1]) if g[0] == "pages" else None for g in got]
    assert n[0] == mx and n[1] < mx and n[2] >= n0 and n[3] < n0 and n[4] >= 1 and n[5:] == [None, None]
    assert got[5] == got[6] == ("nospc", first)


def test_host_empty_batches(prog, tmp_path, world):
    pa, pb, _, _, keys = world
    t = next(s + 1 for s, x in enumerate(SHAPES) if x[0] == "same_key_two_values")
    k = keys[t][0]
    batches = [([(TWIN, None, None, None)], 5, 100), ([(UNHELD, None, None, None), (TWIN, TWIN, None, None)], 5, 100),
               ([(t, None, DC.FF, DC.ZERO), (t, None, DC.RC._step(k, 1), None), (t, None, None, DC.RC._step(k, -1))], 5, 100)]
    _, got, cost = _run(prog, tmp_path, pa, pb, batches)
    assert got == [("pages", [[]] * len(b[0]), len(b[0]), None) for b in batches]
    assert cost[0] == cost[1] == (0, 0)  # equal roots: the root probes and no round
    _, got, _ = _run(prog, tmp_path, {}, {}, batches[:2], tag="none")  # stores without a record
    assert got == [("pages", [[]] * len(b[0]), len(b[0]), None) for b in batches[:2]]


def _needs_the_full_cut(nq):
    """A root branch of 16 leaves, all 16 with different values on the two sides, asked nq times for
    the 14 between the outer two: after the first round every request has 14 items holding a
    difference between two boundary items that are unskipped and turn out empty.  With max_entries
    one less than the 14 * nq differences, the difference `next` comes from lies under item
    max_entries + 2 * nq."""
    ks = [bytes([(c << 4) | 8]) + b"\x88" * 31 for c in range(16)]
    pa = [(k, bytes([c + 1]) * 5, False) for c, k in enumerate(ks)]
    pb = [(k, bytes([c + 101]) * 6, False) for c, k in enumerate(ks)]
    reqs = [(3, None, DC.RC._step(ks[0], 1), DC.RC._step(ks[15], -1))] * nq
    return pa, pb, ks, (reqs, 14 * nq - 1, BIG)


@pytest.mark.parametrize("nq", [1, 2, 3, 17])
def test_a_cut_one_item_smaller_is_seen(prog, tmp_path, oracle, nq):
    """The library's cut answers the constructed input; a frontier cut at max_entries + 2 * nq - 1
    items loses the item that holds thing max_entries + 1 (the answer then claims to be complete)."""
    pa, pb, ks, b = _needs_the_full_cut(nq)
    sa, sb = {3: _oracle(oracle, pa)}, {3: _oracle(oracle, pb)}
    want = BR.expected_diffs(sa, sb, *b)
    assert want[2] == nq - 1 and want[3] == ks[14] and sum(len(p) for p in want[1]) == 14 * nq - 1
    _, got, _ = _run(prog, tmp_path, {3: pa}, {3: pb}, [b])
    assert got == [want]
    _, got, _ = _run(prog, tmp_path, {3: pa}, {3: pb}, [b], less=1)
    assert got != [want] and got[0][2] == nq


def test_the_skip_test_after_the_cut_is_seen(prog, tmp_path, oracle):
    """Branch pairs of 16 children of which only the last differs, several such pairs a batch at small
    budgets: with the skip test made after the cut the equal children fill the frontier and
    differences are lost; made before it, every answer is right."""
    pa, pb = {}, {}
    for seed in range(4):
        pa[seed + 1], pb[seed + 1] = DC.sixteen_children_one_differs(seed)
    sa = {t: _oracle(oracle, p) for t, p in pa.items()}
    sb = {t: _oracle(oracle, p) for t, p in pb.items()}
    batches = [([(1 + (q % 4), None, None, None) for q in range(nq)], mx, BIG) for nq in (1, 2, 4) for mx in (1, 2, 3, 7, 13)]
    want = [BR.expected_diffs(sa, sb, *b) for b in batches]
    assert all(w[0] == "pages" and sum(len(p) for p in w[1]) == min(len(b[0]), b[1]) for w, b in zip(want, batches))
    assert _run(prog, tmp_path, pa, pb, batches)[1] == want
    got = _run(prog, tmp_path, pa, pb, batches, late=1)[1]
    assert sum(1 for w, g in zip(want, got) if w != g) >= 4
