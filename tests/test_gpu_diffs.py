"""GPU: many trie pairs of two forests (or many ranges of one pair) diffed in one call
(kh_trie_diffs_host / kh_dev_trie_diffs), held to tests/diffs_ref.expected_diffs over the oracle's
nodes for the batches of tests/diffs_cases.py (whose conditions tests/test_diffs_ref.py pins): the
pages under one budget, n_done and next, the fit to val_cap, forests loaded from nodes, forests and
their copy() after commits, hashed handles, versions, partial handles, the device-buffer form, the
refusals and the JNI wrapper."""
import ctypes
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

from tests import cases as C
from tests import diff_cases as DC
from tests import diff_ref as DR
from tests import diffs_cases as BC
from tests import diffs_ref as BR
from tests import proof_ref as P

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 1 << 26


def _answer(call):
    """A diffs call's answer in the form of diffs_ref.expected_diffs."""
    from khipu_amd import _lib
    try:
        pages, n_done, nxt = call()
    except _lib.MPTNodeMissingException as e:
        return ("missing", e.missing, e.request)
    except _lib.KhError as e:
        assert e.code == _lib.KH_ENOSPC
        return ("nospc", e.val_bytes)
    return ("pages", pages, n_done, nxt)


@pytest.fixture(scope="module")
def states(oracle):
    return BC.scenario_states(oracle)


@pytest.fixture(scope="module")
def pairs(oracle, states):
    """Per state pair of diffs_cases.RUNS: (side a, side b, one handle, the batches [(requests,
    max_entries, val_cap, the reference's answer)]), computed once."""
    out = {}
    for name in BC.RUNS:
        a, b, same, cand = BC.state_pair(oracle, name, states)
        batches = BC.batches_for(name, BC.full_diffs(a, b, same, cand), same)
        out[name] = (a, b, same, [x + (BR.expected_diffs(a, b, *x, same),) for x in batches])
    return out


def _from_nodes(ctx, side):
    from khipu_amd.device import ResidentForest
    held = {t: root for t, (_, root) in side.items() if root != P.EMPTY_ROOT}
    nodes = {}
    for t in held:
        nodes.update(side[t][0])
    return ResidentForest.from_nodes(ctx, held, nodes)


def _held(side):
    return {t: root for t, (_, root) in side.items() if root != P.EMPTY_ROOT}


def _check(fa, fb, same, batches, tag):
    for reqs, mx, cap, want in batches:
        assert _answer(lambda: fa.diffs(reqs, None if same else fb, mx, cap)) == want, (tag, len(reqs), mx, cap)


def test_scenario_states_as_ids_of_one_forest(khst, pairs):
    from khipu_amd.device import Ctx
    a, _, same, batches = pairs["ids"]
    f = _from_nodes(Ctx(0), a)
    assert same and f.roots() == _held(a)
    _check(f, f, True, batches, "ids")
    # the same forest named explicitly as the other side
    reqs, mx, cap, want = batches[3]
    assert _answer(lambda: f.diffs(reqs, f, mx, cap)) == want
    f.close()


@pytest.mark.parametrize("name", sorted(BC.VERSIONS))
def test_scenario_versions_as_two_forests(khst, pairs, name):
    from khipu_amd.device import Ctx
    a, b, same, batches = pairs[name]
    ctx = Ctx(0)
    fa, fb = _from_nodes(ctx, a), _from_nodes(ctx, b)
    _check(fa, fb, False, batches, name)
    for h in (fa, fb):
        h.close()


def test_scenario_versions_as_a_forest_and_its_copies(khst, states, pairs):
    """One forest follows the scenarios' batches, copy() is taken at each version: a copy has the
    forest's roots, and commits on the forest afterwards leave it alone; what the version pairs hold
    beside the scenarios is committed on copies of the copies, independently."""
    from khipu_amd.device import Ctx, ResidentForest
    ctx = Ctx(0)
    f = ResidentForest(ctx)
    f.commit([(s + 1, k, v) for s, (_, ks, vs, _) in enumerate(BC.SCEN) for k, v in zip(ks, vs)], [])
    copies = [f.copy()]
    assert copies[0].roots() == f.roots() == _held(BC.version(states, 0))
    for v in (1, 2):
        ups = [(s + 1, k, val) for s, sc in enumerate(BC.SCEN) if len(sc[3]) >= v for k, val in sc[3][v - 1][0]]
        dels = [(s + 1, k) for s, sc in enumerate(BC.SCEN) if len(sc[3]) >= v for k in sc[3][v - 1][1]]
        f.commit(ups, dels)
        copies.append(f.copy())
        assert copies[v].roots() == f.roots() == _held(BC.version(states, v)), v
    assert copies[0].roots() == _held(BC.version(states, 0)) and copies[1].roots() == _held(BC.version(states, 1))
    content = {t: [(k, v) for k, v, _ in DR.content(*st)] for t, st in
               ((BC.ONLY_A_ID, states[1][0]), (BC.ONLY_B_ID, states[1][1]), (BC.TWIN_ID, states[0][0]))}
    for name, (va, vb) in sorted(BC.VERSIONS.items()):
        a, b, _, batches = pairs[name]
        fa, fb = copies[va].copy(), copies[vb].copy()
        fa.commit([(t, k, v) for t in (BC.ONLY_A_ID, BC.TWIN_ID) for k, v in content[t]], [])
        fb.commit([(t, k, v) for t in (BC.ONLY_B_ID, BC.TWIN_ID) for k, v in content[t]], [])
        assert fa.roots() == _held(a) and fb.roots() == _held(b), name
        _check(fa, fb, False, batches[:25], name)
        for h in (fa, fb):
            h.close()
    assert copies[2].roots() == _held(BC.version(states, 2))  # (the copies of a copy left it alone)
    for h in copies + [f]:
        h.close()


def _forest60(oracle, hashed):
    """(forest a, its copy after the block, side a, side b of the reference)"""
    from khipu_amd.device import Ctx, ResidentForest
    puts, (ups, dels), twins = BC.forest60_ops(oracle)
    key = (lambda k: k) if hashed else oracle.kec256
    fa = ResidentForest(Ctx(0), hash_keys=hashed)
    fa.commit([(t, key(k), v) for t, k, v in puts], [])
    fb = fa.copy()
    fb.commit([(t, key(k), v) for t, k, v in ups], [(t, key(k)) for t, k in dels])
    a, b = BC.forest60_pair(oracle)
    assert fa.roots() == _held(a) and fb.roots() == _held(b) and fa.roots() != fb.roots()
    assert a[twins[0]][1] == a[twins[1]][1] == b[twins[0]][1] and max(a) >= 1 << 16
    return fa, fb, a, b


@pytest.mark.parametrize("hashed", [False, True], ids=["plain", "hash_keys"])
def test_forest60_against_its_copy_after_a_block(khst, oracle, pairs, hashed):
    fa, fb, a, b = _forest60(oracle, hashed)
    _, _, _, batches = pairs["forest60"]
    _check(fa, fb, False, batches, "forest60")
    for h in (fa, fb):
        h.close()


def _raw_diffs(fa, fb, ta, nq, mx, cap):
    """kh_trie_diffs_host over whole tries, the output arrays as bytes."""
    from khipu_amd import _lib
    tb = np.asarray(ta + [0], np.uint32)
    keys, kinds = np.zeros(32 * mx, np.uint8), np.zeros(mx, np.uint8)
    vals, voff, eoff = np.zeros(cap, np.uint8), np.zeros(mx + 1, np.uint64), np.zeros(nq + 1, np.uint64)
    ne, vb, nd = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    nxt = np.zeros(32, np.uint8)
    fa.ctx._sync()
    fb.ctx._sync()
    rc = _lib.lib().kh_trie_diffs_host(fa.h, tb.ctypes.data, fb.h, None, None, None, nq, mx, cap, keys.ctypes.data,
                                       kinds.ctypes.data, vals.ctypes.data, voff.ctypes.data, eoff.ctypes.data,
                                       ctypes.byref(ne), ctypes.byref(vb), ctypes.byref(nd), nxt.ctypes.data, None)
    assert rc == _lib.KH_OK
    k = int(ne.value)
    return (keys[:32 * k].tobytes(), kinds[:k].tobytes(), vals[:int(vb.value)].tobytes(), [int(x) for x in voff[:k + 1]],
            [int(x) for x in eoff], int(nd.value))


def test_a_batch_is_the_stitched_single_calls(khst, oracle):
    """Every pair of the 60-trie forest in one call against one kh_trie_diff_host call a pair: keys,
    kinds, values and offsets byte for byte."""
    from khipu_amd import _lib
    fa, fb, a, b = _forest60(oracle, False)
    ids = sorted(set(a) | set(b)) + [BC.UNHELD[0]]
    nq, mx, cap = len(ids), 4096, 1 << 18
    keys, kinds, vals, voff, eoff, n_done = _raw_diffs(fa, fb, ids, nq, mx, cap)
    assert n_done == nq and eoff[nq] == len(kinds) > 20
    sk, sd, sv, so, se = b"", b"", b"", [0], [0]
    for t in ids:
        k1, d1 = np.zeros(32 * mx, np.uint8), np.zeros(mx, np.uint8)
        v1, o1 = np.zeros(cap, np.uint8), np.zeros(mx + 1, np.uint64)
        ne, vb, more = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_int(0)
        nxt = np.zeros(32, np.uint8)
        assert _lib.lib().kh_trie_diff_host(fa.h, t, fb.h, t, None, None, mx, cap, k1.ctypes.data, d1.ctypes.data,
                                            v1.ctypes.data, o1.ctypes.data, ctypes.byref(ne), ctypes.byref(vb),
                                            ctypes.byref(more), nxt.ctypes.data, None) == _lib.KH_OK
        n = int(ne.value)
        assert not more.value
        so += [len(sv) + int(x) for x in o1[1:n + 1]]
        sk, sd, sv = sk + k1[:32 * n].tobytes(), sd + d1[:n].tobytes(), sv + v1[:int(vb.value)].tobytes()
        se.append(len(sd))
    assert (keys, kinds, vals, voff, eoff) == (sk, sd, sv, so, se)
    for h in (fa, fb):
        h.close()


def test_following_n_done_and_next_to_the_end(khst, oracle):
    """Budgets 1, 7 and 1,000 paged to the end give every pair's whole difference list; changes_all
    committed on a copy of side a gives side b's roots."""
    fa, fb, a, b = _forest60(oracle, False)
    ids = sorted(set(a) | set(b))
    full = BC.full_diffs(a, b, False, [(t, t) for t in ids])
    want = {t: ([(k, v) for k, kind, v in d if kind != 1], [k for k, kind, _ in d if kind == 1])
            for (t, _), d in full.items() if d}
    assert len(want) >= 20
    for chunk in (1, 7, 1000):
        assert fa.changes_all(fb, ids, chunk=chunk) == want, chunk
    assert fa.changes_all(fb) == want  # (the ids from both sides' roots, equal roots dropped on the host)
    c = fa.copy()
    c.commit([(t, k, v) for t, (ups, _) in want.items() for k, v in ups],
             [(t, k) for t, (_, dels) in want.items() for k in dels])
    assert c.roots() == fb.roots() != fa.roots()
    assert c.changes_all(fb) == {} and c.diffs([(t, None, None, None) for t in ids], fb) == ([[]] * len(ids), len(ids), None)
    for h in (fa, fb, c):
        h.close()


def test_val_cap_edges_and_nospc(khst, oracle):
    from khipu_amd.device import _diffs_changes
    fa, fb, a, b = _forest60(oracle, False)
    ids = sorted(set(a) | set(b))
    reqs = [(t, None, None, None) for t in ids]
    whole = BR.expected_diffs(a, b, reqs, 40)
    vals = [v for p in whole[1] for _, _, v in p]
    first_q = next(q for q, p in enumerate(whole[1]) if p)
    if not vals[0]:  # (start at a difference that carries a value)
        k0 = next(k for k, kind, v in whole[1][first_q] if v)
        reqs = [(ids[first_q], None, k0, None)] + reqs[first_q + 1:]
        whole = BR.expected_diffs(a, b, reqs, 40)
        vals = [v for p in whole[1] for _, _, v in p]
    assert len(vals) == 40 and vals[0]
    total, first = sum(len(v) for v in vals), len(vals[0])
    caps = (total, total - 1, first, first - 1, 0)
    got = [_answer(lambda: fa.diffs(reqs, fb, 40, cap)) for cap in caps]
    assert got == [BR.expected_diffs(a, b, reqs, 40, cap) for cap in caps]
    assert sum(len(p) for p in got[0][1]) == 40 and sum(len(p) for p in got[1][1]) < 40
    assert got[3] == got[4] == ("nospc", first)
    # the paging grows val_cap when a value does not fit
    full = BC.full_diffs(a, b, False, [(t, t) for t in ids])
    out = _diffs_changes(fa.h, True, fb.h, True, [(t, None) for t in ids], 50, val_cap=1)
    assert out == [([(k, v) for k, kind, v in full[(t, t)] if kind != 1], [k for k, kind, _ in full[(t, t)] if kind == 1])
                   for t in ids]
    for h in (fa, fb):
        h.close()


def _two(oracle, n, nchanged, seed):
    """(keys, values, oracle snap of a, of b, upserts, deletes) -- nchanged keys of n updated, gone or new."""
    r = random.Random(seed)
    ks = sorted(C._rk(r) for _ in range(n))
    vs = [C.account_value(r) if i % 3 else C.storage_value(r) for i in range(n)]
    o = oracle.Trie()
    for k, v in zip(ks, vs):
        o.put(k, v)
    sa = DC.snap(o)
    ch = r.sample(ks, nchanged)
    ups = [(k, C.account_value(r)) for k in ch[::3]] + [(C._rk(r), C.account_value(r)) for _ in ch[1::3]]
    dels = ch[2::3]
    DC.fold(o, ups, dels)
    return ks, vs, sa, DC.snap(o), ups, dels


def _ranges_of(r, keys, n):
    return [(o, l) for o, l, _ in DC.RC.random_ranges(r, keys, n)]


def test_identical_pairs_take_no_round(khst, oracle):
    from khipu_amd.device import diffs_counters
    fa, fb, a, b = _forest60(oracle, False)
    same = sorted(t for t in a if t in b and a[t][1] == b[t][1])
    assert len(same) >= 20
    reqs = [(t, None, None, None) for t in same] + [(BC.UNHELD[0], None, None, None), (same[0], None, DC.FF, DC.ZERO)]
    assert fa.diffs(reqs, fb) == ([[]] * len(reqs), len(reqs), None) and diffs_counters() == (0, 0)
    ids = sorted(a)
    assert fa.diffs([(t, None, None, None) for t in ids]) == ([[]] * len(ids), len(ids), None)  # (itself)
    assert diffs_counters() == (0, 0)
    c = fa.copy()
    assert fa.diffs([(t, None, None, None) for t in ids], c) == ([[]] * len(ids), len(ids), None)
    assert diffs_counters() == (0, 0)
    changed = next(t for t in ids if t in b and a[t][1] != b[t][1])
    pages, n_done, _ = fa.diffs(reqs + [(changed, None, None, None)], fb)
    assert n_done == len(reqs) + 1 and pages[-1] and 0 < diffs_counters()[0] <= 68
    for h in (fa, fb, c):
        h.close()


def test_sixty_four_ranges_of_a_large_pair(khst, oracle):
    """nq = 64 over a 2,000-key pair with 5 changed keys: the first frontier alone spans four blocks
    of the fill; single-trie handles, several ranges of the one pair."""
    from khipu_amd.device import Ctx, ResidentTrie, diffs_counters
    ks, vs, sa, sb, ups, dels = _two(oracle, 2000, 5, 77)
    ctx = Ctx(0)
    ta = ResidentTrie(ctx, ks, vs, emit=False)
    tb = ta.copy()
    assert tb.commit(ups, dels) == sb[1]
    full = [t[1] for t in DR.walk_diff(*sa, *sb)]
    assert len(full) == 5
    r = random.Random(6)
    one = [(None, None)] * 3 + [(full[0], full[0]), (DC.RC._step(full[0], 1), full[4]), (None, DC.RC._step(full[0], -1))]
    one += _ranges_of(r, ks, 64 - len(one))
    reqs = [(0, None, o, l) for o, l in one]
    for mx, cap in ((1000, BIG), (7, BIG), (1, BIG), (1000, 100)):
        got = _answer(lambda: ta.diffs(one, tb, mx, cap))
        assert got == BR.expected_diffs({0: sa}, {0: sb}, reqs, mx, cap), (mx, cap)
    rounds, visited = diffs_counters()
    assert 0 < rounds <= 68 and 0 < visited < 64 * 200
    assert _answer(lambda: ta.diffs(one, ta)) == ("pages", [[]] * 64, 64, None)
    # a single trie against a trie of a forest, and the forest against the single trie
    from khipu_amd.device import ResidentForest
    f = ResidentForest.from_nodes(ctx, {9: sb[1]}, sb[0])
    assert _answer(lambda: ta.diffs(one[:9], f, 7, BIG, other_trie=9)) == BR.expected_diffs({0: sa}, {0: sb}, reqs[:9], 7, BIG)
    back = [(9, None, o, l) for o, l in one[:9]]
    assert _answer(lambda: f.diffs(back, ta, 7, BIG)) == BR.expected_diffs({9: sb}, {9: sa}, back, 7, BIG)
    for h in (ta, tb, f):
        h.close()


def test_versions_compact_and_two_contexts(khst, oracle):
    """Under a savepoint the call reads the commits since; after rollback the version before; a
    compacted forest diffs the same; forests on two contexts (two streams) as well."""
    from khipu_amd.device import Ctx
    fa, fb, a, b = _forest60(oracle, False)
    _, (ups, dels), _ = BC.forest60_ops(oracle)
    ids = sorted(set(a) | set(b))
    reqs = [(t, None, None, None) for t in ids]
    want, back = BR.expected_diffs(a, b, reqs, 1000), BR.expected_diffs(b, a, reqs, 1000)
    none = ("pages", [[]] * len(ids), len(ids), None)
    t = fa.copy()
    t.savepoint()
    t.commit([(u, oracle.kec256(k), v) for u, k, v in ups], [(u, oracle.kec256(k)) for u, k in dels])
    assert _answer(lambda: fa.diffs(reqs, t, 1000)) == want and _answer(lambda: t.diffs(reqs, fa, 1000)) == back
    assert _answer(lambda: t.diffs(reqs, fb, 1000)) == none
    t.rollback()
    assert _answer(lambda: fa.diffs(reqs, t, 1000)) == none and _answer(lambda: t.diffs(reqs, fb, 1000)) == want
    fb.compact()
    fa.compact()
    assert _answer(lambda: fa.diffs(reqs, fb, 1000)) == want and _answer(lambda: fb.diffs(reqs, fa, 1000)) == back
    other = _from_nodes(Ctx(0), b)  # (a context, and a stream, of its own)
    assert _answer(lambda: fa.diffs(reqs, other, 1000)) == want and _answer(lambda: other.diffs(reqs, fb, 1000)) == none
    assert _answer(lambda: other.diffs(reqs, fa, 7)) == BR.expected_diffs(b, a, reqs, 7)
    for h in (fa, fb, t, other):
        h.close()


def test_partial_handles(khst, oracle):
    """Partial handles opened from a witness directly: stubs skipped by their references cost
    nothing; a stub that is not skipped gives KH_ENODE with the hash and the request the reference
    names, and only when it is among the first max_entries + 1 things."""
    from khipu_amd.device import Ctx, ResidentTrie
    r = random.Random(51)
    ks = sorted(C._rk(r) for _ in range(300))
    vs = [C.account_value(r) if i % 4 else C.storage_value(r) for i in range(len(ks))]
    some = r.sample(ks, 25)
    o = oracle.Trie()
    for k, v in zip(ks, vs):
        o.put(k, v)
    sa = DC.snap(o)
    ups = [(k, C.account_value(r)) for k in some[:10]]
    DC.fold(o, ups, [])
    sb = DC.snap(o)

    def witness(s):
        w = {s[1]: s[0][s[1]]}
        for k in some:
            w.update({P.kec(e): e for e in P.expected_proof(s[0], s[1], k)[0]})
        return w
    wa, wb = witness(sa), witness(sb)
    ctx = Ctx(0)
    fa = ResidentTrie(ctx, ks, vs, emit=False)
    fb = fa.copy()
    assert fb.commit(ups, []) == sb[1]
    pa = ResidentTrie.from_witness(ctx, sa[1], wa, emit=False)
    pb = ResidentTrie.from_witness(ctx, sb[1], wb, emit=False)
    assert pa.stubs > 0 and pb.stubs > 0
    changed = sorted(k for k, _ in ups)
    one = [(None, changed[2]), (changed[3], changed[3]), (DC.RC._step(changed[3], 1), None), (None, None)]
    reqs = [(0, None, o_, l) for o_, l in one]
    want = BR.expected_diffs({0: sa}, {0: sb}, reqs, 1000)
    assert [len(p) for p in want[1]] == [3, 1, 6, 10]
    for x, y, nx, ny in ((fa, pb, sa[0], wb), (pa, fb, wa, sb[0]), (pa, pb, wa, wb)):
        for mx in (1000, 3, 4):
            assert BR.expected_diffs({0: (nx, sa[1])}, {0: (ny, sb[1])}, reqs, mx) == BR.expected_diffs({0: sa}, {0: sb}, reqs, mx)
            assert _answer(lambda: x.diffs(one, y, mx)) == BR.expected_diffs({0: sa}, {0: sb}, reqs, mx)
    # a change outside the witness: the stub over it is not skipped
    out = next(k for k in ks if k not in some and P.kec(P.expected_proof(sb[0], sb[1], k)[0][-1]) not in wb)
    fc = fb.copy()
    assert fc.commit([(out, b"\x07" * 50)], []) == (DC.fold(o, [(out, b"\x07" * 50)], []) or o.root_hash())
    sc = DC.snap(o)
    lo = [k for k in changed if k < out]
    two = [(None, DC.RC._step(out, -1)), (None, None)]
    reqs2 = [(0, None, o_, l) for o_, l in two]
    want = BR.expected_diffs({0: (wb, sb[1])}, {0: sc}, reqs2, 1000)
    assert want[0] == "missing" and want[1] in sb[0] and want[1] not in wb and want[2] in (0, 1)
    assert _answer(lambda: pb.diffs(two, fc, 1000)) == want
    assert _answer(lambda: fc.diffs(two, pb, 1000)) == BR.expected_diffs({0: sc}, {0: (wb, sb[1])}, reqs2, 1000)
    for mx in (1, 2):  # named only when it is among the first max_entries + 1 things
        assert _answer(lambda: pa.diffs(two, fc, mx)) == BR.expected_diffs({0: (wa, sa[1])}, {0: sc}, reqs2, mx), (mx, len(lo))
    for h in (fa, fb, fc, pa, pb):
        h.close()


def test_device_buffers(khst, oracle):
    """kh_dev_trie_diffs: requests and answer in device buffers, equal to the host form."""
    import torch
    from khipu_amd import _lib
    fa, fb, a, b = _forest60(oracle, False)
    ids = sorted(set(a) | set(b))
    full = BC.full_diffs(a, b, False, [(t, t) for t in ids])
    ch = [t for t in ids if len(full[(t, t)]) >= 2][:9]
    reqs = [(t, None, full[(t, t)][0][0] if i % 3 == 1 else None, full[(t, t)][-1][0] if i % 3 == 2 else None)
            for i, t in enumerate(ch)] + [(BC.UNHELD[0], None, None, None)]
    nq, cap = len(reqs), 1 << 16
    mx = sum(len(p) for p in fa.diffs(reqs, fb, 1 << 12, cap)[0]) // 2
    want = fa.diffs(reqs, fb, mx, cap)
    assert mx >= 9 and want[1] < nq - 1  # (cut: next is read too)

    def dev(x):
        return torch.from_numpy(x).to("cuda:0")
    dt = dev(np.asarray([t for t, _, _, _ in reqs], np.uint32).view(np.int32))
    dor = dev(np.frombuffer(b"".join(o or DC.ZERO for _, _, o, _ in reqs), np.uint8).copy())
    dli = dev(np.frombuffer(b"".join(l or DC.FF for _, _, _, l in reqs), np.uint8).copy())
    dk = torch.zeros(32 * mx, dtype=torch.uint8, device="cuda:0")
    dkind = torch.zeros(mx, dtype=torch.uint8, device="cuda:0")
    dv = torch.zeros(cap, dtype=torch.uint8, device="cuda:0")
    do = torch.zeros(mx + 1, dtype=torch.int64, device="cuda:0")
    de = torch.zeros(nq + 1, dtype=torch.int64, device="cuda:0")
    ne, vb, nd = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    nxt = np.zeros(32, np.uint8)
    fa.ctx._sync()
    fb.ctx._sync()
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    for dtb in (None, p(dt)):  # (tries_b NULL: tries_a)
        rc = _lib.lib().kh_dev_trie_diffs(fa.h, p(dt), fb.h, dtb, p(dor), p(dli), nq, mx, cap, p(dk), p(dkind), p(dv),
                                          p(do), p(de), ctypes.byref(ne), ctypes.byref(vb), ctypes.byref(nd),
                                          nxt.ctypes.data, None)
        assert rc == _lib.KH_OK and ne.value == mx
        off, eo = do.cpu().numpy(), de.cpu().numpy()
        kb, kinds, vbuf = dk.cpu().numpy().tobytes(), dkind.cpu().numpy(), dv.cpu().numpy().tobytes()
        assert int(off[mx]) == vb.value and int(eo[nq]) == mx
        pages = [[(kb[32 * i:32 * i + 32], int(kinds[i]), vbuf[int(off[i]):int(off[i + 1])])
                  for i in range(int(eo[q]), int(eo[q + 1]))] for q in range(nq)]
        assert (pages, int(nd.value), nxt.tobytes()) == want
    for h in (fa, fb):
        h.close()


def test_refusals_leave_the_outputs_untouched(khst, oracle):
    from khipu_amd import _lib
    from khipu_amd.device import Ctx, ResidentTrie
    fa, fb, a, b = _forest60(oracle, False)
    t1 = ResidentTrie(Ctx(0), [b"\x01" * 32], [b"\x02"], emit=False)
    t2 = ResidentTrie(Ctx(0), [b"\x01" * 32, b"\x03" * 32], [b"\x04", b"\x05"], emit=False)
    L = _lib.lib()
    ids = sorted(t for t in a if t in b and a[t][1] != b[t][1])[:3]
    nq = 3
    tb = np.asarray(ids, np.uint32)
    bufs = {n: np.full(s, 0xAB, np.uint8) for n, s in (("keys", 32 * 8), ("kinds", 8), ("vals", 256), ("voff", 8 * 9),
                                                        ("eoff", 8 * (nq + 1)), ("next", 32), ("miss", 32))}
    sc = [ctypes.c_uint64(0xABABABAB) for _ in range(3)]

    def call(ha=None, hb=None, tries=tb, tries_b=None, nq=nq, mx=8, cap=256, drop=()):
        x = {n: (None if n in drop else v.ctypes.data) for n, v in bufs.items()}
        s = [None if f"s{i}" in drop else ctypes.byref(sc[i]) for i in range(3)]
        return L.kh_trie_diffs_host(None if "a" in drop else (ha or fa.h), tries.ctypes.data if tries is not None else None,
                                    None if "b" in drop else (hb or fb.h),
                                    tries_b.ctypes.data if tries_b is not None else None, None, None, nq, mx, cap,
                                    x["keys"], x["kinds"], x["vals"], x["voff"], x["eoff"], s[0], s[1], s[2], x["next"],
                                    x["miss"])

    bad = [dict(nq=0), dict(mx=0), dict(mx=(1 << 31) - nq), dict(mx=1 << 31), dict(tries=None),
           dict(ha=t1.h, tries=None), dict(tries=None, tries_b=tb)]
    bad += [dict(drop=(n,)) for n in ("a", "b", "keys", "kinds", "voff", "eoff", "next", "s0", "s1", "s2")]
    for kw in bad:
        assert call(**kw) == _lib.KH_EINVAL, kw
        assert all((v == 0xAB).all() for v in bufs.values()) and all(s.value == 0xABABABAB for s in sc), kw
    # single tries: the ids may be NULL; a forest b with ids of its own beside a single a
    assert call(ha=t1.h, hb=t2.h, tries=None) == _lib.KH_OK and sc[0].value == 6 and sc[2].value == 3
    assert call(ha=t1.h, tries=None, tries_b=tb) == _lib.KH_OK
    # KH_ENOSPC writes *val_bytes alone
    for v in bufs.values():
        v[:] = 0xAB
    sc[0].value = sc[2].value = 0xABABABAB
    sc[1].value = 0xABABABAB
    assert call(ha=t1.h, hb=t2.h, tries=None, cap=0) == _lib.KH_ENOSPC  # (the first difference carries one byte)
    assert sc[1].value == 1 and sc[0].value == sc[2].value == 0xABABABAB
    assert all((v == 0xAB).all() for v in bufs.values())
    with pytest.raises(_lib.MPTException):
        fa.diffs([(ids[0], None, b"\x00" * 31, None)], fb)
    with pytest.raises(_lib.MPTException):
        fa.diffs([], fb)
    for h in (fa, fb, t1, t2):
        h.close()


def test_diffs_through_the_jni_shim(khst, oracle, tmp_path):
    """Khst.diffs through the in-process JNIEnv of tests/jni_stub: two single tries, batches of ranges
    of the pair followed to their end by n_done / next, with a value array that starts empty, so the
    grow path runs."""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    stub = os.path.join(ROOT, "tests", "jni_stub")
    exe = tmp_path / "jni_diffs_driver"
    rc = subprocess.run([cc, "-std=gnu99", "-O1", "-Wall", "-Werror", "-I", stub, "-I", os.path.join(ROOT, "include"),
                         "-o", str(exe), os.path.join(stub, "jni_diffs_driver.c"), os.path.join(stub, "fake_env.c"),
                         os.path.join(ROOT, "jni", "khst_jni.c"), "-L", os.path.join(ROOT, "khipu_amd"), "-lkhst",
                         "-Wl,-rpath," + os.path.join(ROOT, "khipu_amd"), "-Wl,-rpath-link,/opt/rocm/lib"],
                        capture_output=True, text=True)
    assert rc.returncode == 0, rc.stderr
    ks, vs, sa, sb, ups, dels = _two(oracle, 400, 90, 808)

    def packed(keys, vals):
        voff = np.zeros(len(vals) + 1, np.uint64)
        voff[1:] = np.cumsum([len(v) for v in vals])
        return np.uint64(len(keys)).tobytes() + b"".join(keys) + voff.tobytes() + b"".join(vals)
    full = [(t[1], t[2], t[3]) for t in DR.walk_diff(*sa, *sb)]
    dk = [k for k, _, _ in full]
    batches = [([(DC.ZERO, DC.FF)], 64),
               ([(dk[10], dk[30]), (DC.FF, DC.ZERO), (DC.RC._step(dk[3], 1), dk[5]), (dk[-1], DC.FF)], 7),
               ([(dk[i], dk[i + 4]) for i in range(0, 60, 5)], 1),
               ([(DC.ZERO, dk[20]), (dk[70], DC.FF)], 1000)]
    p = tmp_path / "in.bin"
    with open(p, "wb") as f:
        f.write(packed(ks, vs) + packed([k for k, _ in ups], [v for _, v in ups]))
        f.write(np.uint64(len(dels)).tobytes() + b"".join(dels))
        f.write(np.uint64(len(batches)).tobytes())
        for reqs, mx in batches:
            f.write(np.uint64(len(reqs)).tobytes() + np.uint64(mx).tobytes() + b"".join(x + y for x, y in reqs))
    rc = subprocess.run([str(exe), str(p)], capture_output=True, text=True, timeout=120)
    assert rc.returncode == 0, rc.stderr
    lines = [ln.split() for ln in rc.stdout.split("\n")[:-1]]
    assert lines[-1] == ["E", "0"], lines[-1]
    assert bytes.fromhex(lines[0][1]) == sb[1]
    for j, (reqs, mx) in enumerate(batches):
        total = 0
        for q, (x, y) in enumerate(reqs):
            got = [(bytes.fromhex(ln[3]), int(ln[4]), b"" if ln[5] == "-" else bytes.fromhex(ln[5])) for ln in lines
                   if ln[0] == "K" and ln[1] == str(j) and ln[2] == str(q)]
            want = [d for d in full if x <= d[0] <= y]
            assert got == want, (j, q)
            total += len(want)
        _, n, calls, grows = [ln for ln in lines if ln[0] == "Q" and ln[1] == str(j)][0][1:]
        assert int(n) == total and int(calls) >= max(1, -(-total // mx)) and int(grows) >= 1
