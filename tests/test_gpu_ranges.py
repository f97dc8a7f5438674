"""GPU: many key ranges of a forest (or of one trie) answered in one call (kh_trie_ranges_host /
kh_dev_trie_ranges), held to tests/ranges_ref.py over the oracle's nodes: the pages under one entry
and byte budget, n_done and next, the refusals, partial handles, and the loop closed through
ranges_proof into verify_ranges.  The batches are tests/ranges_cases.py's; tests/test_ranges_ref.py
pins, without a GPU, that they cut in every way."""
import ctypes
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

from tests import cases as C
from tests import proof_ref as P
from tests import range_cases as RC
from tests import range_ref as RR
from tests import ranges_cases as BC
from tests import ranges_ref as BR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_STATES = {}


def _state(oracle, name):
    """(tries {id: (nodes, root)}, content, batches, the reference's answers) of a state, computed once."""
    if name not in _STATES:
        tries = BC.state(oracle, name)
        content = {t: RR.content(nodes, root) for t, (nodes, root) in tries.items()}
        batches = BC.batches_for(name, content)
        _STATES[name] = (tries, content, batches, [BR.expected_ranges(tries, *b) for b in batches])
    return _STATES[name]


def _load(tries, hashed=False, partial=False):
    from khipu_amd.device import Ctx, ResidentForest
    f = ResidentForest(Ctx(0), hash_keys=hashed, emit=False)
    nodes = {}
    for n, _ in tries.values():
        nodes.update(n)
    f.load_nodes({t: root for t, (_, root) in tries.items()}, nodes, partial=partial)
    return f


def _ans(call):
    """A ranges call's answer in the form of ranges_ref.expected_ranges."""
    from khipu_amd import _lib
    try:
        pages, n_done, nxt = call()
    except _lib.MPTNodeMissingException as e:
        return ("missing", e.missing, e.request)
    except _lib.KhError as e:
        assert e.code == _lib.KH_ENOSPC
        return ("nospc", e.val_bytes)
    return ("pages", pages, n_done, nxt)


@pytest.mark.parametrize("name,hashed", [("scenarios", False), ("forest60", False), ("forest60", True), ("big", False)])
def test_batches_match_the_reference(khst, oracle, name, hashed):
    """Every generated batch on a plain handle and on a KH_HASH_KEYS handle (whose pages hold the
    trie keys it was loaded with)."""
    tries, _, batches, wants = _state(oracle, name)
    f = _load(tries, hashed)
    for (reqs, mx, cap), want in zip(batches, wants):
        assert _ans(lambda: f.ranges(reqs, mx, cap)) == want, (name, len(reqs), mx, cap)
    f.close()


def _stitched(f, reqs, mx, cap):
    """The nq single range calls stitched under the batch's budget rule."""
    from khipu_amd import _lib
    pages, rem, left = [([], []) for _ in reqs], mx, cap
    for q, (t, o, l) in enumerate(reqs):
        try:
            keys, vals, more, nxt = f.range(t, o, l, max(rem, 1), left if rem else BC.BIG)
        except _lib.KhError as e:
            assert e.code == _lib.KH_ENOSPC
            if rem == mx:
                return ("nospc", e.val_bytes)
            keys, vals, more, nxt = [], [], True, f.range(t, o, l, 1, BC.BIG)[0][0]
        if rem == 0 and keys:  # the budget ended exactly before this request's first entry
            keys, vals, more, nxt = [], [], True, keys[0]
        pages[q] = (keys, vals)
        if more:
            return ("pages", pages, q, nxt)
        rem -= len(keys)
        left -= sum(len(v) for v in vals)
    return ("pages", pages, len(reqs), None)


def test_a_batch_equals_its_single_calls(khst, oracle):
    tries, _, batches, wants = _state(oracle, "forest60")
    f = _load(tries)
    for (reqs, mx, cap), want in list(zip(batches, wants))[:30]:
        got = _ans(lambda: f.ranges(reqs, mx, cap))
        assert got == _stitched(f, reqs, mx, cap) == want, (len(reqs), mx, cap)
    f.close()


def _follow(f, reqs, budget, cap=BC.BIG):
    """Every request's entries, following n_done / next until the batch is done; -> (pages, calls)."""
    out = [([], []) for _ in reqs]
    todo, first, calls = list(reqs), 0, 0
    while todo:
        pages, n_done, nxt = f.ranges(todo, budget, cap)
        calls += 1
        for q, (ks, vs) in enumerate(pages):
            assert q <= n_done or not ks
            out[first + q][0].extend(ks)
            out[first + q][1].extend(vs)
        if n_done < len(todo):
            t, _, l = todo[n_done]
            todo[n_done] = (t, nxt, l)
        todo, first = todo[n_done:], first + n_done
    return out, calls


@pytest.mark.parametrize("name,budget", [("forest60", 1), ("forest60", 7), ("forest60", 1000), ("big", 7),
                                         ("big", 1000), ("scenarios", 1000)])
def test_following_next_returns_everything(khst, oracle, name, budget):
    tries, content, _, _ = _state(oracle, name)
    f = _load(tries)
    ids = list(tries) + [BC.UNHELD]
    if name == "scenarios":
        ids = ids[:6] + ids[-4:]
    got, calls = _follow(f, [(t, None, None) for t in ids], budget)
    for t, (ks, vs) in zip(ids, got):
        assert list(zip(ks, vs)) == content.get(t, []), t
    total = sum(len(content.get(t, [])) for t in ids)
    assert calls == max(1, -(-total // budget))
    f.close()


def test_val_cap_edges_and_nospc(khst, oracle):
    """The cap exactly the bytes of the first k entries, and one byte less, for k inside a request
    and at a request's first entry; KH_ENOSPC reports the first value's size."""
    tries, content, _, _ = _state(oracle, "forest60")
    f = _load(tries)
    ids = [t for t in tries if len(content[t]) >= 3][:4]
    reqs = [(ids[0], None, None), (BC.EMPTY_IDS[0], None, None), (ids[1], content[ids[1]][1][0], None),
            (ids[2], None, None), (ids[3], None, None)]
    vals = [v for _, vs in BR.expected_ranges(tries, reqs, 1 << 20)[1] for v in vs]
    n0 = len(content[ids[0]])
    for k in (1, 2, n0, n0 + 1, len(vals) - 1, len(vals)):
        exact = sum(len(v) for v in vals[:k])
        for cap in (exact, exact - 1):
            got = _ans(lambda: f.ranges(reqs, 1 << 20, cap))
            assert got == BR.expected_ranges(tries, reqs, 1 << 20, cap), (k, cap)
            if got[0] == "pages":
                assert sum(len(ks) for ks, _ in got[1]) == (k if cap == exact else k - 1)
    first = len(vals[0])
    assert _ans(lambda: f.ranges(reqs, 5, first - 1)) == ("nospc", first) == _ans(lambda: f.ranges(reqs, 5, 0))
    # (an empty request and an unheld one before the entry that does not fit)
    lead = [(BC.UNHELD, None, None), (BC.EMPTY_IDS[1], None, None)] + reqs
    assert _ans(lambda: f.ranges(lead, 5, first - 1)) == ("nospc", first)
    f.close()


def _grown(oracle, r, n_tries=6):
    """A forest grown by a commit, with the oracle's tries: (forest, {id: oracle trie})."""
    from khipu_amd.device import Ctx, ResidentForest
    f = ResidentForest(Ctx(0), emit=False)
    ids = [r.randrange(1 << 32) for _ in range(n_tries)]
    o = {t: oracle.Trie() for t in ids}
    ups = [(t, C._rk(r), C.storage_value(r)) for t in ids for _ in range(r.choice([2, 9, 30]))]
    roots = f.commit(ups)
    for t, k, v in ups:
        o[t].put(k, v)
    assert all(roots[t] == o[t].root_hash() for t in ids)
    return f, o


def _stores(o):
    out = {t: (x.reachable() if x.root_hash() != P.EMPTY_ROOT else {}, x.root_hash()) for t, x in o.items()}
    for e in BC.EMPTY_IDS:
        out[e] = ({}, P.EMPTY_ROOT)
    return out


def _check(f, stores, r, n, tag):
    content = {t: RR.content(nodes, root) for t, (nodes, root) in stores.items()}
    for reqs, mx, cap in BC.batches(r, content, n):
        assert _ans(lambda: f.ranges(reqs, mx, cap)) == BR.expected_ranges(stores, reqs, mx, cap), (tag, len(reqs), mx)
    return content


def test_savepoint_rollback_compact(khst, oracle):
    """Under a savepoint a batch reads the commits since; after rollback the version before; a
    compacted forest reads the same."""
    r = random.Random(71)
    f, o = _grown(oracle, r)
    before = _stores(o)
    c0 = _check(f, before, r, 20, "open")
    f.savepoint()
    ids = list(o)
    ups = [(t, C._rk(r), C.storage_value(r)) for t in ids[:4] for _ in range(8)]
    dels = [(ids[0], c0[ids[0]][0][0]), (ids[5], c0[ids[5]][-1][0])]
    f.commit(ups, dels)
    for t, k, v in ups:
        o[t].put(k, v)
    for t, k in dels:
        o[t].remove(k)
    c1 = _check(f, _stores(o), r, 20, "savepoint")
    assert c1 != c0
    f.rollback()
    _check(f, before, r, 20, "rollback")
    f.compact()
    _check(f, before, r, 20, "compact")
    f.close()


def test_single_trie_handle_copy_compact(khst, oracle):
    """Several ranges of the one trie of a ResidentTrie (`tries` is NULL), on the handle, its copy
    and the compacted copy."""
    from khipu_amd.device import Ctx, ResidentTrie
    r = random.Random(72)
    ks = sorted(C._rk(r) for _ in range(300))
    vs = [C.account_value(r) if i % 3 else C.storage_value(r) for i in range(len(ks))]
    o = oracle.Trie()
    for k, v in zip(ks, vs):
        o.put(k, v)
    stores = {0: (o.reachable(), o.root_hash())}
    t = ResidentTrie(Ctx(0), ks, vs, emit=False)
    c = t.copy()
    dels = ks[40:90]
    t.commit([], dels)
    c.compact()
    reqs = [(None, ks[9]), (ks[5], ks[30]), (ks[200], None), (None, None), (ks[7], ks[6]), (RC._step(ks[299], 1), None)]
    for mx in (1, 10, 11, 37, 136, 137, 435, 436, 1000):
        want = BR.expected_ranges(stores, [(0, a, b) for a, b in reqs], mx)
        assert _ans(lambda: c.ranges(reqs, mx)) == want, mx
    for k in dels:
        o.remove(k)
    stores = {0: (o.reachable(), o.root_hash())}
    for mx in (1, 10, 100, 1000):
        assert _ans(lambda: t.ranges(reqs, mx)) == BR.expected_ranges(stores, [(0, a, b) for a, b in reqs], mx), mx
    assert t.ranges([(None, None)] * 3, 1000)[0] == [t.range(max_entries=1000)[:2]] * 3
    e = ResidentTrie(Ctx(0), [], [], emit=False)
    assert e.ranges([(None, None), (ks[1], None)]) == ([([], []), ([], [])], 2, None)
    for h in (t, c, e):
        h.close()


def test_single_and_batched_calls_report_the_same_rounds(khst, oracle):
    """khst_range_rounds after a single call and after the one-request batch of it (the two share
    the round loop that counts): none on an empty trie, one on a one-key trie (the root item is a
    leaf: the first round closes the walk), and equal on the 2,000-entry trie, with equal entries."""
    from khipu_amd._lib import lib
    from khipu_amd.device import Ctx, ResidentTrie
    rounds = lib().khst_range_rounds
    rounds.restype = ctypes.c_uint32
    r = random.Random(73)
    key, val = C._rk(r), C.account_value(r)
    for t, want, entries in ((ResidentTrie(Ctx(0), [], [], emit=False), 0, ([], [])),
                             (ResidentTrie(Ctx(0), [key], [val], emit=False), 1, ([key], [val]))):
        assert t.range()[:2] == entries and rounds() == want
        assert t.ranges([(None, None)]) == ([entries], 1, None) and rounds() == want
        t.close()
    tries, content, _, _ = _state(oracle, "big")
    ks = [k for k, _ in content[5]]
    assert len(ks) == 2000
    f = _load(tries)
    for o, l, mx in ((None, None, 3000), (None, None, 700), (ks[300], ks[1500], 500), (ks[1999], None, 10)):
        keys, vals, more, nxt = f.range(5, o, l, mx, BC.BIG)
        single = rounds()
        assert f.ranges([(5, o, l)], mx, BC.BIG) == ([(keys, vals)], 0 if more else 1, nxt), (o, l, mx)
        assert rounds() == single and 0 < single <= 66 and keys, (o, l, mx)
    f.close()


def test_partial_forest(khst, oracle):
    """A partial forest refuses with the hash AND the request the reference's walk over the held
    nodes names, answers the batches that end before a missing subtree, and a fetch loop from
    root-only loads ends at the reference's answer."""
    from khipu_amd import _lib
    tries, content, _, _ = _state(oracle, "forest60")
    r = random.Random(73)
    ids = [t for t in tries if len(content[t]) >= 10][:8]
    full = {t: tries[t] for t in ids}
    wit = {}
    for t in ids:
        nodes, root = tries[t]
        w = {root: nodes[root]}
        for k, _ in r.sample(content[t], 2):
            w.update({P.kec(e): e for e in P.expected_proof(nodes, root, k)[0]})
        wit[t] = (w, root)
    f = _load(wit, partial=True)
    assert f.stubs > 0
    seen = set()
    for reqs, mx, cap in BC.batches(r, {t: content[t] for t in ids}, 60):
        want = BR.expected_ranges(wit, reqs, mx, cap)
        assert _ans(lambda: f.ranges(reqs, mx, cap)) == want, (len(reqs), mx)
        seen.add(want[0])
        if want[0] == "missing":
            assert want[1] in tries[reqs[want[2]][0]][0]  # the request's trie holds that node
    assert seen >= {"pages", "missing"}
    f.close()
    # the fetch loop: root nodes only, every refusal answered from the store of the request's trie
    f = _load({t: ({root: nodes[root]}, root) for t, (nodes, root) in full.items()}, partial=True)
    reqs = [(t, content[t][2][0], None) for t in ids] + [(ids[0], None, content[ids[0]][4][0])]
    fetched = 0
    while True:
        try:
            got = f.ranges(reqs, 50)
            break
        except _lib.MPTNodeMissingException as e:
            store = tries[reqs[e.request][0]][0]
            assert e.missing in store
            assert f.fill({e.missing: store[e.missing]}) >= 1
            fetched += 1
    assert fetched >= 1 and ("pages",) + got == BR.expected_ranges(full, reqs, 50)
    f.close()


def test_device_buffers(khst, oracle):
    """kh_dev_trie_ranges: requests and answer in device buffers, equal to the host form."""
    import torch
    from khipu_amd import _lib
    tries, content, _, _ = _state(oracle, "forest60")
    f = _load(tries)
    ids = [t for t in tries if len(content[t]) >= 3][:9]
    reqs = [(t, content[t][0][0] if i % 3 == 1 else None, content[t][-1][0] if i % 3 == 2 else None)
            for i, t in enumerate(ids)] + [(BC.UNHELD, None, None)]
    nq, cap = len(reqs), 1 << 16
    mx = sum(len(ks) for ks, _ in f.ranges(reqs, 1 << 12, cap)[0]) // 2
    want = f.ranges(reqs, mx, cap)
    assert mx >= 13 and want[1] < nq - 1  # (cut: next is read too)

    def dev(a):
        return torch.from_numpy(a).to("cuda:0")
    dt = dev(np.asarray([t for t, _, _ in reqs], np.uint32).view(np.int32))
    dor = dev(np.frombuffer(b"".join(o or RC.ZERO for _, o, _ in reqs), np.uint8).copy())
    dli = dev(np.frombuffer(b"".join(l or RC.FF for _, _, l in reqs), np.uint8).copy())
    dk = torch.zeros(32 * mx, dtype=torch.uint8, device="cuda:0")
    dv = torch.zeros(cap, dtype=torch.uint8, device="cuda:0")
    do = torch.zeros(mx + 1, dtype=torch.int64, device="cuda:0")
    de = torch.zeros(nq + 1, dtype=torch.int64, device="cuda:0")
    ne, vb, nd = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    nxt = np.zeros(32, np.uint8)
    f.ctx._sync()
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rc = _lib.lib().kh_dev_trie_ranges(f.h, p(dt), p(dor), p(dli), nq, mx, p(dk), p(dv), cap, p(do), p(de),
                                       ctypes.byref(ne), ctypes.byref(vb), ctypes.byref(nd), nxt.ctypes.data, None)
    assert rc == _lib.KH_OK and ne.value == mx
    off, eo = do.cpu().numpy(), de.cpu().numpy()
    kb, vbuf = dk.cpu().numpy().tobytes(), dv.cpu().numpy().tobytes()
    assert int(off[mx]) == vb.value and int(eo[nq]) == mx
    pages = [([kb[32 * i:32 * i + 32] for i in range(int(eo[q]), int(eo[q + 1]))],
              [vbuf[int(off[i]):int(off[i + 1])] for i in range(int(eo[q]), int(eo[q + 1]))]) for q in range(nq)]
    assert (pages, int(nd.value), nxt.tobytes()) == want
    f.close()


def test_refusals_leave_the_outputs_untouched(khst, oracle):
    from khipu_amd import _lib
    from khipu_amd.device import Ctx, ResidentTrie
    tries, content, _, _ = _state(oracle, "big")
    f = _load(tries)
    t1 = ResidentTrie(Ctx(0), [b"\x01" * 32], [b"\x02"], emit=False)
    L = _lib.lib()
    nq = 3
    tb = np.asarray([5, 6, 9], np.uint32)
    bufs = {n: np.full(s, 0xAB, np.uint8) for n, s in (("keys", 32 * 8), ("vals", 256), ("voff", 8 * 9),
                                                        ("eoff", 8 * (nq + 1)), ("next", 32), ("miss", 32))}
    sc = [ctypes.c_uint64(0xABABABAB) for _ in range(3)]

    def call(h=None, tries=tb, nq=nq, mx=8, drop=()):
        a = {n: (None if n in drop else b.ctypes.data) for n, b in bufs.items()}
        s = [None if f"s{i}" in drop else ctypes.byref(sc[i]) for i in range(3)]
        return L.kh_trie_ranges_host(f.h if h is None else h, tries.ctypes.data if tries is not None else None, None,
                                     None, nq, mx, a["keys"], a["vals"], 256, a["voff"], a["eoff"], s[0], s[1], s[2],
                                     a["next"], a["miss"])

    bad = [dict(nq=0), dict(mx=0), dict(mx=(1 << 31) - nq), dict(mx=1 << 31), dict(tries=None)]
    bad += [dict(drop=(n,)) for n in ("keys", "voff", "eoff", "next", "s0", "s1", "s2")]
    for kw in bad:
        assert call(**kw) == _lib.KH_EINVAL, kw
        assert all((b == 0xAB).all() for b in bufs.values()) and all(s.value == 0xABABABAB for s in sc), kw
    assert call(h=t1.h, tries=None, mx=8) == _lib.KH_OK and sc[0].value == 3  # (a single trie: tries may be NULL)
    # KH_ENOSPC writes *val_bytes alone
    for b in bufs.values():
        b[:] = 0xAB
    sc[0].value = sc[2].value = 0xABABABAB
    first = len(content[5][0][1])
    assert L.kh_trie_ranges_host(f.h, tb.ctypes.data, None, None, nq, 8, bufs["keys"].ctypes.data, bufs["vals"].ctypes.data,
                                 first - 1, bufs["voff"].ctypes.data, bufs["eoff"].ctypes.data, ctypes.byref(sc[0]),
                                 ctypes.byref(sc[1]), ctypes.byref(sc[2]), bufs["next"].ctypes.data,
                                 bufs["miss"].ctypes.data) == _lib.KH_ENOSPC
    assert sc[1].value == first and sc[0].value == sc[2].value == 0xABABABAB
    assert all((b == 0xAB).all() for b in bufs.values())
    with pytest.raises(_lib.MPTException):
        f.ranges([(5, b"\x00" * 31, None)])
    with pytest.raises(_lib.MPTException):
        f.ranges([])
    f.close()
    t1.close()


def test_ranges_proof_into_verify_ranges(khst, oracle):
    """Closing the loop: ranges_proof over a mixed batch -- whole tries, a non-zero origin, a limit
    and a cut tail -- goes into verify_ranges in ONE call: every answered request is KH_RANGE_OK
    with the reference's `more`; one changed value turns that request alone BAD_ROOT."""
    from khipu_amd import _lib
    from khipu_amd.device import verify_ranges
    tries, content, _, _ = _state(oracle, "forest60")
    f = _load(tries, hashed=True)
    big = [t for t in tries if len(content[t]) >= 30]
    small = [t for t in tries if 3 <= len(content[t]) <= 10]
    a, b, c = big[0], big[1], big[2]
    reqs = [(small[0], None, None), (a, content[a][7][0], None), (small[1], None, None),
            (b, None, content[b][11][0]), (BC.EMPTY_IDS[0], None, None), (small[2], RC._step(content[small[2]][1][0], 1), None),
            (c, None, None), (small[3], None, None)]
    mx = sum(len(BR.expected_ranges(tries, [q], 1000)[1][0][0]) for q in reqs[:6]) + 17
    pages, n_done, nxt, table, proved = f.ranges_proof(reqs, mx)
    assert ("pages", pages, n_done, nxt) == BR.expected_ranges(tries, reqs, mx)
    assert n_done == 6 and len(pages[6][0]) == 17 and proved == [0, 1, 0, 1, 0, 1, 1, 0]
    m = n_done + 1  # the answered requests and the cut one
    roots = [tries[t][1] for t, _, _ in reqs[:m]]
    origins = [o for _, o, _ in reqs[:m]]
    got = verify_ranges(roots, origins, pages[:m], table, proved[:m])
    for q, (st, more, miss) in enumerate(got):
        last = pages[q][0][-1] if pages[q][0] else None
        want_more = bool(proved[q]) and any(k > last for k, _ in content[reqs[q][0]])
        assert (st, more, miss) == (_lib.KH_RANGE_OK, want_more, None), q
    assert [g[1] for g in got] == [False, False, False, True, False, False, True]
    for q in (1, 3, 6, 0):
        bad = [(list(ks), list(vs)) for ks, vs in pages[:m]]
        bad[q][1][len(bad[q][1]) // 2] = b"\x7f" + bad[q][1][len(bad[q][1]) // 2]
        st = [g[0] for g in verify_ranges(roots, origins, bad, table, proved[:m])]
        assert st == [_lib.KH_RANGE_BAD_ROOT if i == q else _lib.KH_RANGE_OK for i in range(m)], q
    # the single-trie form: several proved ranges of one trie in one table
    from khipu_amd.device import Ctx, ResidentTrie
    ks = [k for k, _ in content[a]]
    t = ResidentTrie(Ctx(0), ks, [v for _, v in content[a]], emit=False)
    assert t.get_root() == tries[a][1]
    one = [(None, ks[4]), (ks[9], ks[20]), (ks[25], None)]
    pages, n_done, nxt, table, proved = t.ranges_proof(one, 1000)
    assert n_done == 3 and nxt is None and proved == [1, 1, 1]
    got = verify_ranges([tries[a][1]] * 3, [o for o, _ in one], pages, table, proved)
    assert [g[:2] for g in got] == [(_lib.KH_RANGE_OK, True), (_lib.KH_RANGE_OK, True), (_lib.KH_RANGE_OK, False)]
    t.close()
    f.close()


def test_ranges_through_the_jni_shim(khst, oracle, tmp_path):
    """ranges through the in-process JNIEnv of tests/jni_stub: batches of ranges of one trie followed
    to their end by n_done / next, with a value array that starts empty, so the grow path runs."""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    stub = os.path.join(ROOT, "tests", "jni_stub")
    exe = tmp_path / "jni_ranges_driver"
    rc = subprocess.run([cc, "-std=gnu99", "-O1", "-Wall", "-Werror", "-I", stub, "-I", os.path.join(ROOT, "include"),
                         "-o", str(exe), os.path.join(stub, "jni_ranges_driver.c"), os.path.join(stub, "fake_env.c"),
                         os.path.join(ROOT, "jni", "khst_jni.c"), "-L", os.path.join(ROOT, "khipu_amd"), "-lkhst",
                         "-Wl,-rpath," + os.path.join(ROOT, "khipu_amd"), "-Wl,-rpath-link,/opt/rocm/lib"],
                        capture_output=True, text=True)
    assert rc.returncode == 0, rc.stderr
    rnd = random.Random(809)
    keys = [C._rk(rnd) for _ in range(400)]
    vals = [C.account_value(rnd) if i % 3 else C.storage_value(rnd) for i in range(len(keys))]
    voff = np.zeros(len(vals) + 1, np.uint64)
    voff[1:] = np.cumsum([len(v) for v in vals])
    srt = sorted(keys)
    batches = [([(RC.ZERO, RC.FF)], 64),
               ([(srt[100], srt[180]), (RC.FF, RC.ZERO), (RC._step(srt[10], 1), srt[12]), (srt[399], RC.FF)], 7),
               ([(srt[i], srt[i + 9]) for i in range(0, 170, 10)], 1),
               ([(RC.ZERO, srt[50]), (srt[390], RC.FF)], 1000)]
    p = tmp_path / "in.bin"
    with open(p, "wb") as fo:
        fo.write(np.uint32(32).tobytes() + np.uint64(len(keys)).tobytes())
        fo.write(b"".join(keys) + voff.tobytes() + b"".join(vals))
        fo.write(np.uint64(len(batches)).tobytes())
        for reqs, mx in batches:
            fo.write(np.uint64(len(reqs)).tobytes() + np.uint64(mx).tobytes() + b"".join(a + b for a, b in reqs))
    rc = subprocess.run([str(exe), str(p)], capture_output=True, text=True, timeout=120)
    assert rc.returncode == 0, rc.stderr
    lines = [ln.split() for ln in rc.stdout.split("\n")[:-1]]
    assert lines[-1] == ["E", "0"], lines[-1]
    have = sorted(zip(keys, vals))
    for j, (reqs, mx) in enumerate(batches):
        total = 0
        for q, (a, b) in enumerate(reqs):
            got = [(bytes.fromhex(x[3]), b"" if x[4] == "-" else bytes.fromhex(x[4])) for x in lines
                   if x[0] == "K" and x[1] == str(j) and x[2] == str(q)]
            want = [(k, v) for k, v in have if a <= k <= b]
            assert got == want, (j, q)
            total += len(want)
        _, n, calls, grows = [x for x in lines if x[0] == "Q" and x[1] == str(j)][0][1:]
        assert int(n) == total and int(calls) >= max(1, -(-total // mx)) and int(grows) >= 1
