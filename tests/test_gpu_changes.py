"""GPU: the keys changed since a savepoint, read from the journal (kh_trie_changes_since_host), held to
tests/changes_ref.expected over the Python dicts each test maintains -- and, where value-only
branches are involved, to trie_diff(copy taken at the savepoint, current), which test_gpu_diff.py
holds to its own reference."""
import random

import numpy as np
import pytest

from tests import cases as C
from tests import changes_ref as CR
from tests import proof_cases

pytestmark = pytest.mark.gpu
BIG = 1 << 30


def _ans(h, level=0, reverse=False, start=None, max_entries=1024, val_cap=BIG):
    """One call's answer in the form of changes_ref.expected (a single trie under trie id 0)."""
    from khipu_amd import _lib
    from khipu_amd.device import ResidentForest
    forest = isinstance(h, ResidentForest)
    try:
        ents, more, nxt, total = h.changes_since(level, reverse, start if forest or start is None else start[1],
                                                 max_entries, val_cap)
    except _lib.KhError as e:
        assert e.code == _lib.KH_ENOSPC
        return ("nospc", e.val_bytes, e.n_total)
    if not forest:
        ents, nxt = [(0,) + e for e in ents], (0, nxt) if more else None
    return ("page", ents, more, nxt, total)


def _apply(d, ups, dels, t=0):
    """the commit's upserts then deletes on a model dict"""
    for k, v in ups:
        d[(t, k)] = (v, False)
    for k in dels:
        d.pop((t, k), None)


def _accounts(r, n):
    return {C._rk(r): C.account_value(r) for _ in range(n)}


def _model(kv, t=0):
    return {(t, k): (v, False) for k, v in kv.items()}


def _block(r, kv, new=60, change=60, same=30, gone=40, absent=10):
    """A commit with every kind of op over the trie's keys kv."""
    ks = r.sample(sorted(kv), change + same + gone)
    ups = [(C._rk(r), C.account_value(r)) for _ in range(new)]
    ups += [(k, C.account_value(r)) for k in ks[:change]] + [(k, kv[k]) for k in ks[change:change + same]]
    dels = ks[change + same:] + [C._rk(r) for _ in range(absent)]
    r.shuffle(ups)
    return ups, dels


@pytest.fixture(scope="module")
def one_commit(khst):
    """A trie of 600 accounts, a savepoint, one commit: (trie, before, after), shared and left unchanged."""
    from khipu_amd.device import Ctx, ResidentTrie
    r = random.Random(101)
    kv = _accounts(r, 600)
    t = ResidentTrie(Ctx(0), list(kv), list(kv.values()), emit=True)
    before = _model(kv)
    t.savepoint()
    ups, dels = _block(r, kv)
    t.commit(ups, dels)
    after = dict(before)
    _apply(after, ups, dels)
    yield t, before, after
    t.close()


def test_one_commit_matches_the_model_and_reads_only(one_commit):
    t, before, after = one_commit
    root, nodes, export = t.get_root(), t.nodes(), list(t.export_nodes())
    want = CR.expected(before, after)
    assert {e[2] for e in want[1]} == {1, 2, 3} and want[4] == 160
    assert _ans(t) == want
    assert _ans(t, reverse=True) == CR.expected(before, after, True)
    assert _ans(t, level=1) == want
    ups, dels = t.changes_since_all()
    assert ([(0,) + u for u in ups], [(0, k) for k in dels]) == CR.ops(want[1])
    # read-only: the root, the last commit's write-back set and the export are as before
    assert (t.get_root(), t.nodes(), list(t.export_nodes())) == (root, nodes, export)
    assert t.savepoint_depth() == 1


def test_reverse_answer_undoes_the_commit(khst):
    """The reverse ops committed on the handle give the savepoint's root -- and then nothing differs:
    every key was deleted and put back, or put and deleted, across commits."""
    from khipu_amd.device import Ctx, ResidentTrie
    r = random.Random(102)
    kv = _accounts(r, 300)
    t = ResidentTrie(Ctx(0), list(kv), list(kv.values()), emit=False)
    root0 = t.get_root()
    t.savepoint()
    t.commit(*_block(r, kv, 40, 40, 10, 30, 5))
    ups, dels = t.changes_since_all(reverse=True)
    assert len(ups) == 70 and len(dels) == 40
    assert t.commit(ups, dels) == root0
    assert t.changes_since() == ([], False, None, 0)
    assert t.changes_since(reverse=True) == ([], False, None, 0)
    t.close()


def test_three_commits_under_one_savepoint(khst):
    from khipu_amd.device import Ctx, ResidentTrie
    r = random.Random(103)
    kv = _accounts(r, 400)
    # two keys alone under a 10-nibble prefix: deleting one collapses their branch and re-anchors the other
    ka = bytearray(C._rk(r))
    kb = bytearray(ka)
    kb[5] ^= 0x80
    ka, kb = bytes(ka), bytes(kb)
    kv[ka], kv[kb] = b"leaves", b"stays, re-anchored"
    t = ResidentTrie(Ctx(0), list(kv), list(kv.values()), emit=False)
    before = _model(kv)
    after = dict(before)
    keys = sorted(k for k in kv if k not in (ka, kb))
    p, q, c2 = C._rk(r), keys[0], keys[1]
    t.savepoint()
    commits = [([(p, b"put"), (c2, b"first change")], [q, ka]),
               ([(p, b"changed"), (q, kv[q]), (c2, b"second change")], []),
               ([(kb, b"changed after the re-anchor")], [p])]
    for i, (ups, dels) in enumerate(commits):
        t.commit(ups, dels)
        _apply(after, ups, dels)
        assert _ans(t) == CR.expected(before, after), i
        if i == 0:  # the re-anchored sibling is not a difference
            assert [e[1] for e in _ans(t)[1]] == sorted([p, c2, q, ka])
    got = {k: (kind, v) for _, k, kind, v in _ans(t)[1]}
    assert got == {c2: (3, b"second change"), ka: (1, b""), kb: (3, b"changed after the re-anchor")}
    assert _ans(t, reverse=True) == CR.expected(before, after, True)
    t.close()


def test_nested_savepoints(khst):
    from khipu_amd.device import Ctx, ResidentTrie
    r = random.Random(104)
    kv = _accounts(r, 300)
    t = ResidentTrie(Ctx(0), list(kv), list(kv.values()), emit=True)
    v0 = _model(kv)
    t.savepoint()
    b1 = _block(r, kv, 20, 20, 5, 10, 2)
    t.commit(*b1)
    v1 = dict(v0)
    _apply(v1, *b1)
    t.savepoint()
    kv1 = {k: v for (_, k), (v, _) in v1.items()}
    b2 = _block(r, kv1, 20, 20, 5, 10, 2)
    t.commit(*b2)
    v2 = dict(v1)
    _apply(v2, *b2)
    assert _ans(t, level=0) == _ans(t, level=2) == CR.expected(v1, v2)
    assert _ans(t, level=1) == CR.expected(v0, v2)
    assert _ans(t, level=0) != _ans(t, level=1)
    t.rollback()  # the inner one: only the outer commit is left
    assert t.savepoint_depth() == 1 and _ans(t, level=1) == _ans(t, level=0) == CR.expected(v0, v1)
    t.savepoint()
    t.commit(*b2)
    t.release()  # the inner one is kept: level 0 is the old level 1
    assert t.savepoint_depth() == 1 and _ans(t, level=0) == CR.expected(v0, v2)
    t.rollback()
    t.savepoint()
    assert t.changes_since() == ([], False, None, 0) and t.changes_since(level=1) == ([], False, None, 0)
    t.close()


def test_forest_one_call_covers_every_trie(khst, oracle):
    from khipu_amd.device import Ctx, ResidentForest
    r = random.Random(105)
    ctx = Ctx(0)
    f = ResidentForest(ctx)
    shared = C._rk(r)
    before = {}
    for t in range(39):
        for k in [C._rk(r) for _ in range(8)] + ([shared] if t in (1, 2) else []):
            before[(t, k)] = (C.account_value(r), False)
    items = [(t, k, v) for (t, k), (v, _) in before.items()]
    f.commit(items[:160])
    f.commit(items[160:])
    f.savepoint()
    cp = f.copy()
    after = dict(before)
    ups = [(39, C._rk(r), b"a new trie") for _ in range(5)] + [(1, shared, b"one"), (2, shared, b"two")]
    dels = [tk for tk in before if tk[0] == 5]  # trie 5 is emptied
    for t in range(39):
        if t != 5:
            ups.append((t, C._rk(r), C.account_value(r)))
            if t % 3 == 0:
                ups.append((t,) + r.choice([(k, b"changed") for (u, k) in before if u == t]))
    assert len({t for t, _, _ in ups} | {5}) == 40 and len(ups) + len(dels) <= 200
    f.commit(ups, dels)
    for t, k, v in ups:
        after[(t, k)] = (v, False)
    for tk in dels:
        del after[tk]
    # one more trie loaded from a node store under the savepoint: every key of it is kind 2
    kv = _accounts(r, 30)
    o = oracle.Trie()
    for k, v in kv.items():
        o.put(k, v)
    f.load_nodes({700: o.root_hash()}, o.reachable())
    after.update(_model(kv, 700))
    want = CR.expected(before, after)
    got = _ans(f)
    assert got == want
    assert [(e[0], e[1]) for e in got[1]] == sorted((e[0], e[1]) for e in got[1])
    assert {e[2] for e in got[1] if e[0] == 700} == {2} and {e[2] for e in got[1] if e[0] == 5} == {1}
    assert _ans(f, reverse=True) == CR.expected(before, after, True)
    # pages chained by the (trie, key) pair, a start inside a trie, a start at a trie the forest lacks
    assert _ans(f, start=(2, shared), max_entries=3) == CR.expected(before, after, False, (2, shared), 3, BIG)
    assert _ans(f, start=(40, bytes(32))) == CR.expected(before, after, False, (40, bytes(32)))
    out, start = [], None
    while True:
        g = _ans(f, start=start, max_entries=37)
        out += g[1]
        if not g[2]:
            break
        start = g[3]
    assert out == want[1]
    # the existing batched diff against the copy taken at the savepoint says the same
    ups_all, dels_all = f.changes_since_all()
    by_trie = {}
    for t, k, v in ups_all:
        by_trie.setdefault(t, ([], []))[0].append((k, v))
    for t, k in dels_all:
        by_trie.setdefault(t, ([], []))[1].append(k)
    assert by_trie == cp.changes_all(f)
    for h in (cp, f):
        h.close()


def test_block_commit_host_under_caller_savepoints(khst, oracle):
    from khipu_amd import _lib, codec
    from khipu_amd.device import block_commit_host
    from tests.test_gpu_versioned import _host_pair
    keys, vals, state, forest = _host_pair(khst, 200, 31)
    slot = lambda i: bytes(31) + bytes([i])  # noqa: E731
    u8 = lambda b: np.frombuffer(b + bytes(8), np.uint8).copy()  # noqa: E731

    def block(s_ups, a_ups, a_dels):
        """s_ups [(trie, slot key, value)], a_ups [(key, body, trie or KH_NO_TRIE)], a_dels [key]"""
        sv, av = [v for _, _, v in s_ups], [b for _, b, _ in a_ups]
        return block_commit_host(
            state, forest, np.array([t for t, _, _ in s_ups], np.uint32), u8(b"".join(k for _, k, _ in s_ups)),
            u8(b"".join(sv)), np.concatenate([[0], np.cumsum([len(v) for v in sv])]).astype(np.uint64), None, None,
            u8(b"".join(k for k, _, _ in a_ups)), u8(b"".join(av)),
            np.concatenate([[0], np.cumsum([len(b) for b in av])]).astype(np.uint64),
            np.array([t for _, _, t in a_ups], np.uint32), u8(b"".join(a_dels)) if a_dels else None)

    def patched(body, trie, slots):
        o = oracle.Trie()
        for (t, k), (v, _) in slots.items():
            if t == trie:
                o.put(k, v)
        b = bytearray(body)
        b[len(b) - 65:len(b) - 33] = o.root_hash()
        return bytes(b)

    s_after = {}
    b1 = [(0, slot(1), b"\x05"), (0, slot(2), b"\x06"), (7, slot(1), b"\x07")]
    block(b1, [(keys[0], codec.account_rlp(1, 5), 0), (keys[1], codec.account_rlp(1, 6), 7)], [])
    for t, k, v in b1:
        s_after[(t, oracle.kec256(k))] = (v, False)
    a_before = _model(dict(zip(keys, vals)))
    a_before[(0, keys[0])] = (patched(codec.account_rlp(1, 5), 0, s_after), False)
    a_before[(0, keys[1])] = (patched(codec.account_rlp(1, 6), 7, s_after), False)
    s_before = dict(s_after)
    state.savepoint()
    forest.savepoint()
    b2 = [(0, slot(1), b"\x15"), (0, slot(3), b"\x16"), (9, slot(1), b"\x17"), (7, slot(1), b"\x07")]
    bodies = [codec.account_rlp(2, 50), codec.account_rlp(3, 60), codec.account_rlp(4, 70)]
    block(b2, [(keys[0], bodies[0], 0), (keys[2], bodies[1], 9), (keys[3], bodies[2], _lib.KH_NO_TRIE)], [keys[4]])
    for t, k, v in b2:
        s_after[(t, oracle.kec256(k))] = (v, False)
    a_after = dict(a_before)
    a_after[(0, keys[0])] = (patched(bodies[0], 0, s_after), False)
    a_after[(0, keys[2])] = (patched(bodies[1], 9, s_after), False)
    a_after[(0, keys[3])] = (bodies[2], False)
    del a_after[(0, keys[4])]
    assert state.savepoint_depth() == 1 and forest.savepoint_depth() == 1  # (the call's own are gone)
    assert _ans(forest) == CR.expected(s_before, s_after)
    assert sorted((e[0], e[2]) for e in _ans(forest)[1]) == [(0, 2), (0, 3), (9, 2)]  # (trie 7's re-put is none)
    got = _ans(state)
    assert got == CR.expected(a_before, a_after)
    assert {e[1]: e[3] for e in got[1]}[keys[2]] != bodies[1]  # the body carries the patched storage root
    assert _ans(state, reverse=True) == CR.expected(a_before, a_after, True)
    state.close()
    forest.close()


def test_value_only_branch_is_a_difference_of_equal_values(khst):
    from khipu_amd.device import Ctx, ResidentTrie
    ks, vs, blocks, (k1, _, _) = proof_cases.vb_case(False)
    t = ResidentTrie(Ctx(0), ks, vs, emit=False)
    t.savepoint()
    cp = t.copy()
    t.commit([(k1, vs[ks.index(k1)])], [])  # the value it had: the leaf still becomes a value-only branch
    assert t.changes_since() == ([(k1, 3, vs[ks.index(k1)])], False, None, 1)
    assert cp.diff(t, max_entries=1000) == t.changes_since(max_entries=1000)[:3]
    for ups, dels in blocks[:4]:
        t.commit(ups, dels)
        assert cp.diff(t, max_entries=1000) == t.changes_since(max_entries=1000)[:3]
        assert t.diff(cp, max_entries=1000) == t.changes_since(reverse=True, max_entries=1000)[:3]
    for h in (cp, t):
        h.close()


def test_partial_handle_answers_exactly(khst):
    """Opened from the batch's commit witness: the answer is the full handle's, no copy of the
    partial handle is made and no node is reported missing."""
    from khipu_amd.device import Ctx, ResidentTrie
    r = random.Random(107)
    kv = _accounts(r, 800)
    ctx = Ctx(0)
    t = ResidentTrie(ctx, list(kv), list(kv.values()), emit=False)
    ups, dels = _block(r, kv, 30, 30, 10, 25, 5)
    witness, _ = t.commit_witness(ups, dels)
    p = ResidentTrie.from_witness(ctx, t.get_root(), witness, emit=False)
    assert p.stubs > 0
    after = _model(kv)
    _apply(after, ups, dels)
    for h in (t, p):
        h.savepoint()
        h.commit(ups, dels)
    assert p.get_root() == t.get_root() and p.stubs > 0
    assert _ans(p) == _ans(t) == CR.expected(_model(kv), after)
    assert _ans(p, reverse=True, max_entries=7) == CR.expected(_model(kv), after, True, None, 7, BIG)
    for h in (t, p):
        h.close()


def test_paging_and_caps(one_commit):
    t, before, after = one_commit
    full = CR.differences(before, after)
    out, start = [], None
    for _ in range(len(full) + 1):
        g = _ans(t, start=start, max_entries=1)
        assert g == CR.expected(before, after, False, start, 1, BIG)
        out += g[1]
        if not g[2]:
            break
        start = g[3]
    assert out == full
    # val_cap cuts mid-answer; a first value that does not fit is KH_ENOSPC with its size and n_total
    i = next(i for i, d in enumerate(full) if d[3])
    start, first = (0, full[i][1]), len(full[i][3])
    for cap in (first, first + 1, 5 * first, first - 1, 0):
        assert _ans(t, start=start, val_cap=cap) == CR.expected(before, after, False, start, 1024, cap), cap
    assert _ans(t, start=start, val_cap=first - 1) == ("nospc", first, len(full) - i)
    assert len(_ans(t, start=start, val_cap=5 * first)[1]) < len(full) - i
    # a start that is no difference: between two, before the first, past the last
    k = full[4][1]
    between = k[:31] + bytes([k[31] ^ 1]) if k[31] & 1 == 0 else None
    for s in (between, bytes(32), b"\xff" * 32):
        if s is not None:
            assert _ans(t, start=(0, s)) == CR.expected(before, after, False, (0, s))
    assert _ans(t, start=(0, b"\xff" * 32))[1:] == ([], False, None, 0)


def test_device_buffers(one_commit):
    """kh_dev_trie_changes_since: trie ids, keys, kinds, values and offsets into device buffers, equal
    to the host form; a short page names the next pair."""
    import ctypes
    import torch
    from khipu_amd import _lib
    t, before, after = one_commit
    want = CR.expected(before, after, True, None, 100, 1 << 16)
    dt = torch.full((100,), 7, dtype=torch.int32, device="cuda:0")
    dk = torch.zeros(32 * 100, dtype=torch.uint8, device="cuda:0")
    dkind = torch.zeros(100, dtype=torch.uint8, device="cuda:0")
    dv = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda:0")
    do = torch.zeros(101, dtype=torch.int64, device="cuda:0")
    ne, vb, tot, more, nt = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_int(0), ctypes.c_uint32(9)
    nxt = np.zeros(32, np.uint8)
    t.ctx._sync()
    p = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    rc = _lib.lib().kh_dev_trie_changes_since(t.h, 0, _lib.KH_CHANGES_REVERSE, 0, None, 100, 1 << 16, p(dt), p(dk),
                                              p(dkind), p(dv), p(do), ctypes.byref(ne), ctypes.byref(vb),
                                              ctypes.byref(tot), ctypes.byref(more), ctypes.byref(nt), nxt.ctypes.data)
    assert rc == _lib.KH_OK
    k = int(ne.value)
    off = do.cpu().numpy()
    kb, kinds, vbuf, tr = dk.cpu().numpy().tobytes(), dkind.cpu().numpy(), dv.cpu().numpy().tobytes(), dt.cpu().numpy()
    assert int(off[k]) == vb.value
    got = [(int(tr[j]), kb[32 * j:32 * j + 32], int(kinds[j]), vbuf[int(off[j]):int(off[j + 1])]) for j in range(k)]
    assert ("page", got, bool(more.value), (int(nt.value), nxt.tobytes()), int(tot.value)) == want
    assert k == 100 and want[2] and list(tr[k:]) == []
    bad = ctypes.c_void_p(do.data_ptr() + 4)  # a misaligned voff is refused before any launch
    assert _lib.lib().kh_dev_trie_changes_since(t.h, 0, 0, 0, None, 100, 1 << 16, p(dt), p(dk), p(dkind), p(dv), bad,
                                                ctypes.byref(ne), ctypes.byref(vb), ctypes.byref(tot),
                                                ctypes.byref(more), ctypes.byref(nt), nxt.ctypes.data) == _lib.KH_EINVAL


def test_growth_under_the_savepoint(khst):
    """Twelve commits of 200 upserts onto 150 keys: the record array grows past its first capacity and the
    anchor map is rebuilt between the savepoint and the call; the answer is the model's."""
    from khipu_amd.device import Ctx, ResidentTrie
    r = random.Random(108)
    kv = _accounts(r, 150)
    t = ResidentTrie(Ctx(0), list(kv), list(kv.values()), emit=False)
    before = _model(kv)
    after = dict(before)
    u0 = t.usage()
    t.savepoint()
    for i in range(12):
        ups = [(C._rk(r), bytes([i + 1]) * 3) for _ in range(195)] + [(k, b"again") for k in r.sample(sorted(kv), 5)]
        t.commit(ups, [])
        _apply(after, ups, [])
    u1 = t.usage()
    assert u0["records"] < 4096 < u1["records"] and u1["map_slots"] > u0["map_slots"]
    assert _ans(t, max_entries=4000) == CR.expected(before, after, False, None, 4000, BIG)
    ups, dels = t.changes_since_all()  # (sized from n_total: more than one call's default)
    assert len(ups) == CR.expected(before, after, False, None, 4000, BIG)[4] and not dels
    t.close()


def test_hashed_keys_and_a_lazy_tail(khst, oracle):
    from khipu_amd.device import Ctx, ResidentTrie
    r = random.Random(109)
    addrs = [bytes(r.getrandbits(8) for _ in range(20)) for _ in range(300)]
    kv = {a: C.account_value(r) for a in addrs}
    # emit=False: the commit returns with its tail in flight; the call right after it settles it
    t = ResidentTrie(Ctx(0), addrs, list(kv.values()), hash_keys=True, emit=False)
    before = {(0, oracle.kec256(a)): (v, False) for a, v in kv.items()}
    t.savepoint()
    ups = [(a, b"changed") for a in addrs[:50]] + [(bytes(r.getrandbits(8) for _ in range(20)), b"new") for _ in range(50)]
    t.commit(ups, addrs[50:80])
    got = _ans(t)
    after = dict(before)
    _apply(after, [(oracle.kec256(a), v) for a, v in ups], [oracle.kec256(a) for a in addrs[50:80]])
    assert got == CR.expected(before, after) and got[4] == 130
    from khipu_amd.device import changes_counters
    assert changes_counters() == 1  # (hashes: the first word orders them)
    t.close()


def test_dense_keys_sort_on_all_four_words(khst):
    """Keys that share their first 8 bytes (and some their first 16 and 24): the order on the first
    word alone is flagged and the call sorts again on the whole key; hashed keys take one sort."""
    from khipu_amd.device import Ctx, ResidentTrie, changes_counters
    r = random.Random(111)
    ks = [bytes(8) + bytes([i % 3]) * 8 + bytes([i % 5]) * 8 + bytes(4) + i.to_bytes(4, "big") for i in range(400)]
    kv = {k: bytes([1 + i % 100]) for i, k in enumerate(ks)}
    t = ResidentTrie(Ctx(0), ks, list(kv.values()), emit=False)
    before = _model(kv)
    after = dict(before)
    t.savepoint()
    ups = [(k, b"changed") for k in r.sample(ks, 80)] + [(bytes(24) + bytes([9]) * 4 + i.to_bytes(4, "big"), b"new")
                                                        for i in range(40)]
    dels = r.sample(ks, 60)
    t.commit(ups, dels)
    _apply(after, ups, dels)
    assert _ans(t) == CR.expected(before, after)
    assert changes_counters() == 5
    assert _ans(t, reverse=True, max_entries=9) == CR.expected(before, after, True, None, 9, BIG)
    t.close()


def test_refusals_leave_the_handle_usable(khst):
    from khipu_amd import _lib
    from khipu_amd.device import Ctx, ResidentTrie
    r = random.Random(110)
    kv = _accounts(r, 200)
    t = ResidentTrie(Ctx(0), list(kv), list(kv.values()), emit=False)

    def refused(**kw):
        with pytest.raises(_lib.KhError) as e:
            t.changes_since(**kw)
        assert e.value.code == _lib.KH_EINVAL

    refused()  # no savepoint
    t.savepoint()
    k = sorted(kv)[0]
    t.commit([(k, b"v")], [])
    refused(level=2)
    refused(max_entries=0)
    refused(max_entries=1 << 31)
    o = np.zeros(256, np.uint8)
    n = np.zeros(8, np.uint64)
    import ctypes
    more, nt = ctypes.c_int(0), ctypes.c_uint32(0)
    args = (None, 4, 64, None, o.ctypes.data, o.ctypes.data, o.ctypes.data, n.ctypes.data, ctypes.byref(ctypes.c_uint64()),
            ctypes.byref(ctypes.c_uint64()), None, ctypes.byref(more), ctypes.byref(nt), o.ctypes.data)
    assert _lib.lib().kh_trie_changes_since_host(t.h, 0, 0x2, 0, *args) == _lib.KH_EINVAL  # an unknown flag
    assert _lib.lib().kh_trie_changes_since_host(None, 0, 0, 0, *args) == _lib.KH_EINVAL
    assert t.changes_since() == ([(k, 3, b"v")], False, None, 1)
    t.rollback()
    refused()
    assert t.get([k]) == [kv[k]]
    t.close()
