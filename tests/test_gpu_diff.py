"""GPU: two resident tries diffed in key order (kh_trie_diff_host / kh_dev_trie_diff), held to
tests/diff_ref.expected_diff over the oracle's nodes: kinds, pages, `more` and `next`, the fit to
val_cap, skipped subtrees (the round and visited-item counters), forests, hashed handles, versions,
partial handles and the refusals."""
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
from tests import proof_ref as P

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCEN = DC.scenarios()
BIG = 1 << 30
NO_VB = ("accounts", "storage", "to_empty", "from_empty", "single", "same_key_batch", "large_batch")


def _answer(call):
    """A diff call's answer in the form of diff_ref.expected_diff."""
    from khipu_amd import _lib
    try:
        ents, more, nxt = call()
    except _lib.MPTNodeMissingException as e:
        return ("missing", e.missing)
    except _lib.KhError as e:
        assert e.code == _lib.KH_ENOSPC
        return ("nospc", e.val_bytes)
    return ("page", ents, more, nxt)


def _paged(diff, chunk):
    out, origin = [], None
    while True:
        ents, more, nxt = diff(origin, chunk)
        assert len(ents) <= chunk
        out += ents
        if not more:
            return out
        origin = nxt


def _check_pair(r, diff, sa, sb, tag, nq=6, paged=True):
    """diff(origin, limit, max_entries, val_cap) of the device against the reference over the two
    stores: the whole answer, a sample of the constructed queries, and (paged) paging to the end at
    budgets 1, 7 and 1000."""
    full = [(t[1], t[2], t[3]) for t in DR.walk_diff(*sa, *sb)]
    assert _answer(lambda: diff(None, None, 1000, BIG)) == DR.expected_diff(*sa, *sb, None, None, 1000, BIG), tag
    qs = DC.queries(r, full)
    for o, l, mx, cap in r.sample(qs, min(nq, len(qs))):
        assert _answer(lambda: diff(o, l, mx, cap)) == DR.expected_diff(*sa, *sb, o, l, mx, cap), \
            (tag, o and o.hex(), l and l.hex(), mx, cap)
    for chunk in (1, 7, 1000) if paged else ():
        if len(full) > 100 * chunk:  # (a few hundred calls at the most)
            continue
        assert _paged(lambda o, c: diff(o, None, c, BIG), chunk) == full, (tag, chunk)
    return full


@pytest.fixture(scope="module")
def world(oracle):
    """Per scenario, the reference's states [(nodes, root)], computed once."""
    return {s[0]: DC.states(oracle, s) for s in SCEN}


@pytest.mark.parametrize("i", range(len(SCEN)), ids=[s[0] for s in SCEN])
def test_diff_between_versions(khst, world, i):
    """One handle follows the commits, copy() is taken at each state; every ordered pair of states at
    most 3 apart, as two handles and as two ids of one forest loaded from the states' nodes; and
    changes() committed on a copy of one state gives the other's root."""
    from khipu_amd.device import Ctx, ResidentForest, ResidentTrie
    name, ks, vs, batches = SCEN[i]
    st = world[name]
    ctx = Ctx(0)
    t = ResidentTrie(ctx, ks, vs, emit=False)
    copies = [t.copy()]
    for b, (ups, dels) in enumerate(batches):
        assert t.commit(ups, dels) == st[b + 1][1], (name, b)
        copies.append(t.copy())
    held = {j: s[1] for j, s in enumerate(st) if s[1] != P.EMPTY_ROOT}
    nodes = {}
    for s in st:
        nodes.update(s[0])
    f = ResidentForest.from_nodes(ctx, held, nodes) if held else ResidentForest(ctx)
    r = random.Random(i)
    kinds = set()
    for a, b in DC.pairs(len(st)):
        tag = (name, a, b)
        full = _check_pair(r, lambda o, l, mx, cap: copies[a].diff(copies[b], o, l, mx, cap), st[a], st[b], tag,
                           paged=abs(a - b) == 1)
        kinds |= {k for _, k, _ in full}
        assert _answer(lambda: f.diff(a, f, b, None, None, 1000, BIG)) == ("page", full[:1000], len(full) > 1000,
                                                                        full[1000][0] if len(full) > 1000 else None), tag
        if name in NO_VB and abs(a - b) == 1:
            ups, dels = copies[a].changes(copies[b], chunk=64)
            assert (ups, dels) == ([(k, v) for k, kind, v in full if kind != 1], [k for k, kind, _ in full if kind == 1])
            c = copies[a].copy()
            assert c.commit(ups, dels) == st[b][1], tag
            assert c.diff(copies[b]) == ([], False, None)
            assert f.changes(a, f, b) == (ups, dels)
            c.close()
    if name == "accounts":
        assert kinds == {1, 2, 3}
    if name == "vb_equal_value":  # a value-only branch against a leaf of equal value is a difference
        (k, kind, v), = [(t[1], t[2], t[3]) for t in DR.walk_diff(*st[0], *st[1])]
        assert kind == 3 and v == vs[ks.index(k)]
    for h in copies + [t, f]:
        h.close()


def test_diff_hashed_handle(khst, oracle):
    """KH_HASH_KEYS handles: the keys of the answer are the kec256 values."""
    from khipu_amd.device import Ctx, ResidentTrie
    r = random.Random(20)
    ks = [bytes(r.getrandbits(8) for _ in range(20)) for _ in range(300)]
    vs = [C.account_value(r) if i % 2 else C.storage_value(r) for i in range(len(ks))]
    o = oracle.Trie()
    for k, v in zip(ks, vs):
        o.put(oracle.kec256(k), v)
    sa = DC.snap(o)
    t = ResidentTrie(Ctx(0), ks, vs, hash_keys=True, emit=False)
    base = t.copy()
    ups, dels = [(k, C.account_value(r)) for k in ks[:20]] + [(b"new" + bytes([j]) * 17, b"\x05") for j in range(9)], ks[50:90]
    DC.fold(o, [(oracle.kec256(k), v) for k, v in ups], [oracle.kec256(k) for k in dels])
    assert t.commit(ups, dels) == o.root_hash()
    sb = DC.snap(o)
    full = _check_pair(r, lambda o_, l, mx, cap: base.diff(t, o_, l, mx, cap), sa, sb, "hashed")
    assert len(full) == 20 + 9 + 40
    assert base.changes(t) == ([(k, v) for k, kind, v in full if kind != 1], [k for k, kind, _ in full if kind == 1])
    for h in (t, base):
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


def test_diff_val_cap_and_nospc(khst, oracle):
    from khipu_amd.device import Ctx, ResidentTrie, _diff_changes
    ks, vs, sa, sb, ups, dels = _two(oracle, 300, 150, 31)
    ctx = Ctx(0)
    a = ResidentTrie(ctx, ks, vs, emit=False)
    b = a.copy()
    assert b.commit(ups, dels) == sb[1]
    full = DR.expected_diff(*sa, *sb, None, None, 64)
    origin = next(k for k, kind, v in full[1] if kind != 1)
    full = DR.expected_diff(*sa, *sb, origin, None, 64)
    total, first = sum(len(v) for _, _, v in full[1]), len(full[1][0][2])
    caps = (total, total - 1, first, first - 1, 0)
    got = [_answer(lambda: a.diff(b, origin, None, 64, cap)) for cap in caps]
    assert got == [DR.expected_diff(*sa, *sb, origin, None, 64, cap) for cap in caps]
    assert len(got[0][1]) == 64 and len(got[1][1]) < 64 and got[1][2] and len(got[2][1]) >= 1
    assert got[3] == got[4] == ("nospc", first)
    # changes() grows val_cap when a value does not fit the first page
    want = [(t[1], t[2], t[3]) for t in DR.walk_diff(*sa, *sb)]
    u, d = _diff_changes(a.h, None, b.h, None, 50, val_cap=1)
    assert (u, d) == ([(k, v) for k, kind, v in want if kind != 1], [k for k, kind, _ in want if kind == 1])
    for h in (a, b):
        h.close()


def test_diff_skips_equal_subtrees(khst, oracle):
    """Identical handles take zero rounds past the root pair; 2,000 keys with 5 changed select fewer
    items than the two full scans (each side against an empty trie) -- by far."""
    from khipu_amd.device import Ctx, ResidentTrie, diff_counters
    ks, vs, sa, sb, ups, dels = _two(oracle, 2000, 5, 77)
    ctx = Ctx(0)
    a = ResidentTrie(ctx, ks, vs, emit=False)
    b = a.copy()
    assert a.diff(b) == ([], False, None) and diff_counters() == (0, 0)
    assert a.diff(a) == ([], False, None) and diff_counters() == (0, 0)
    assert b.commit(ups, dels) == sb[1]
    want = DR.expected_diff(*sa, *sb)
    assert _answer(lambda: a.diff(b)) == want and len(want[1]) == 5
    rounds, visited = diff_counters()
    e = ResidentTrie(ctx, [], [], emit=False)
    ents, more, _ = a.diff(e, max_entries=4000)
    assert [(k, kind) for k, kind, _ in ents] == [(k, 1) for k in ks] and not more
    scan_a = diff_counters()[1]
    ents, more, _ = e.diff(b, max_entries=4000)
    assert len(ents) == len(DR.content(*sb)) and {kind for _, kind, _ in ents} == {2}
    scan_b = diff_counters()[1]
    assert scan_a > 2000 and scan_b > 2000
    assert 0 < visited < 200 and visited < (scan_a + scan_b) // 20 and rounds <= 67
    for h in (a, b, e):
        h.close()


def test_diff_versions_and_compact(khst, oracle):
    """Under a savepoint the diff reads the commits since; after rollback the version before; a
    compacted handle diffs the same; handles on two contexts (two streams) as well."""
    from khipu_amd.device import Ctx, ResidentTrie
    ks, vs, sa, sb, ups, dels = _two(oracle, 300, 60, 41)
    ctx = Ctx(0)
    t = ResidentTrie(ctx, ks, vs, emit=False)
    base = t.copy()
    t.savepoint()
    assert t.commit(ups, dels) == sb[1]
    want = DR.expected_diff(*sa, *sb)
    back = DR.expected_diff(*sb, *sa)
    assert want[1] and _answer(lambda: base.diff(t)) == want and _answer(lambda: t.diff(base)) == back
    c = t.copy()
    t.rollback()
    assert base.diff(t) == ([], False, None)
    assert _answer(lambda: t.diff(c)) == want
    c.compact()
    base.compact()
    assert _answer(lambda: base.diff(c)) == want and _answer(lambda: c.diff(base)) == back
    other = ResidentTrie(Ctx(0), ks, vs, emit=False)  # (a context, and a stream, of its own)
    assert other.commit(ups, dels) == sb[1]
    assert _answer(lambda: base.diff(other)) == want and _answer(lambda: other.diff(c)) == ("page", [], False, None)
    for h in (t, base, c, other):
        h.close()


def test_diff_frontier_past_one_block_of_the_fill(khst, oracle):
    """More frontier items than one block of the fill holds (BS / EXP_LANES = 16), cut and uncut."""
    from khipu_amd.device import Ctx, ResidentTrie
    ks, vs, sa, sb, ups, dels = _two(oracle, 300, 150, 5)
    ctx = Ctx(0)
    a = ResidentTrie(ctx, ks, vs, emit=False)
    b = a.copy()
    assert b.commit(ups, dels) == sb[1]
    for mx in (15, 16, 17, 63, 64, 65, 257):
        assert _answer(lambda: a.diff(b, None, None, mx, BIG)) == DR.expected_diff(*sa, *sb, None, None, mx, BIG), mx
    assert len(DR.expected_diff(*sa, *sb, None, None, 257, BIG)[1]) > 100
    for h in (a, b):
        h.close()


def test_diff_partial_handles(khst, oracle):
    """A partial handle against its full twin: stubs skipped by their references cost nothing, so the
    diff is complete where both hold the changed paths; a stub that is not skipped gives KH_ENODE
    with the hash the reference names."""
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
    want = DR.expected_diff(*sa, *sb)
    assert len(want[1]) == 10
    for x, y, nx, ny in ((fa, pb, sa[0], wb), (pa, fb, wa, sb[0]), (pa, pb, wa, wb)):
        assert DR.expected_diff(nx, sa[1], ny, sb[1]) == want
        assert _answer(lambda: x.diff(y)) == want
        assert _answer(lambda: x.diff(y, None, None, 3, BIG)) == DR.expected_diff(nx, sa[1], ny, sb[1], None, None, 3, BIG)
    # a change outside the witness: the stub over it is not skipped
    out = next(k for k in ks if k not in some and P.kec(P.expected_proof(sb[0], sb[1], k)[0][-1]) not in wb)
    fc = fb.copy()
    root_c = fc.commit([(out, b"\x07" * 50)], [])
    DC.fold(o, [(out, b"\x07" * 50)], [])
    sc = DC.snap(o)
    assert root_c == sc[1]
    want = DR.expected_diff(wb, sb[1], sc[0], sc[1])
    assert want[0] == "missing" and want[1] in sb[0] and want[1] not in wb
    assert _answer(lambda: pb.diff(fc)) == want
    assert _answer(lambda: fc.diff(pb)) == DR.expected_diff(sc[0], sc[1], wb, sb[1]) == want
    # ... and a budget of one names it only when it is among the first two things
    first = DR.expected_diff(wa, sa[1], sc[0], sc[1], None, None, 1)
    assert _answer(lambda: pa.diff(fc, None, None, 1, BIG)) == first
    for h in (fa, fb, fc, pa, pb):
        h.close()


def test_diff_device_buffers(khst, oracle):
    """kh_dev_trie_diff: keys, kinds, values and offsets into device buffers, equal to the host form."""
    import torch
    from khipu_amd import _lib
    from khipu_amd.device import Ctx, ResidentTrie
    ks, vs, sa, sb, ups, dels = _two(oracle, 300, 150, 33)
    ctx = Ctx(0)
    a = ResidentTrie(ctx, ks, vs, emit=False)
    b = a.copy()
    assert b.commit(ups, dels) == sb[1]
    want = a.diff(b, max_entries=100, val_cap=1 << 16)
    dk = torch.zeros(32 * 100, dtype=torch.uint8, device="cuda:0")
    dkind = torch.zeros(100, dtype=torch.uint8, device="cuda:0")
    dv = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda:0")
    do = torch.zeros(101, dtype=torch.int64, device="cuda:0")
    ne, vb, more = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_int(0)
    nxt = np.zeros(32, np.uint8)
    ctx._sync()
    p = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    rc = _lib.lib().kh_dev_trie_diff(a.h, 0, b.h, 0, None, None, 100, 1 << 16, p(dk), p(dkind), p(dv), p(do),
                                     ctypes.byref(ne), ctypes.byref(vb), ctypes.byref(more), nxt.ctypes.data, None)
    assert rc == _lib.KH_OK and ne.value == 100 and more.value == 1
    off = do.cpu().numpy()
    kb, kinds, vbuf = dk.cpu().numpy().tobytes(), dkind.cpu().numpy(), dv.cpu().numpy().tobytes()
    assert int(off[100]) == vb.value
    assert ([(kb[32 * j:32 * j + 32], int(kinds[j]), vbuf[int(off[j]):int(off[j + 1])]) for j in range(100)], True,
            nxt.tobytes()) == want
    assert want == DR.expected_diff(*sa, *sb, None, None, 100, 1 << 16)[1:]
    for h in (a, b):
        h.close()


def test_diff_arguments(khst, oracle):
    from khipu_amd import _lib
    from khipu_amd.device import Ctx, ResidentForest, ResidentTrie
    r = random.Random(32)
    ks = sorted(C._rk(r) for _ in range(40))
    vs = [C.account_value(r) for _ in ks]
    ctx = Ctx(0)
    t = ResidentTrie(ctx, ks, vs, emit=False)
    e = ResidentTrie(ctx, [], [], emit=False)
    f = ResidentForest(ctx)
    for bad in (0, 1 << 31):
        with pytest.raises(_lib.MPTException):
            t.diff(e, max_entries=bad)
    out = np.zeros(64, np.uint8)
    w = ctypes.c_uint64(0)
    m = ctypes.c_int(0)
    args = (None, None, 1, 8, out.ctypes.data, out.ctypes.data, out.ctypes.data, out.ctypes.data, ctypes.byref(w),
            ctypes.byref(w), ctypes.byref(m), out.ctypes.data, None)
    assert _lib.lib().kh_trie_diff_host(t.h, 0, None, 0, *args) == _lib.KH_EINVAL
    assert _lib.lib().kh_trie_diff_host(None, 0, t.h, 0, *args) == _lib.KH_EINVAL
    assert t.diff(e, origin=ks[5], limit=ks[4]) == ([], False, None)  # origin > limit
    assert t.diff(e, origin=ks[5], limit=ks[5]) == ([(ks[5], 1, b"")], False, None)
    assert e.diff(t, origin=ks[5], limit=ks[5]) == ([(ks[5], 2, vs[5])], False, None)
    assert e.diff(t, max_entries=1 << 22, val_cap=1 << 16) == ([(k, 2, v) for k, v in zip(ks, vs)], False, None)
    assert e.diff(t, limit=ks[9], max_entries=9) == ([(k, 2, v) for k, v in zip(ks[:9], vs[:9])], True, ks[9])
    assert e.diff(e) == e.diff(ResidentTrie(ctx, [], [], emit=False)) == ([], False, None)
    # an id the forest does not hold is an empty side, on either side; one forest with two ids is allowed
    assert f.diff(7, t)[0] == [(k, 2, v) for k, v in zip(ks, vs)] and t.diff(f, other_trie=7)[0] == [(k, 1, b"") for k in ks]
    f.commit([(3, ks[0], b"\x01"), (4, ks[0], b"\x02"), (4, ks[1], b"\x03")], [])
    assert f.diff(3, f, 4) == ([(ks[0], 3, b"\x02"), (ks[1], 2, b"\x03")], False, None)
    assert f.diff(4, f, 4) == f.diff(9, f, 8) == ([], False, None)
    for h in (t, e, f):
        h.close()


def test_diff_through_the_jni_shim(khst, oracle, tmp_path):
    """Khst.diff through the in-process JNIEnv of tests/jni_stub: 400 keys, a block committed on a
    copy, the differences paged to the end by `next` with a value array that starts empty, so the
    grow path runs."""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    stub = os.path.join(ROOT, "tests", "jni_stub")
    exe = tmp_path / "jni_diff_driver"
    rc = subprocess.run([cc, "-std=gnu99", "-O1", "-Wall", "-Werror", "-I", stub, "-I", os.path.join(ROOT, "include"),
                         "-o", str(exe), os.path.join(stub, "jni_diff_driver.c"), os.path.join(stub, "fake_env.c"),
                         os.path.join(ROOT, "jni", "khst_jni.c"), "-L", os.path.join(ROOT, "khipu_amd"), "-lkhst",
                         "-Wl,-rpath," + os.path.join(ROOT, "khipu_amd"), "-Wl,-rpath-link,/opt/rocm/lib"],
                        capture_output=True, text=True)
    assert rc.returncode == 0, rc.stderr
    ks, vs, sa, sb, ups, dels = _two(oracle, 400, 90, 808)

    def packed(keys, vals):
        voff = np.zeros(len(vals) + 1, np.uint64)
        voff[1:] = np.cumsum([len(v) for v in vals])
        return np.uint64(len(keys)).tobytes() + b"".join(keys) + voff.tobytes() + b"".join(vals)
    q = [(DC.ZERO, DC.FF, 64), (DC.ZERO, DC.FF, 7), (ks[100], ks[300], 1), (DC.FF, DC.ZERO, 5)]
    p = tmp_path / "in.bin"
    with open(p, "wb") as f:
        f.write(packed(ks, vs) + packed([k for k, _ in ups], [v for _, v in ups]))
        f.write(np.uint64(len(dels)).tobytes() + b"".join(dels))
        f.write(np.uint64(len(q)).tobytes() + b"".join(a + b + np.uint64(mx).tobytes() for a, b, mx in q))
    rc = subprocess.run([str(exe), str(p)], capture_output=True, text=True, timeout=120)
    assert rc.returncode == 0, rc.stderr
    lines = [ln.split() for ln in rc.stdout.split("\n")[:-1]]
    assert lines[-1] == ["E", "0"], lines[-1]
    assert bytes.fromhex(lines[0][1]) == sb[1]
    full = [(t[1], t[2], t[3]) for t in DR.walk_diff(*sa, *sb)]
    for j, (a, b, mx) in enumerate(q):
        got = [(bytes.fromhex(x[2]), int(x[3]), b"" if x[4] == "-" else bytes.fromhex(x[4])) for x in lines
               if x[0] == "K" and x[1] == str(j)]
        want = [d for d in full if a <= d[0] <= b]
        assert got == want, j
        _, n, pages, grows = [x for x in lines if x[0] == "Q" and x[1] == str(j)][0][1:]
        assert int(n) == len(want) and int(pages) >= max(1, -(-len(want) // mx))
        assert int(grows) >= (1 if any(v for _, _, v in want) else 0)
