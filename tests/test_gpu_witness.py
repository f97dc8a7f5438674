"""GPU: commit witnesses (kh_trie_commit_witness_host) -- every node a handle opened from a witness
needs to commit a batch at the first attempt, the sibling a collapsing branch is merged with
included.  The expected witness is tests/witness_ref.expected (node encodings and key sets alone);
sufficiency and minimality are checked against the engine itself: a handle opened by from_witness
commits the batch to the oracle's root, and without any one node the open or the commit raises
MPTNodeMissingException.  The shapes are the commit scenarios, hand cases with known answers and
two dense-key sequences."""
import ctypes
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

from tests import cases as C
from tests import fuzz_cases as F
from tests import partial_cases as P
from tests import proof_ref
from tests import witness_cases as WC
from tests import witness_ref
from tests import writeback as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMPTY = W.EMPTY_TRIE_HASH
MINIMAL_CAP = 64  # nodes: only bounds the drop-one loop's time


def _trie(oracle, keys, vals):
    o = oracle.Trie()
    for k, v in zip(keys, vals):
        o.put(k, v)
    return o


def _fold(o, ups, dels):
    for k, v in ups:
        o.put(k, v)
    for k in dels:
        o.remove(k)
    return o.root_hash()


def _check_batch(khst, ctx, full, pre, root, live, ups, dels, new_root, tag, minimal=None, strict=False,
                 hash_keys=False, enc=None):
    """One batch on the full handle `full` (at `root`, store `pre`, trie keys `live`): the witness
    equals the reference's, a handle opened from it commits the batch to new_root, and no node can
    be dropped -- minimal: None (not asked), or the largest witness the drop-one loop runs on
    (strict: a larger one fails).  enc: raw key -> trie key (a KH_HASH_KEYS handle).  Returns the witness."""
    from khipu_amd.device import ResidentTrie
    enc = enc or (lambda k: k)
    wit, ncol = full.commit_witness(ups, dels)
    want, want_col = witness_ref.expected(pre, root, live, [enc(k) for k, _ in ups], [enc(k) for k in dels])
    assert set(wit) == want, (tag, len(set(wit) - want), len(want - set(wit)))
    assert all(pre[h] == e for h, e in wit.items()), tag
    assert ncol == want_col and full.witness_nodes == len(want), tag
    if not ups and not dels:  # (no ops: nothing is needed, not even the root a handle opens from)
        assert wit == {}, tag
        return wit
    # sufficient
    p = ResidentTrie.from_witness(ctx, root, wit, hash_keys=hash_keys)
    assert p.commit(ups, dels) == new_root, tag
    assert p.missing() == [], tag
    p.close()
    if strict:
        assert len(wit) <= minimal, (tag, len(wit))
    if minimal is not None and len(wit) <= minimal:
        for h in wit:
            less = {x: e for x, e in wit.items() if x != h}
            with pytest.raises(khst.MPTNodeMissingException):
                q = ResidentTrie.from_witness(ctx, root, less, hash_keys=hash_keys)  # (the root: refused here)
                try:
                    q.commit(ups, dels)
                finally:
                    q.close()
    return wit


MINIMAL = ("single", "to_empty", "recut_opened_branch", "deep")


@pytest.mark.parametrize("sc", C.commit_scenarios(), ids=lambda s: s[0])
def test_commit_scenarios(khst, oracle, sc):
    """Equality, sufficiency and (the small ones) minimality on every batch, asked before the batch
    is applied; then the full handle's own commit gives the same root."""
    from khipu_amd.device import Ctx, ResidentTrie
    name, ks, vs, batches = sc
    ctx = Ctx(0)
    o = _trie(oracle, ks, vs)
    full = ResidentTrie(ctx, ks, vs)
    live = set(ks)
    for i, (ups, dels) in enumerate(batches):
        pre, root = W.reachable(o), o.root_hash()
        new_root = _fold(o, ups, dels)
        wit = _check_batch(khst, ctx, full, pre, root, live, ups, dels, new_root, (name, i),
                           MINIMAL_CAP if name in MINIMAL else None)
        assert full.get_root() == root  # (read-only)
        assert full.commit(ups, dels) == new_root, (name, i)
        live = (live | {k for k, _ in ups}) - set(dels)
        if name == "large_batch":
            assert len(ups) + len(dels) == 1500 and len(wit) > 256  # (more than a block of ops and of nodes)
    full.close()


@pytest.mark.parametrize("case", WC.hand_cases(), ids=lambda c: c[0])
def test_hand_cases(khst, oracle, case):
    from khipu_amd.device import Ctx, ResidentTrie
    name, ks, vs, ups, dels, cover, ncol = case
    ctx = Ctx(0)
    o = _trie(oracle, ks, vs)
    pre, root = o.reachable(), o.root_hash()
    full = ResidentTrie(ctx, ks, vs)
    new_root = _fold(o, ups, dels)
    wit = _check_batch(khst, ctx, full, pre, root, set(ks), ups, dels, new_root, name, MINIMAL_CAP, strict=True)
    assert set(wit) == WC.want(pre, root, cover) and full.commit_witness(ups, dels)[1] == ncol
    assert full.commit(ups, dels) == new_root
    full.close()


@pytest.mark.parametrize("seed", F.TRIE_SEEDS[:2])
def test_dense_key_sequences(khst, oracle, seed):
    """20 steps of a dense-key sequence (value-only branches, long extensions, word-edge depths):
    before every accepted commit the handle is opened from the model's store and asked."""
    from khipu_amd.device import Ctx, ResidentTrie
    ctx = Ctx(0)
    pre, n = None, 0
    for i, step, m in F.trie_run(seed, oracle, nsteps=20):
        if step["op"] == "commit" and not step["refused"] and pre[1] != EMPTY:
            nodes, root, live = pre
            full = ResidentTrie.from_nodes(ctx, root, nodes)
            _check_batch(khst, ctx, full, nodes, root, live, step["ups"], step["dels"], m.root(), (seed, i), 24)
            full.close()
            n += 1
        pre = (dict(W.reachable(m.t)), m.root(), set(m.live))
    assert n >= 2


def test_hashed_20_byte_keys(khst, oracle):
    """A KH_HASH_KEYS handle with 20-byte keys: the witness is that of the hashed keys."""
    from khipu_amd.device import Ctx, ResidentTrie
    r = random.Random(20)
    ctx = Ctx(0)
    raw = [bytes(r.getrandbits(8) for _ in range(20)) for _ in range(300)]
    vs = [C.account_value(r) for _ in raw]
    enc = proof_ref.kec
    o = _trie(oracle, [enc(k) for k in raw], vs)
    full = ResidentTrie(ctx, raw, vs, hash_keys=True)
    pre, root = o.reachable(), o.root_hash()
    assert full.root == root
    new = [bytes(r.getrandbits(8) for _ in range(20)) for _ in range(6)]
    ups = [(k, C.account_value(r)) for k in r.sample(raw, 10) + new]
    dels = r.sample(raw, 40) + new[:2] + [bytes(20)]
    new_root = _fold(o, [(enc(k), v) for k, v in ups], [enc(k) for k in dels])
    _check_batch(khst, ctx, full, pre, root, {enc(k) for k in raw}, ups, dels, new_root, "hashed",
                 hash_keys=True, enc=enc)
    assert full.commit(ups, dels) == new_root
    full.close()


@pytest.mark.parametrize("name", ["storage", "deep", "to_empty"])
def test_against_the_fetch_loop(khst, oracle, name):
    """What the call replaces: a handle opened with the root node only commits the batch by
    tests/test_gpu_partial.py::test_fetch_loop's retry loop; the nodes supplied, plus the root, are
    exactly the witness."""
    from khipu_amd.device import Ctx, ResidentTrie
    _, ks, vs, batches = next(s for s in C.commit_scenarios() if s[0] == name)
    ctx = Ctx(0)
    o = _trie(oracle, ks, vs)
    full = ResidentTrie(ctx, ks, vs)
    for i, (ups, dels) in enumerate(batches):
        pre, root = W.reachable(o), o.root_hash()
        new_root = _fold(o, ups, dels)
        if root == EMPTY:
            assert full.commit_witness(ups, dels) == ({}, 0)
            assert full.commit(ups, dels) == new_root
            continue
        wit, _ = full.commit_witness(ups, dels)
        t = ResidentTrie.from_witness(ctx, root, {root: pre[root]})
        supplied = {root}
        for rounds in range(131):
            try:
                got = t.commit(ups, dels)
                break
            except khst.MPTNodeMissingException:
                hs = {h for _, h in t.missing()}
                assert hs and not hs & supplied, (name, i, rounds)
                assert t.fill({h: pre[h] for h in hs}) == len(hs)
                supplied |= hs
        else:
            raise AssertionError((name, i, "more than 130 rounds"))
        assert got == new_root and supplied == set(wit), (name, i, len(supplied), len(wit))
        t.close()
        assert full.commit(ups, dels) == new_root
    full.close()


def _state(t, forest=False):
    return (t.roots() if forest else t.get_root(), list(t.export_nodes()), t.stubs, len(t),
            t.last_roots() if forest else None, t.nodes(), t.missing())


def test_read_only(khst, oracle):
    """Root, export bytes and order, a cursor in flight, stubs, len, the write-back set and the
    missing list are as before the call; again with a savepoint open after a commit, where the call
    reads the commits since the savepoint."""
    from khipu_amd.device import Ctx, ResidentTrie
    _, ks, vs, batches = next(s for s in C.commit_scenarios() if s[0] == "storage")
    ctx = Ctx(0)
    o = _trie(oracle, ks, vs)
    t = ResidentTrie(ctx, ks, vs, emit=True)
    live = set(ks)
    (u0, d0), (u1, d1), (u2, d2) = batches
    assert t.commit(u0, d0) == _fold(o, u0, d0)
    live = (live | {k for k, _ in u0}) - set(d0)
    before = _state(t)
    cur = t.export_cursor()
    first, done = t.export_chunk(cur, node_cap=3)
    assert not done
    want = witness_ref.expected(W.reachable(o), o.root_hash(), live, [k for k, _ in u1], d1)
    wit, ncol = t.commit_witness(u1, d1)
    assert (set(wit), ncol) == want
    rest = []
    while not done:  # the cursor from before the call goes on (get_root, a root_of, would end it)
        pairs, done = t.export_chunk(cur)
        rest += pairs
    assert first + rest == before[1]
    assert _state(t) == before
    # a savepoint, a commit, the call: the version after that commit is read; then back
    t.savepoint()
    assert t.commit(u1, d1) == _fold(o, u1, d1)
    live = (live | {k for k, _ in u1}) - set(d1)
    mid = _state(t)
    want = witness_ref.expected(W.reachable(o), o.root_hash(), live, [k for k, _ in u2], d2)
    wit, ncol = t.commit_witness(u2, d2)
    assert (set(wit), ncol) == want and ncol > 0
    assert _state(t) == mid and t.savepoint_depth() == 1
    t.rollback()
    assert _state(t) == before
    t.close()


def test_forest(khst, oracle):
    """A batch over four tries of a forest, an id it does not hold and a trie the batch empties:
    the witness is the per-trie reference's, a node two tries hold is listed once per trie, and a
    forest loaded partially from it commits the batch to the oracle's roots."""
    from khipu_amd.device import Ctx, ResidentForest
    r = random.Random(31)
    ctx = Ctx(0)
    ids = F.FOREST_IDS
    kv = {}
    for j, t in enumerate(ids):
        ks = [C._rk(r) for _ in range([60, 3, 120, 40, 25][j])]
        kv[t] = dict(zip(ks, [C.storage_value(r) if j % 2 else C.account_value(r) for _ in ks]))
    kv[ids[3]] = dict(kv[ids[0]])  # two ids, one root: every node of one is a node of the other
    tr = {t: _trie(oracle, list(kv[t]), list(kv[t].values())) for t in ids}
    roots = {t: o.root_hash() for t, o in tr.items()}
    store = {}
    for o in tr.values():
        store.update(o.reachable())
    full = ResidentForest.from_nodes(ctx, roots, store, emit=True)
    absent = 12345
    ups, dels = [], []
    shared = list(kv[ids[0]])[:5]
    for t in (ids[0], ids[3]):  # the same ops in the two equal tries
        ups += [(t, k, b"n" * 40) for k in shared[:2]] + [(t, C._rk(r), b"m" * 35)]
        dels += [(t, k) for k in shared[2:]]
    ups += [(ids[2], k, C.account_value(r)) for k in list(kv[ids[2]])[:8]] + [(absent, C._rk(r), b"x" * 33)]
    dels += [(ids[2], k) for k in list(kv[ids[2]])[60:100]] + [(absent, C._rk(r))]
    dels += [(ids[1], k) for k in kv[ids[1]]]  # emptied
    touched = [ids[0], ids[3], ids[2], ids[1]]
    want, want_col, total = set(), 0, 0
    for t in touched:
        w, n = witness_ref.expected(tr[t].reachable(), roots[t], set(kv[t]), [k for x, k, _ in ups if x == t],
                                    [k for x, k in dels if x == t])
        want |= w
        want_col += n
        total += len(w)
    before = _state(full, forest=True)
    wit, ncol = full.commit_witness(ups, dels)
    assert set(wit) == want and all(store[h] == e for h, e in wit.items())
    assert ncol == want_col and full.witness_nodes == total and total > len(want)  # once per trie
    assert _state(full, forest=True) == before
    new_roots = {}
    for t in touched:
        new_roots[t] = _fold(tr[t], [(k, v) for x, k, v in ups if x == t], [k for x, k in dels if x == t])
    assert new_roots[ids[1]] == EMPTY
    pf = ResidentForest(ctx)
    pf.load_partial({t: roots[t] for t in touched}, wit)
    assert pf.stubs > 0
    got = pf.commit(ups, dels)
    assert pf.missing() == []
    assert {t: got.get(t, EMPTY) for t in touched} == new_roots
    assert full.commit(ups, dels) == got
    # trie ids are required on a forest
    with pytest.raises(khst.MPTException):
        full._commit_witness([k for _, k, _ in ups], None, [], None)
    pf.close()
    full.close()


def test_partial_handles(khst, oracle):
    """On a handle opened from W(B1) the call gives W(B1) again; a batch that reaches stubs, and
    one whose only need is a collapse onto a plain stub, raise with the list the commit of the same
    batch leaves in missing(); the handle is unchanged both times."""
    from khipu_amd.device import Ctx, ResidentTrie
    r = random.Random(8)
    ctx = Ctx(0)
    ks = [C._rk(r) for _ in range(300)]
    vs = [C.account_value(r) for _ in ks]
    o = _trie(oracle, ks, vs)
    pre, root = o.reachable(), o.root_hash()
    full = ResidentTrie(ctx, ks, vs)
    b1 = ([(k, C.account_value(r)) for k in r.sample(ks, 8)] + [(C._rk(r), b"v" * 40)], r.sample(ks, 12))
    wit, ncol = full.commit_witness(*b1)
    assert ncol > 0
    p = ResidentTrie.from_witness(ctx, root, wit)
    assert p.stubs > 0
    before = _state(p)
    assert p.commit_witness(*b1) == (wit, ncol)
    assert _state(p) == before
    # B2: keys whose paths leave the witness
    held = set(wit)
    out = [k for k in ks if not set(P.path_hashes(pre, root, k)[0]) <= held][:6]
    assert len(out) == 6
    b2 = ([(out[0], b"w" * 40), (b1[0][0][0], b"w" * 41)], out[1:])
    with pytest.raises(khst.MPTNodeMissingException) as e:
        p.commit_witness(*b2)
    listed = e.value.missing
    assert len(listed) == len(set(listed)) >= 1 and _state(p) == before
    with pytest.raises(khst.MPTNodeMissingException):
        p.commit(*b2)
    assert sorted(p.missing()) == sorted(listed)
    assert {h for _, h in listed} <= P.fetchable(pre, root, out) - held
    p.close()
    full.close()
    # the collapse onto a plain stub: {A, B} held as {root, A}; deleting A needs leaf B
    o = _trie(oracle, [WC.A, WC.B], WC.V[:2])
    nodes, root = o.reachable(), o.root_hash()
    hA, hB = (P.path_hashes(nodes, root, k)[0][-1] for k in (WC.A, WC.B))
    t = ResidentTrie.from_witness(ctx, root, {root: nodes[root], hA: nodes[hA]})
    before = _state(t)
    with pytest.raises(khst.MPTNodeMissingException) as e:
        t.commit_witness(deletes=[WC.A])
    assert e.value.missing == [(0, hB)] and e.value.code == -4 and _state(t) == before
    with pytest.raises(khst.MPTNodeMissingException):
        t.commit(deletes=[WC.A])
    assert t.missing() == [(0, hB)]
    # miss_cap 0 still reports the number; nothing else is written
    rc, (nn, nl, nc, nm), (hs, rl, of, mt, mh) = t.commit_witness_raw([], None, [WC.A], None)
    assert rc == khst._lib.KH_ENODE and nm == 1 and (nn, nl, nc) == (0, 0, 0) and not mh.any()
    t.close()


def test_negotiation_and_arguments(khst, oracle):
    from khipu_amd import _lib
    from khipu_amd.device import Ctx, ResidentForest, ResidentTrie
    lib = _lib.lib()
    ctx = Ctx(0)
    o = _trie(oracle, [WC.A, WC.B], WC.V[:2])
    nodes, root = o.reachable(), o.root_hash()
    t = ResidentTrie(ctx, [WC.A, WC.B], WC.V[:2])
    # KH_ENOSPC writes the sizes; a retry with exactly those succeeds
    rc, (nn, nl, nc, nm), _ = t.commit_witness_raw([], None, [WC.A], None)
    assert rc == _lib.KH_ENOSPC and nn == 3 and nl == sum(len(e) for e in nodes.values())
    for caps in ((nn - 1, nl), (nn, nl - 1)):
        assert t.commit_witness_raw([], None, [WC.A], None, caps)[0] == _lib.KH_ENOSPC
    rc, sizes, (hs, rl, of, _, _) = t.commit_witness_raw([], None, [WC.A], None, (nn, nl))
    assert rc == _lib.KH_OK and sizes == (3, nl, 1, 0)
    assert {hs[32 * j:32 * j + 32].tobytes(): rl[int(of[j]):int(of[j + 1])].tobytes() for j in range(3)} == nodes
    # no ops
    rc, sizes, _ = t.commit_witness_raw([], None, [], None)
    assert rc == _lib.KH_OK and sizes == (0, 0, 0, 0)
    assert t.commit_witness() == ({}, 0)
    # KH_EINVAL
    bad = (_lib.KH_EINVAL, (0, 0, 0, 0))
    assert t.commit_witness_raw([b"\x01" * 20], None, [], None)[:2] == bad            # klen on a raw-key handle
    assert t.commit_witness_raw([WC.A], None, [], None, flags=_lib.KH_HASH_KEYS)[:2] == bad  # the handle's encoder
    assert t.commit_witness_raw([WC.A], None, [], None, flags=1 << 30)[:2] == bad      # unknown flag
    f = ResidentForest(ctx)
    f.commit([(5, WC.A, b"v" * 40)], [])
    assert f.commit_witness_raw([WC.A], None, [], None)[:2] == bad                     # a forest without trie ids
    assert f.commit_witness_raw([WC.A], [5], [WC.B], None)[:2] == bad
    assert f.commit_witness_raw([WC.A], [5], [WC.B], [5], (8, 4096))[0] == _lib.KH_OK
    kb = np.frombuffer(WC.A, np.uint8).copy()
    n64 = ctypes.c_uint64
    a, b, c, d = n64(0), n64(0), n64(0), n64(0)
    args = lambda h, nup, outs: lib.kh_trie_commit_witness_host(  # noqa: E731
        h, None, kb.ctypes.data, nup, None, None, 0, 32, 0, None, 0, None, 0, None, *outs, None, None, 0, ctypes.byref(d))
    ok = (ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
    assert args(None, 1, ok) == _lib.KH_EINVAL                                          # a null handle
    assert args(t.h, 1, (None, ctypes.byref(b), ctypes.byref(c))) == _lib.KH_EINVAL     # a null required output
    assert args(t.h, 1, (ctypes.byref(a), ctypes.byref(b), None)) == _lib.KH_ENOSPC     # n_collapse is nullable
    assert args(t.h, 1 << 31, ok) == _lib.KH_EINVAL                                     # nup + ndel >= 2^31
    assert lib.kh_trie_commit_witness_host(t.h, None, None, 1, None, None, 0, 32, 0, None, 0, None, 0, None, *ok, None,
                                           None, 0, ctypes.byref(d)) == _lib.KH_EINVAL  # null keys
    assert t.get_root() == root
    f.close()
    t.close()


def test_through_the_jni_shim(khst, oracle, tmp_path):
    """Khst.commitWitness through the in-process JNIEnv of tests/jni_stub: the same table as ctypes
    on the storage scenario's first batch (updates, and deletes that collapse branches)."""
    from khipu_amd.device import Ctx, ResidentTrie
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    stub = os.path.join(ROOT, "tests", "jni_stub")
    exe = tmp_path / "jni_witness_driver"
    rc = subprocess.run([cc, "-std=gnu99", "-O1", "-Wall", "-Werror", "-I", stub, "-I", os.path.join(ROOT, "include"),
                         "-o", str(exe), os.path.join(stub, "jni_witness_driver.c"), os.path.join(stub, "fake_env.c"),
                         os.path.join(ROOT, "jni", "khst_jni.c"), "-L", os.path.join(ROOT, "khipu_amd"), "-lkhst",
                         "-Wl,-rpath," + os.path.join(ROOT, "khipu_amd"), "-Wl,-rpath-link,/opt/rocm/lib"],
                        capture_output=True, text=True)
    assert rc.returncode == 0, rc.stderr
    _, ks, vs, batches = next(s for s in C.commit_scenarios() if s[0] == "storage")
    ups, dels = batches[0]
    t = ResidentTrie(Ctx(0), ks, vs)
    rc_, (nn, nl, _, _), _ = t.commit_witness_raw([k for k, _ in ups], None, dels, None)
    assert rc_ == khst._lib.KH_ENOSPC
    rc_, (_, _, nc, _), (hs, rl, of, _, _) = t.commit_witness_raw([k for k, _ in ups], None, dels, None, (nn, nl))
    assert rc_ == khst._lib.KH_OK and nc > 0
    t.close()
    voff = np.zeros(len(ks) + 1, np.uint64)
    voff[1:] = np.cumsum([len(v) for v in vs])
    p = tmp_path / "in.bin"
    with open(p, "wb") as f:
        f.write(np.array([len(ks), len(ups), len(dels)], np.uint64).tobytes())
        f.write(b"".join(ks) + voff.tobytes() + b"".join(vs))
        f.write(b"".join(k for k, _ in ups) + b"".join(dels))
    r = subprocess.run([str(exe), str(p)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = [ln.split() for ln in r.stdout.split("\n")[:-1]]
    assert lines[0] == ["W", "0", str(nn), str(nl), str(nc)], lines[0]
    got = [(bytes.fromhex(x[1]), bytes.fromhex(x[2])) for x in lines if x[0] == "N"]
    # (table order is the handle's record order: the two handles were opened by different calls)
    assert sorted(got) == sorted((hs[32 * j:32 * j + 32].tobytes(), rl[int(of[j]):int(of[j + 1])].tobytes())
                                 for j in range(nn))
    assert lines[-1] == ["E", "0"]
