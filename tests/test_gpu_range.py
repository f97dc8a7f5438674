"""GPU: a resident trie or forest read in key order (kh_trie_range_host / kh_dev_trie_range), held to
tests/range_ref.py over the oracle's nodes: pages, `more` and `next`, the fit to val_cap, the
refusal of a partial handle, and the boundary proofs of a page."""
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

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMPTY = P.EMPTY_ROOT
SCEN = C.commit_scenarios()


def _oracle(oracle, ks, vs):
    o = oracle.Trie()
    for k, v in zip(ks, vs):
        o.put(k, v)
    return o


def _fold(o, ups, dels):
    for k, v in ups:
        o.put(k, v)
    for k in dels:
        o.remove(k)


def _nodes(o):
    return o.reachable() if o.root_hash() != EMPTY else {}


def _page(call):
    """A range call's answer in the form of range_ref.expected_range."""
    from khipu_amd import _lib
    try:
        keys, vals, more, nxt = call()
    except _lib.MPTNodeMissingException as e:
        return ("missing", e.missing)
    except _lib.KhError as e:
        assert e.code == _lib.KH_ENOSPC
        return ("nospc", e.val_bytes)
    return ("page", keys, vals, more, nxt)


def _check_state(t, o, r, tag, nranges=200, chunks=(1, 7, 1000), **kw):
    """items() in chunks and nranges random ranges of handle t (kw: trie=id on a forest) against o."""
    snap = RR.Snapshot(_nodes(o), o.root_hash())
    for chunk in chunks:
        assert list(t.items(chunk=chunk, **kw)) == snap.items, (tag, chunk)
    for a, b, mx in RC.random_ranges(r, snap.keys, nranges):
        assert _page(lambda: t.range(origin=a, limit=b, max_entries=mx, **kw)) == snap.expected_range(a, b, mx), \
            (tag, a and a.hex(), b and b.hex(), mx)
    return snap


@pytest.mark.parametrize("i", range(len(SCEN)), ids=[s[0] for s in SCEN])
def test_range_after_commits(khst, oracle, i):
    from khipu_amd.device import Ctx, ResidentTrie
    name, ks, vs, batches = SCEN[i]
    o = _oracle(oracle, ks, vs)
    t = ResidentTrie(Ctx(0), ks, vs, emit=False)
    for b in range(len(batches) + 1):
        if b:
            _fold(o, *batches[b - 1])
            assert t.commit(*batches[b - 1]) == o.root_hash(), (name, b)
        _check_state(t, o, random.Random(1000 * i + b), (name, b))
    t.close()


def test_range_hashed_handle(khst, oracle):
    """A KH_HASH_KEYS handle: the keys of a page are the kec256 values."""
    from khipu_amd.device import Ctx, ResidentTrie
    r = random.Random(20)
    ks = [bytes(r.getrandbits(8) for _ in range(20)) for _ in range(300)]
    vs = [C.account_value(r) if i % 2 else C.storage_value(r) for i in range(len(ks))]
    o = _oracle(oracle, [oracle.kec256(k) for k in ks], vs)
    t = ResidentTrie(Ctx(0), ks, vs, hash_keys=True, emit=False)
    _check_state(t, o, r, "open")
    ups, dels = [(k, C.account_value(r)) for k in ks[:20]] + [(b"new" + bytes([j]) * 17, b"\x05") for j in range(9)], ks[50:90]
    _fold(o, [(oracle.kec256(k), v) for k, v in ups], [oracle.kec256(k) for k in dels])
    assert t.commit(ups, dels) == o.root_hash()
    _check_state(t, o, r, "commit")
    t.close()


def test_range_val_cap(khst, oracle):
    """val_cap at exactly a page's bytes, one less, the first value, one less than it, and 0."""
    from khipu_amd.device import Ctx, ResidentTrie
    r = random.Random(31)
    ks = [C._rk(r) for _ in range(300)]
    vs = [C.account_value(r) if i % 3 else C.storage_value(r) for i in range(len(ks))]
    o = _oracle(oracle, ks, vs)
    t = ResidentTrie(Ctx(0), ks, vs, emit=False)
    snap = RR.Snapshot(_nodes(o), o.root_hash())
    origin = snap.keys[17]
    full = snap.expected_range(origin, None, 64)
    total, first = sum(len(v) for v in full[2]), len(full[2][0])
    got = [_page(lambda: t.range(origin, None, 64, cap)) for cap in (total, total - 1, first, first - 1, 0)]
    assert got == [snap.expected_range(origin, None, 64, cap) for cap in (total, total - 1, first, first - 1, 0)]
    assert len(got[0][1]) == 64 and len(got[1][1]) == 63 and got[1][3] and got[1][4] == full[1][63]
    assert len(got[2][1]) == 1 and got[3] == got[4] == ("nospc", first)
    # items() grows val_cap when a value does not fit the first page
    from khipu_amd.device import _range_items
    assert list(_range_items(t.h, None, None, 50, None, val_cap=1)) == snap.items
    t.close()


def test_range_arguments(khst, oracle):
    from khipu_amd import _lib
    from khipu_amd.device import Ctx, ResidentForest, ResidentTrie
    r = random.Random(32)
    ks = sorted(C._rk(r) for _ in range(40))
    vs = [C.account_value(r) for _ in ks]
    t = ResidentTrie(Ctx(0), ks, vs, emit=False)
    for bad in (0, 1 << 31):
        with pytest.raises(_lib.MPTException):
            t.range(max_entries=bad)
    assert t.range(origin=ks[5], limit=ks[4]) == ([], [], False, None)  # origin > limit
    assert t.range(origin=ks[5], limit=ks[5]) == ([ks[5]], [vs[5]], False, None)
    assert t.range(max_entries=1 << 22, val_cap=1 << 16)[:3] == (ks, vs, False)  # (frontiers sized by the trie)
    assert t.range(limit=ks[9], max_entries=10) == (ks[:10], vs[:10], False, None)
    assert t.range(limit=ks[9], max_entries=9) == (ks[:9], vs[:9], True, ks[9])
    e = ResidentTrie(Ctx(0), [], [], emit=False)
    assert e.range() == ([], [], False, None) and list(e.items()) == []
    f = ResidentForest(Ctx(0))
    assert f.range(7) == ([], [], False, None)
    for h in (t, e, f):
        h.close()


def test_range_device_buffers(khst, oracle):
    """kh_dev_trie_range: keys, values and offsets into device buffers, equal to the host form."""
    import torch
    from khipu_amd import _lib
    from khipu_amd.device import Ctx, ResidentTrie
    r = random.Random(33)
    ks = [C._rk(r) for _ in range(300)]
    vs = [C.account_value(r) for _ in ks]
    ctx = Ctx(0)
    t = ResidentTrie(ctx, ks, vs, emit=False)
    want = t.range(max_entries=100, val_cap=1 << 16)
    dk = torch.zeros(32 * 100, dtype=torch.uint8, device="cuda:0")
    dv = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda:0")
    do = torch.zeros(101, dtype=torch.int64, device="cuda:0")
    ne, vb, more = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_int(0)
    nxt = np.zeros(32, np.uint8)
    ctx._sync()
    rc = _lib.lib().kh_dev_trie_range(t.h, 0, None, None, 100, ctypes.c_void_p(dk.data_ptr()),
                                      ctypes.c_void_p(dv.data_ptr()), 1 << 16, ctypes.c_void_p(do.data_ptr()),
                                      ctypes.byref(ne), ctypes.byref(vb), ctypes.byref(more), nxt.ctypes.data, None)
    assert rc == _lib.KH_OK and ne.value == 100 and more.value == 1
    off = do.cpu().numpy()
    kb, vbuf = dk.cpu().numpy().tobytes(), dv.cpu().numpy().tobytes()
    assert int(off[100]) == vb.value
    assert ([kb[32 * j:32 * j + 32] for j in range(100)], [vbuf[int(off[j]):int(off[j + 1])] for j in range(100)], True,
            nxt.tobytes()) == want
    t.close()


def _forest(oracle):
    """60 tries over 3 blocks with hashed 32-byte slots and ids up to 2^32, and twin tries holding
    the same slots and values."""
    from khipu_amd.device import Ctx, ResidentForest
    r = random.Random(78)
    f = ResidentForest(Ctx(0), hash_keys=True, emit=False)
    tries = {}
    ids = [r.randrange(1 << 16, 1 << 32) for _ in range(56)] + [0, 7, 65535, 65536]
    twins = [r.randrange(1 << 32) for _ in range(2)]
    for blk in range(3):
        ups, dels = [], []
        for t in (ids if blk == 0 else r.sample(ids, 25)):
            for _ in range(r.choice([1, 3, 10, 40])):
                ups.append((t, bytes(r.getrandbits(8) for _ in range(32)), C.storage_value(r)))
        if blk == 1:
            ups += [(tw, bytes([j]) * 32, b"\x01" * 40) for tw in twins for j in range(6)]
        if blk == 2:
            dels = [(t, s) for t, s, _ in r.sample(first, 30)]
        if blk == 0:
            first = list(ups)
        got = f.commit(ups, dels)
        for t, slot, v in ups:
            tries.setdefault(t, oracle.Trie()).put(oracle.kec256(slot), v)
        for t, slot in dels:
            tries[t].remove(oracle.kec256(slot))
        for t in got:
            assert got[t] == tries[t].root_hash(), (blk, t)
    return f, tries, ids, twins


def test_range_forest(khst, oracle):
    f, tries, ids, twins = _forest(oracle)
    assert len(ids) == 60 and max(ids) >= 1 << 16
    r = random.Random(6)
    for t in ids + twins:
        _check_state(f, tries[t], r, t, nranges=6, chunks=(1, 1000), trie=t)
    assert list(f.items(twins[0])) == list(f.items(twins[1])) and len(list(f.items(twins[0]))) == 6
    unheld = next(x for x in range(1 << 20, 1 << 21) if x not in tries)
    assert f.range(unheld) == ([], [], False, None)
    f.close()


def test_range_versions_copy_compact_reopen(khst, oracle):
    """Under a savepoint a page reads the commits since; after rollback the version before; a copy,
    a compacted handle and a handle reopened from the exported nodes read the same."""
    from khipu_amd.device import Ctx, ResidentTrie
    r = random.Random(41)
    ks = [C._rk(r) for _ in range(300)]
    vs = [C.account_value(r) for _ in ks]
    o = _oracle(oracle, ks, vs)
    ctx = Ctx(0)
    t = ResidentTrie(ctx, ks, vs, emit=False)
    before = _check_state(t, o, r, "open", nranges=30, chunks=(7,))
    t.savepoint()
    ups, dels = [(k, C.account_value(r)) for k in ks[:30]] + [(C._rk(r), b"\x09") for _ in range(30)], ks[100:160]
    _fold(o, ups, dels)
    assert t.commit(ups, dels) == o.root_hash()
    after = _check_state(t, o, r, "savepoint", nranges=30, chunks=(7,))
    assert after.items != before.items
    c = t.copy()
    t.rollback()
    assert list(t.items(chunk=1000)) == before.items
    assert list(c.items(chunk=1000)) == after.items
    c.compact()
    _check_state(c, o, r, "compact", nranges=30, chunks=(7,))
    root, nodes = c.checkpoint()
    c2 = ResidentTrie.from_nodes(ctx, root, nodes, emit=False)
    _check_state(c2, o, r, "from_nodes", nranges=30, chunks=(7,))
    for h in (t, c, c2):
        h.close()


def test_range_partial_handle(khst, oracle):
    """A partial handle refuses with the hash the reference's walk over the held nodes names, and
    serves the pages that end before a missing subtree; a fetch loop from the root alone ends with
    the whole content."""
    from khipu_amd import _lib
    from khipu_amd.device import Ctx, ResidentTrie
    r = random.Random(51)
    ks = sorted(C._rk(r) for _ in range(120))
    vs = [C.account_value(r) if i % 4 else C.storage_value(r) for i in range(len(ks))]
    o = _oracle(oracle, ks, vs)
    root, nodes = o.root_hash(), o.reachable()
    some = r.sample(ks, 12)
    wit = {root: nodes[root]}
    for k in some:
        wit.update({P.kec(e): e for e in P.expected_proof(nodes, root, k)[0]})
    t = ResidentTrie.from_witness(Ctx(0), root, wit, emit=False)
    assert t.stubs > 0
    seen = set()
    for a, b, mx in RC.random_ranges(r, ks, 200) + [(k, k, 1) for k in some]:
        want = RR.expected_range(wit, root, a, b, mx)
        assert _page(lambda: t.range(a, b, mx)) == want, (a and a.hex(), b and b.hex(), mx)
        seen.add(want[0])
    assert seen == {"page", "missing"}
    t.close()
    # the fetch loop
    t = ResidentTrie.from_witness(Ctx(0), root, {root: nodes[root]}, emit=False)
    got, origin, fetched = [], None, 0
    while True:
        try:
            keys, vals, more, nxt = t.range(origin, None, 16)
        except _lib.MPTNodeMissingException as e:
            assert e.missing in nodes and e.missing not in (root,)
            assert t.fill({e.missing: nodes[e.missing]}) >= 1
            fetched += 1
            continue
        got += list(zip(keys, vals))
        if not more:
            break
        origin = nxt
    assert fetched >= 1 and got == list(zip(ks, vs)) and t.stubs == 0
    t.close()


@pytest.mark.parametrize("hashed", [False, True], ids=["raw", "hashed"])
def test_range_proof(khst, oracle, hashed):
    """range_proof: the page plus the proofs of origin and of the last returned key (or limit), over
    trie keys -- on a hashed handle KH_PROVE_TRIE_KEYS keeps them from being hashed again."""
    from khipu_amd.device import Ctx, ResidentTrie, verify_proofs
    r = random.Random(61)
    raw = [bytes(r.getrandbits(8) for _ in range(20 if hashed else 32)) for _ in range(300)]
    vs = [C.account_value(r) for _ in raw]
    tk = [oracle.kec256(k) for k in raw] if hashed else raw
    o = _oracle(oracle, tk, vs)
    root, nodes = o.root_hash(), o.reachable()
    snap = RR.Snapshot(nodes, root)
    t = ResidentTrie(Ctx(0), raw, vs, hash_keys=hashed, emit=False)
    for a, b, mx in [(None, None, 10), (snap.keys[40], snap.keys[80], 1000), (RC._step(snap.keys[5], 1), None, 7),
                     (RC._step(snap.keys[299], 1), None, 7), (snap.keys[9], snap.keys[9], 3)]:
        keys, vals, more, nxt, table = t.range_proof(a, b, mx)
        assert ("page", keys, vals, more, nxt) == snap.expected_range(a, b, mx)
        ends = [a or RC.ZERO, keys[-1] if keys else (b or RC.FF)]
        want = [P.expected_proof(nodes, root, k) for k in ends]
        assert table.proofs() == [p for p, _ in want]
        assert sorted(table.nodes) == sorted({e for p, _ in want for e in p})
        st, got = verify_proofs(root, ends, table)
        assert got == [v for _, v in want] and st == [int(v is not None) for v in got]
    t.close()


def test_range_through_the_jni_shim(khst, oracle, tmp_path):
    """range through the in-process JNIEnv of tests/jni_stub: 400 keys, ranges paged to their end by
    `next` with a value array that starts empty, so the grow path runs."""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    stub = os.path.join(ROOT, "tests", "jni_stub")
    exe = tmp_path / "jni_range_driver"
    rc = subprocess.run([cc, "-std=gnu99", "-O1", "-Wall", "-Werror", "-I", stub, "-I", os.path.join(ROOT, "include"),
                         "-o", str(exe), os.path.join(stub, "jni_range_driver.c"), os.path.join(stub, "fake_env.c"),
                         os.path.join(ROOT, "jni", "khst_jni.c"), "-L", os.path.join(ROOT, "khipu_amd"), "-lkhst",
                         "-Wl,-rpath," + os.path.join(ROOT, "khipu_amd"), "-Wl,-rpath-link,/opt/rocm/lib"],
                        capture_output=True, text=True)
    assert rc.returncode == 0, rc.stderr
    rnd = random.Random(808)
    keys = [C._rk(rnd) for _ in range(400)]
    vals = [C.account_value(rnd) if i % 3 else C.storage_value(rnd) for i in range(len(keys))]
    voff = np.zeros(len(vals) + 1, np.uint64)
    voff[1:] = np.cumsum([len(v) for v in vals])
    srt = sorted(keys)
    q = [(RC.ZERO, RC.FF, 64), (srt[100], srt[180], 7), (RC._step(srt[10], 1), srt[12], 1), (srt[399], RC.FF, 5),
         (RC.FF, RC.ZERO, 5)]
    p = tmp_path / "in.bin"
    with open(p, "wb") as f:
        f.write(np.uint32(32).tobytes() + np.uint64(len(keys)).tobytes())
        f.write(b"".join(keys) + voff.tobytes() + b"".join(vals))
        f.write(np.uint64(len(q)).tobytes() + b"".join(a + b + np.uint64(mx).tobytes() for a, b, mx in q))
    rc = subprocess.run([str(exe), str(p)], capture_output=True, text=True, timeout=120)
    assert rc.returncode == 0, rc.stderr
    lines = [ln.split() for ln in rc.stdout.split("\n")[:-1]]
    assert lines[-1] == ["E", "0"], lines[-1]
    o = _oracle(oracle, keys, vals)
    snap = RR.Snapshot(o.reachable(), o.root_hash())
    for j, (a, b, mx) in enumerate(q):
        got = [(bytes.fromhex(x[2]), b"" if x[3] == "-" else bytes.fromhex(x[3])) for x in lines
               if x[0] == "K" and x[1] == str(j)]
        want = [(k, v) for k, v in snap.items if a <= k <= b]
        assert got == want, j
        _, n, pages, grows = [x for x in lines if x[0] == "Q" and x[1] == str(j)][0][1:]
        assert int(n) == len(want) and int(pages) >= max(1, -(-len(want) // mx))
        assert int(grows) >= (1 if want else 0)
