"""GPU: range responses filled into partial handles (kh_trie_fill_ranges_host through
ResidentTrie.fill_range and ResidentForest.fill_ranges).  Every expectation is the oracle's
(oracle.Trie) or the model's (tests/fillrange_ref.py, which imports nothing of the library); the
pages are the library's own range_proof of a full handle; the shapes (tests/fillrange_cases.py) are
the smallest at which each path can go wrong."""
import random

import pytest

from tests import fillrange_cases as FC
from tests import fillrange_ref as F
from tests import proof_ref as P

pytestmark = pytest.mark.gpu
OK, BAD_ORDER, MISSING, BAD_NODE, BAD_ROOT, INCOMPLETE = range(6)


def _trie(oracle, items):
    o = oracle.Trie()
    for k, v in items:
        o.put(k, v)
    return o


class Model:
    """The receiving handle as tests/fillrange_ref.py sees it."""

    def __init__(self, nodes, root, held=None):
        self.nodes, self.root, self.held = nodes, root, set(held) if held else {root}

    def fill(self, encs):
        self.held = F.fill_nodes(self.nodes, self.root, self.held, encs)

    def page(self, origin, keys, vals):
        res = F.fill_range(self.nodes, self.root, self.held, origin, keys, vals)
        if res.status == OK:
            self.held = res.held
        return res

    @property
    def stubs(self):
        return len(F.stubs(self.nodes, self.root, self.held))

    def __len__(self):
        return F.keys_held(self.nodes, self.root, self.held)


@pytest.fixture(scope="module")
def crafted(oracle):
    items = FC.crafted()
    o = _trie(oracle, items)
    return dict(items=items, nodes=o.reachable(), root=o.root_hash())


def _snapshot(t):
    return list(t.export_nodes()), t.get_root(), t.stubs, len(t), t.nodes()


def test_two_leaves_from_a_root_only_handle(khst, oracle):
    from khipu_amd.device import Ctx, ResidentTrie
    A, B = b"\x11" + b"\xaa" * 31, b"\x52" + b"\xbb" * 31  # (the `two` fixture of tests/test_gpu_partial.py)
    vA, vB = b"a" * 40, b"b" * 44
    o = _trie(oracle, [(A, vA), (B, vB)])
    nodes, root = o.reachable(), o.root_hash()
    t = ResidentTrie.from_witness(Ctx(0), root, {root: nodes[root]})
    assert t.stubs == 2 and len(t) == 0
    # the proof of [0, B] is the root and leaf B: stub A is left, inside the span
    proof = P.expected_proof(nodes, root, FC.ZERO)[0] + P.expected_proof(nodes, root, B)[0]
    t.fill(proof)
    assert t.stubs == 1 and len(t) == 1
    assert t.fill_range(None, ([A, B], [vA, vB])) == ([OK], [0], {"keys": 1, "stubs": 1})
    assert t.stubs == 0 and len(t) == 2 and t.get_root() == root
    assert dict(t.export_nodes(verify=True)) == nodes
    assert set(t.nodes()) == set(nodes) - {root, P.kec(proof[-1])}  # leaf A alone is new to the handle
    t.close()


@pytest.mark.parametrize("size", FC.PAGES)
def test_walk_from_a_root_only_handle(khst, oracle, crafted, size):
    """Pages of `size` served by a full handle, first from the origin inside the extension (its
    proof leaves a STUB_BRANCH stub inside the span), then from zero until the trie is whole."""
    from khipu_amd.device import Ctx, ResidentTrie
    items, nodes, root = crafted["items"], crafted["nodes"], crafted["root"]
    ctx = Ctx(0)
    S = ResidentTrie(ctx, [k for k, _ in items], [v for _, v in items])
    assert S.root == root
    t = ResidentTrie.from_witness(ctx, root, {root: nodes[root]})
    m = Model(nodes, root)
    origin, phase, pages = FC.EXT_ORIGIN, 0, 0
    while True:
        keys, vals, more, _, table = S.range_proof(origin, None, size)
        t.fill(table)
        m.fill(table.nodes)
        assert (t.stubs, len(t)) == (m.stubs, len(m))
        before = dict(t.export_nodes())
        want = m.page(origin, keys, vals)
        st, left, cnt = t.fill_range(origin, (keys, vals))
        assert (st, left, cnt) == ([OK], [m.stubs], {"keys": want.n_keys, "stubs": want.n_stubs}), (pages, origin.hex())
        assert t.get_root() == root and (t.stubs, len(t)) == (m.stubs, len(m))
        after = dict(t.export_nodes())
        assert set(after) == m.held
        assert t.nodes() == {h: e for h, e in after.items() if h not in before}  # the write-back set
        pages += 1
        if more and left[0]:
            origin = FC.step(keys[-1])
        elif phase == 0:
            origin, phase = FC.ZERO, 1
        else:
            break
        assert pages < 200
    assert t.stubs == 0 and len(t) == len(items)
    assert dict(t.export_nodes(verify=True)) == nodes
    assert t.get([k for k, _ in items]) == [v for _, v in items]
    # the synced trie commits like any other
    o = _trie(oracle, items)
    up, gone = items[len(items) // 2][0], items[len(items) // 3][0]
    o.put(up, b"\x2a" * 50)
    o.remove(gone)
    assert t.commit({up: b"\x2a" * 50}, [gone]) == o.root_hash()
    t.close()
    S.close()


def test_refusals_leave_the_handle_as_it_was(khst, oracle, crafted):
    from khipu_amd.device import Ctx, ResidentTrie
    items, nodes, root = crafted["items"], crafted["nodes"], crafted["root"]
    ctx = Ctx(0)
    keys, vals, proof, _ = FC.page(items, nodes, root, FC.ZERO, 64)
    # MISSING: the range without its proof runs into the root-only handle's stub
    t0 = ResidentTrie.from_witness(ctx, root, {root: nodes[root]})
    snap0 = _snapshot(t0)
    want = F.fill_range(nodes, root, {root}, FC.ZERO, keys, vals)
    assert want.status == MISSING
    assert t0.fill_range(None, (keys, vals))[0] == [MISSING]
    assert set(t0.missing()) == {(0, h) for h in want.missing}
    assert _snapshot(t0) == snap0
    t0.close()
    # the rest on a handle that holds the page's boundary proofs
    t = ResidentTrie.from_witness(ctx, root, {root: nodes[root]})
    m = Model(nodes, root)
    t.fill(proof)
    m.fill(proof)
    snap = _snapshot(t)
    assert snap[2] == m.stubs and snap[3] == len(m)
    zero = [0] * 64
    ins = [p for p, _ in F.stubs(nodes, root, m.held) if F.inside(p, zero, P.nibbles(keys[-1]))]
    under = {tuple(p): [k for k in keys if P.nibbles(k)[:len(p)] == p] for p in ins}
    big = next(ks for ks in under.values() if len(ks) >= 2)
    drop = lambda gone: ([k for k in keys if k not in gone], [v for k, v in zip(keys, vals) if k not in gone])
    j = keys.index(big[0])
    flipped = bytearray(vals[j])
    flipped[-1] ^= 0x10
    absent = FC.step(keys[j])
    assert absent not in dict(items) and absent < keys[j + 1]
    assert F._walk_key(nodes, root, m.held, P.nibbles(keys[-1]))[0] == "leaf"  # the proof brought the last leaf
    cases = [
        ("one key of an inside stub omitted", FC.ZERO, *drop(big[:1]), BAD_ROOT),
        ("every key of an inside stub omitted", FC.ZERO, *drop(big), BAD_ROOT),
        ("a value changed by one byte", FC.ZERO, keys, vals[:j] + [bytes(flipped)] + vals[j + 1:], BAD_ROOT),
        ("an invented key", FC.ZERO, keys[:j + 1] + [absent] + keys[j + 1:],
         vals[:j + 1] + [b"\x07" * 33] + vals[j + 1:], BAD_ROOT),
        ("a resident leaf re-delivered with another value", FC.ZERO, keys, vals[:-1] + [vals[-1] + b"\x01"], BAD_ROOT),
        ("keys out of order", FC.ZERO, keys[:j] + [keys[j + 1], keys[j]] + keys[j + 2:], vals, BAD_ORDER),
        ("an empty value", FC.ZERO, keys, vals[:j] + [b""] + vals[j + 1:], BAD_ORDER),
        ("a first key below the origin", FC.step(keys[0]), keys, vals, BAD_ORDER),
        ("no entries, stubs at or after the origin", FC.ZERO, [], [], INCOMPLETE),
    ]
    for what, origin, ks, vs, status in cases:
        assert F.fill_range(nodes, root, m.held, origin, ks, vs).status == status, what
        assert t.fill_range(origin, (ks, vs)) == ([status], [snap[2]], {"keys": 0, "stubs": 0}), what
        assert _snapshot(t) == snap, what
    # a savepoint open: KH_EINVAL, as for kh_trie_fill_nodes
    t.savepoint()
    with pytest.raises(khst.MPTException) as e:
        t.fill_range(None, (keys, vals))
    assert e.value.code == -1
    t.rollback()
    assert _snapshot(t) == snap
    # the honest page, then the same page again: OK with nothing to gain
    want = m.page(FC.ZERO, keys, vals)
    assert t.fill_range(None, (keys, vals)) == ([OK], [m.stubs], {"keys": want.n_keys, "stubs": want.n_stubs})
    done = _snapshot(t)
    assert t.fill_range(None, (keys, vals)) == ([OK], [m.stubs], {"keys": 0, "stubs": 0})
    assert _snapshot(t)[:4] == done[:4] and t.nodes() == {}
    t.close()


def test_forest_many_ranges_in_one_call(khst, oracle, crafted):
    from khipu_amd.device import Ctx, ResidentForest
    items, nodes, root = crafted["items"], crafted["nodes"], crafted["root"]
    r = random.Random(11)
    rk = lambda: bytes(r.getrandbits(8) for _ in range(32))
    slots = sorted((rk(), bytes(r.getrandbits(8) for _ in range(r.choice((1, 33))))) for _ in range(10))
    one = [(rk(), b"\x05")]
    kept = {1: sorted((rk(), b"v" * 40) for _ in range(5)), 2: sorted((rk(), b"\x09") for _ in range(20))}
    roots = {t: _trie(oracle, kv).root_hash() for t, kv in kept.items()}
    BIG, MID, EMPTY_ID, TAIL = (1 << 31) + 5, 70000, 11, 7  # (ids past the trie-id bits the handle has sorted so far)
    # trie 7: the crafted trie, synced up to its last page of 64 by the model
    origins = FC.walk_origins(items, 64)
    m = Model(nodes, root)
    for o in origins[:-1]:
        ks, vs, proof, _ = FC.page(items, nodes, root, o, 64)
        m.fill(proof)
        assert m.page(o, ks, vs).status == OK
    tk, tv, tproof, more = FC.page(items, nodes, root, origins[-1], 64)
    assert tk and not more and m.stubs > 0
    ctx = Ctx(0)
    Fo = ResidentForest(ctx, emit=True)
    assert Fo.commit([(t, k, v) for t, kv in kept.items() for k, v in kv]) == roots
    Fo.load_partial({TAIL: root}, {h: nodes[h] for h in m.held})
    assert Fo.stubs == m.stubs and len(Fo) == 25 + len(m)
    m.fill(tproof)
    want = F.fill_range(nodes, root, m.held, origins[-1], tk, tv)
    assert want.status == OK and F.stubs(nodes, root, want.held) == []
    w_root, o_root = _trie(oracle, slots).root_hash(), _trie(oracle, one).root_hash()
    assert F.whole(w_root, *zip(*slots)) == OK
    pair = lambda kv: ([k for k, _ in kv], [v for _, v in kv])
    good = [(BIG, w_root, None, pair(slots)), (MID, o_root, None, pair(one)), (TAIL, root, origins[-1], (tk, tv)),
            (EMPTY_ID, P.EMPTY_ROOT, None, ([], []))]
    bad = (9, w_root, None, pair(slots[:-1]))  # a whole trie with its last slot left out
    Fo.fill(tproof)
    snap = ({t: list(Fo.export_nodes(trie=t)) for t in (1, 2, TAIL)}, Fo.roots(), Fo.stubs, len(Fo), Fo.nodes(),
            Fo.last_roots())
    st, _, cnt = Fo.fill_ranges(good + [bad])
    assert st == [OK, OK, OK, OK, BAD_ROOT] and cnt == {"keys": 0, "stubs": 0}
    assert ({t: list(Fo.export_nodes(trie=t)) for t in (1, 2, TAIL)}, Fo.roots(), Fo.stubs, len(Fo), Fo.nodes(),
            Fo.last_roots()) == snap
    with pytest.raises(khst.MPTException) as e:  # a trie id listed twice
        Fo.fill_ranges(good + [good[0]])
    assert e.value.code == -1
    # the retry without the bad range
    st, left, cnt = Fo.fill_ranges(good)
    assert (st, left) == ([OK] * 4, [0] * 4) and cnt == {"keys": 11 + want.n_keys, "stubs": want.n_stubs}
    assert Fo.stubs == 0 and len(Fo) == 25 + 11 + len(items)
    assert Fo.roots() == {**roots, TAIL: root, BIG: w_root, MID: o_root}
    assert Fo.last_roots() == {TAIL: root, BIG: w_root, MID: o_root, EMPTY_ID: P.EMPTY_ROOT}
    for t in (1, 2):  # the tries the call did not name
        assert list(Fo.export_nodes(trie=t)) == snap[0][t]
    assert dict(Fo.export_nodes(trie=TAIL, verify=True)) == nodes
    assert dict(Fo.export_nodes(trie=BIG, verify=True)) == _trie(oracle, slots).reachable()
    assert dict(Fo.export_nodes(trie=MID, verify=True)) == _trie(oracle, one).reachable()
    new = {**_trie(oracle, slots).reachable(), **_trie(oracle, one).reachable(),
           **{h: nodes[h] for h in want.held - m.held}}
    assert Fo.nodes() == new  # whole tries with their root nodes, and the tail's new nodes
    assert Fo.get([(BIG, slots[3][0]), (MID, one[0][0]), (TAIL, tk[-1]), (2, kept[2][0][0])]) == \
        [slots[3][1], one[0][1], tv[-1], kept[2][0][1]]
    Fo.close()


def test_hashed_key_handle_takes_trie_keys(khst, oracle):
    from khipu_amd.device import Ctx, ResidentTrie
    r = random.Random(3)
    addrs = [bytes(r.getrandbits(8) for _ in range(20)) for _ in range(40)]
    vals = [bytes(r.getrandbits(8) for _ in range(r.choice((1, 40, 70)))) for _ in addrs]
    ctx = Ctx(0)
    S = ResidentTrie(ctx, addrs, vals, hash_keys=True)
    root = S.root
    t = ResidentTrie.from_witness(ctx, root, {root: dict(S.export_nodes())[root]}, hash_keys=True)
    origin, left = FC.ZERO, [1]
    while left[0]:
        keys, vs, more, _, table = S.range_proof(origin, None, 16)
        assert sorted(keys) == keys and not set(keys) & set(addrs)  # trie keys: the kec256 values
        st, left, _ = t.fill_range(origin, (keys, vs), proof=table)
        assert st == [OK] and t.get_root() == root
        assert more or left == [0]
        origin = FC.step(keys[-1])
    assert len(t) == 40 and t.get(addrs) == vals
    assert dict(t.export_nodes(verify=True)) == dict(S.export_nodes())
    t.close()
    S.close()


def test_fill_through_the_jni_shim(khst, oracle, crafted, tmp_path):
    """fillRanges through the in-process JNIEnv of tests/jni_stub: a page with one key left out is
    refused and leaves the handle as it was, the honest page is taken."""
    import os
    import shutil
    import subprocess

    import numpy as np
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    root_dir = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    stub = os.path.join(root_dir, "tests", "jni_stub")
    exe = tmp_path / "jni_fillrange_driver"
    rc = subprocess.run([cc, "-std=gnu99", "-O1", "-Wall", "-Werror", "-I", stub, "-I", os.path.join(root_dir, "include"),
                         "-o", str(exe), os.path.join(stub, "jni_fillrange_driver.c"), os.path.join(stub, "fake_env.c"),
                         os.path.join(root_dir, "jni", "khst_jni.c"), "-L", os.path.join(root_dir, "khipu_amd"), "-lkhst",
                         "-Wl,-rpath," + os.path.join(root_dir, "khipu_amd"), "-Wl,-rpath-link,/opt/rocm/lib"],
                        capture_output=True, text=True)
    assert rc.returncode == 0, rc.stderr
    items, nodes, root = crafted["items"], crafted["nodes"], crafted["root"]
    origin = FC.step(items[20][0])
    keys, vals, proof, _ = FC.page(items, nodes, root, origin, 16)
    m = Model(nodes, root)
    m.fill(proof)
    j = next(j for j in range(1, 15) if F._walk_key(nodes, root, m.held, P.nibbles(keys[j]))[0] == "stub")
    bad = (keys[:j] + keys[j + 1:], vals[:j] + vals[j + 1:])
    assert F.fill_range(nodes, root, m.held, origin, *bad).status == BAD_ROOT
    stubs0, size0 = m.stubs, len(m)
    want = m.page(origin, keys, vals)
    encs = [nodes[root]] + proof

    def offs(xs):
        o = np.zeros(len(xs) + 1, np.uint64)
        o[1:] = np.cumsum([len(x) for x in xs])
        return o.tobytes()
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(root + origin + np.uint64(len(encs)).tobytes() + offs(encs) + b"".join(encs))
        for ks, vs in (bad, (keys, vals)):
            f.write(np.asarray([len(ks), sum(len(v) for v in vs)], np.uint64).tobytes())
            f.write(b"".join(ks) + b"".join(vs) + offs(vs))
    rc = subprocess.run([str(exe), str(tmp_path / "in.bin")], capture_output=True, text=True, timeout=120)
    assert rc.returncode == 0, rc.stderr
    lines = [ln.split() for ln in rc.stdout.split("\n")[:-1]]
    assert lines[0] == ["O", "1", "0", str(stubs0)]
    assert lines[1] == ["F", "1", str(BAD_ROOT), str(stubs0), "0", "0", "0", str(size0), str(stubs0)]
    assert lines[2] == ["F", "0", str(OK), str(m.stubs), str(want.n_keys), str(want.n_stubs), "0", str(len(m)),
                        str(m.stubs)]
    assert lines[3] == ["E", "0"]
