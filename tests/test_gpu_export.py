"""GPU: a resident handle's nodes read back out -- kh_trie_export_nodes (the node store of the
current version, re-encoded from the records, in chunks) and kh_trie_nodes_by_hash
(getMptNodeByHash) -- bit-exact against the oracle's reachable(): every node reachable from the
root with an encoding >= 32 B, plus the root."""
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

from tests import cases as C
from tests import export_cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMPTY = bytes.fromhex("56e81f171bcc55a6ff8345e692c0f86e5b48e01b996cadc001622fb5e363b421")


def _oracle(oracle, ks, vs):
    o = oracle.Trie()
    for k, v in zip(ks, vs):
        o.put(k, v)
    return o


def _want(o):
    return o.reachable() if o.root_hash() != EMPTY else {}


def _fold(o, ups, dels):
    for k, v in ups:
        o.put(k, v)
    for k in dels:
        o.remove(k)


@pytest.mark.parametrize("i", range(len(C.commit_scenarios())), ids=[s[0] for s in C.commit_scenarios()])
def test_export_after_commits(khst, oracle, i):
    """The exported node set after the open and after every batch of every commit scenario, with
    and without KH_EMIT_NODES on the handle, every encoding re-hashed on the device (verify)."""
    from khipu_amd.device import Ctx, ResidentTrie
    name, ks, vs, batches = C.commit_scenarios()[i]
    o = _oracle(oracle, ks, vs)
    t = ResidentTrie(Ctx(0), ks, vs, emit=i % 2 == 0)
    for b in range(len(batches) + 1):
        if b:
            _fold(o, *batches[b - 1])
            assert t.commit(*batches[b - 1]) == o.root_hash(), (name, b)
        pairs = list(t.export_nodes(verify=True))
        got = dict(pairs)
        assert got == _want(o), (name, b)
        if name in ("accounts", "storage", "large_batch", "same_key_batch"):  # random keys: no node twice
            assert len(pairs) == len(got), (name, b)
    t.close()


def test_export_embedded_nodes(khst, oracle):
    """Leaves embedded in depth-63 branches embedded in depth-62 branches: children written
    verbatim, and none of them exported on its own."""
    from khipu_amd.device import Ctx, ResidentTrie
    ks, vs = export_cases.embedded_case()
    want = _oracle(oracle, ks, vs).reachable()
    assert export_cases.holds_embedded_child(want)
    t = ResidentTrie(Ctx(0), ks, vs, emit=False)
    pairs = list(t.export_nodes(verify=True))
    assert dict(pairs) == want and len(pairs) == len(want)
    t.close()


@pytest.mark.parametrize("small", [False, True], ids=["hashed", "inline"])
def test_export_value_only_branch(khst, oracle, small):
    """khipu's value-only branch (forest.h VB_DEPTH), made by a re-put under a depth-63 branch:
    as a hashed node and embedded in its parent; under an extension once its sibling is gone."""
    from khipu_amd.device import Ctx, ResidentTrie
    r = random.Random(64 if small else 63)
    val = (lambda: bytes([r.randrange(1, 0x80)])) if small else (lambda: C.account_value(r))

    def pair():
        k1 = bytearray(C._rk(r))
        k2 = bytearray(k1)
        k2[31] ^= 0x01
        return bytes(k1), bytes(k2)
    k1, k2 = pair()
    k3 = bytearray(k1)
    k3[31] = (k3[31] & 0x0F) | (((k3[31] >> 4) ^ 0x3) << 4)
    k3 = bytes(k3)
    q1, q2 = pair()
    others = [C._rk(r) for _ in range(300)]
    ks = others + [k1, k2, q1, q2]
    vs = [val() for _ in ks]
    o = _oracle(oracle, ks, vs)
    t = ResidentTrie(Ctx(0), ks, vs, emit=False)
    blocks = [([(k1, val()), (others[0], val()), (q1, val())], []),
              ([(k1, val())], [others[1]]),
              ([(others[3], val())], [k2]),
              ([(k3, val())], []),
              ([(k1, val()), (q1, val())], [others[4]]),
              ([], [k3])]
    for b, (ups, dels) in enumerate(blocks):
        _fold(o, ups, dels)
        assert t.commit(ups, dels) == o.root_hash(), b
        assert dict(t.export_nodes(verify=True)) == o.reachable(), b
    t.close()


def test_export_chunking_and_cursor(khst, oracle):
    """Small buffers: many calls whose union is the node set; a buffer the next record does not
    fit reports what it needs; a cursor does not survive a commit, a rollback or a compaction."""
    from khipu_amd import _lib
    from khipu_amd.device import Ctx, ResidentTrie
    r = random.Random(404)
    ks = [C._rk(r) for _ in range(2000)]
    vs = [C.account_value(r) for _ in ks]
    want = _oracle(oracle, ks, vs).reachable()
    t = ResidentTrie(Ctx(0), ks, vs, emit=False)
    cur, got, calls, done = t.export_cursor(), [], 0, False
    while not done:
        pairs, done = t.export_chunk(cur, node_cap=3, rlp_cap=700)
        assert len(pairs) <= 3 and sum(len(e) for _, e in pairs) <= 700
        got += pairs
        calls += 1
        assert calls < 10 * len(want)
    assert calls >= len(want) // 3 and calls > 100 and dict(got) == want and len(got) == len(want)
    # not even the next record fits: sizes reported, cursor unchanged, and those sizes succeed
    cur = t.export_cursor()
    with pytest.raises(_lib.KhError) as ei:
        t.export_chunk(cur, node_cap=3, rlp_cap=10)
    assert ei.value.code == _lib.KH_ENOSPC and (cur.next, cur.epoch) == (0, 0)
    nn, nb = ei.value.needed
    assert 1 <= nn <= 2 and nb > 10
    pairs, _ = t.export_chunk(cur, node_cap=nn, rlp_cap=nb)
    assert len(pairs) == nn and sum(len(e) for _, e in pairs) == nb and all(want[h] == e for h, e in pairs)
    # a cursor held across a commit / a rollback / a compaction
    t.commit([(ks[0], C.account_value(r))], [])
    with pytest.raises(_lib.MPTException):
        t.export_chunk(cur, node_cap=3, rlp_cap=700)
    t.savepoint()
    t.commit([(ks[1], C.account_value(r))], [])
    cur = t.export_cursor()
    t.export_chunk(cur, node_cap=3, rlp_cap=700)
    t.rollback()
    with pytest.raises(_lib.MPTException):
        t.export_chunk(cur, node_cap=3, rlp_cap=700)
    cur = t.export_cursor()
    t.export_chunk(cur, node_cap=3, rlp_cap=700)
    t.compact()
    with pytest.raises(_lib.MPTException):
        t.export_chunk(cur, node_cap=3, rlp_cap=700)
    # release keeps a cursor: it changes no record
    t.savepoint()
    cur = t.export_cursor()
    t.export_chunk(cur, node_cap=3, rlp_cap=700)
    t.release()
    t.export_chunk(cur, node_cap=3, rlp_cap=700)
    t.close()


def _forest(khst, oracle):
    """60 tries over 8 blocks (the shape of test_forest_vs_oracle), hashed keys; the same slot and
    value alone in two further tries (one node, two roots)."""
    from khipu_amd.device import Ctx, ResidentForest
    r = random.Random(78)
    f = ResidentForest(Ctx(0), hash_keys=True, emit=False)
    tries = {}
    ids = [r.randrange(1 << 32) for _ in range(60)]
    twins = [r.randrange(1 << 32) for _ in range(2)]
    for blk in range(8):
        ups, dels = [], []
        for t in r.sample(ids, 25):
            live = getattr(tries.get(t), "_live", [])
            for _ in range(r.choice([1, 3, 10, 40])):
                slot = bytes(r.getrandbits(8) for _ in range(32)) if not live or r.random() < 0.6 else r.choice(live)
                ups.append((t, slot, C.storage_value(r)))
            if live and r.random() < 0.5:
                for slot in r.sample(live, min(len(live), r.choice([1, 5, len(live)]))):
                    dels.append((t, slot))
        if blk == 2:
            ups += [(twins[0], b"\x11" * 32, b"\x01" * 40), (twins[1], b"\x11" * 32, b"\x01" * 40)]
        got = f.commit(ups, dels)
        for t, slot, v in ups:
            o = tries.setdefault(t, oracle.Trie())
            o.put(oracle.kec256(slot), v)
            o._live = list(dict.fromkeys(getattr(o, "_live", []) + [slot]))
        for t, slot in dels:
            tries[t].remove(oracle.kec256(slot))
            tries[t]._live = [s for s in tries[t]._live if s != slot]
        for t in got:
            assert got[t] == tries[t].root_hash(), (blk, t)
    return f, tries, twins


def test_export_forest(khst, oracle):
    f, tries, twins = _forest(khst, oracle)
    want = {}
    for o in tries.values():
        want.update(_want(o))
    pairs = list(f.export_nodes(verify=True))
    assert dict(pairs) == want
    twin_root = tries[twins[0]].root_hash()
    assert tries[twins[1]].root_hash() == twin_root
    assert sum(1 for h, _ in pairs if h == twin_root) == 2  # both roots
    full = [t for t, o in tries.items() if len(_want(o)) > 3]
    for t in (full[0], full[-1], twins[1]):
        assert dict(f.export_nodes(trie=t, verify=True)) == tries[t].reachable(), t
    assert list(f.export_nodes(trie=0x7FFFFFFF)) == []
    # by hash through the forest: every node, the shared one, an absent one
    hs = list(want)[:3000] + [twin_root, b"\x42" * 32]
    got = f.nodes_by_hash(hs)
    assert got[:-1] == [want[h] for h in hs[:-1]] and got[-1] is None
    f.close()


def test_export_empty(khst):
    from khipu_amd.device import Ctx, ResidentForest, ResidentTrie
    t = ResidentTrie(Ctx(0), [], [], emit=False)
    pairs, done = t.export_chunk(t.export_cursor(), node_cap=0, rlp_cap=0)
    assert pairs == [] and done
    assert t.checkpoint() == (EMPTY, {}) and t.nodes_by_hash([EMPTY]) == [None]
    f = ResidentForest(Ctx(0))
    assert list(f.export_nodes()) == [] and f.nodes_by_hash([b"\x01" * 32]) == [None]
    t.close()
    f.close()


@pytest.mark.parametrize("hash_keys", [False, True], ids=["raw", "hashed"])
def test_checkpoint_round_trip(khst, oracle, hash_keys):
    """checkpoint() after three commits with deletes feeds from_nodes: the same root, the same
    answers, and a further commit on the reopened trie matches the oracle."""
    from khipu_amd.device import Ctx, ResidentTrie
    r = random.Random(606)
    klen = 20 if hash_keys else 32
    tk = (lambda k: oracle.kec256(k)) if hash_keys else (lambda k: k)
    ks = [bytes(r.getrandbits(8) for _ in range(klen)) for _ in range(1500)]
    live = {k: C.account_value(r) for k in ks}
    o = _oracle(oracle, [tk(k) for k in live], live.values())
    ctx = Ctx(0)
    t = ResidentTrie(ctx, list(live), list(live.values()), hash_keys=hash_keys, emit=False)
    for _ in range(3):
        ups = [(k, C.account_value(r)) for k in r.sample(list(live), 40)]
        ups += [(bytes(r.getrandbits(8) for _ in range(klen)), C.account_value(r)) for _ in range(20)]
        dels = r.sample([k for k in live if k not in dict(ups)], 60)
        _fold(o, [(tk(k), v) for k, v in ups], [tk(k) for k in dels])
        live.update(ups)
        for k in dels:
            del live[k]
        assert t.commit(ups, dels) == o.root_hash()
    root, nodes = t.checkpoint(verify=True)
    assert root == o.root_hash() and nodes == o.reachable()
    t2 = ResidentTrie.from_nodes(ctx, root, nodes, hash_keys=hash_keys, emit=False)
    assert t2.root == root and len(t2) == len(live)
    probe = r.sample(list(live), 50) + dels[:10]
    assert t2.get(probe) == [live.get(k) for k in probe]
    k, v = next(iter(live)), C.account_value(r)
    o.put(tk(k), v)
    assert t2.commit([(k, v)], []) == o.root_hash()
    t2.close()
    t.close()


def test_nodes_by_hash(khst, oracle):
    """One call: every reachable hash (more than one LDS table's worth), absent hashes, a repeated
    hash and the previous version's root; then across a savepoint and its rollback."""
    from khipu_amd import _lib
    from khipu_amd.device import Ctx, ResidentTrie
    r = random.Random(707)
    ks = [C._rk(r) for _ in range(2000)]
    vs = [C.account_value(r) for _ in ks]
    o = _oracle(oracle, ks, vs)
    t = ResidentTrie(Ctx(0), ks, vs, emit=False)
    for _ in range(2):
        old_root = t.root
        ups = [(k, C.account_value(r)) for k in r.sample(ks, 30)] + [(C._rk(r), C.account_value(r)) for _ in range(10)]
        _fold(o, ups, [])
        assert t.commit(ups, []) == o.root_hash()
    want = o.reachable()
    present = list(want)
    assert 2048 < len(present) < 4000
    absent = [C._rk(r) for _ in range(50)]
    hs = present + absent + [present[7], old_root]
    got = t.nodes_by_hash(hs)
    assert got[:len(present)] == [want[h] for h in present]
    assert got[len(present):len(present) + 50] == [None] * 50
    assert got[-2] == want[present[7]] and got[-1] is None
    # savepoint, commit: the new root is found; rollback: the earlier root again, the new one not
    root0 = t.root
    t.savepoint()
    k, v = ks[3], C.account_value(r)
    root1 = t.commit([(k, v)], [])
    assert root1 != root0
    a, b = t.nodes_by_hash([root1, root0])
    assert a is not None and oracle.kec256(a) == root1 and b is None
    t.rollback()
    a, b = t.nodes_by_hash([root1, root0])
    assert a is None and b == want[root0]
    assert t.nodes_by_hash([]) == []
    with pytest.raises(_lib.MPTException):
        t.nodes_by_hash([b"\x00" * 32] * 4097)
    assert t.nodes_by_hash([root0] * 4096) == [want[root0]] * 4096
    t.close()


def test_export_through_the_jni_shim(khst, oracle, tmp_path):
    """exportNodes (the cursor loop over small arrays, grown on -1) and nodesByHash through the
    in-process JNIEnv of tests/jni_stub."""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    stub = os.path.join(ROOT, "tests", "jni_stub")
    exe = tmp_path / "jni_export_driver"
    rc = subprocess.run([cc, "-std=gnu99", "-O1", "-Wall", "-Werror", "-I", stub, "-I", os.path.join(ROOT, "include"),
                         "-o", str(exe), os.path.join(stub, "jni_export_driver.c"), os.path.join(stub, "fake_env.c"),
                         os.path.join(ROOT, "jni", "khst_jni.c"), "-L", os.path.join(ROOT, "khipu_amd"), "-lkhst",
                         "-Wl,-rpath," + os.path.join(ROOT, "khipu_amd"), "-Wl,-rpath-link,/opt/rocm/lib"],
                        capture_output=True, text=True)
    assert rc.returncode == 0, rc.stderr
    rnd = random.Random(808)
    keys = [C._rk(rnd) for _ in range(400)]
    vals = [C.account_value(rnd) for _ in keys]
    voff = np.zeros(len(vals) + 1, np.uint64)
    voff[1:] = np.cumsum([len(v) for v in vals])
    p = tmp_path / "in.bin"
    with open(p, "wb") as f:
        f.write(np.uint32(32).tobytes() + np.uint64(len(keys)).tobytes())
        f.write(b"".join(keys) + voff.tobytes() + b"".join(vals))
    rc = subprocess.run([str(exe), str(p)], capture_output=True, text=True, timeout=120)
    assert rc.returncode == 0, rc.stderr
    lines = [ln.split() for ln in rc.stdout.split("\n")[:-1]]
    assert lines[-1] == ["E", "0"], lines[-1]
    want = _oracle(oracle, keys, vals).reachable()
    nodes = [(bytes.fromhex(x[1]), bytes.fromhex(x[2])) for x in lines if x[0] == "N"]
    assert dict(nodes) == want and len(nodes) == len(want)
    calls, grows = [(int(x[1]), int(x[2])) for x in lines if x[0] == "C"][0]
    assert grows >= 1 and calls > 10
    by = [(bytes.fromhex(x[1]), None if x[2] == "-" else bytes.fromhex(x[2])) for x in lines if x[0] == "B"]
    assert len(by) == 41 and all(e == want[h] for h, e in by[:40]) and by[40][1] is None
