"""GPU: storage tries paged into a resident forest from a node store and out again --
kh_forest_load_nodes, kh_forest_roots, kh_forest_evict -- against forests built by commits and
against the oracle.  The shapes: 60 tries of 1-300 slots (one of them export_cases' embedded
nodes) and one of 20,000 slots, so that a round's frontier spans several waves and 256-thread
blocks and the walk takes more than four rounds."""
import ctypes
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

from tests import cases as C
from tests import export_cases
from tests import writeback as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMPTY = W.EMPTY_TRIE_HASH
BIG = 60


class World:
    """The reference, computed once and left unchanged: per trie id the final {key: value}, the
    oracle's root and reachable(); the two commits that build it (the second deletes)."""

    def __init__(self, oracle):
        r = random.Random(2024)
        self.oracle = oracle
        self.kv, self.first, self.second_del, self.second_up = {}, [], [], []
        sizes = [1, 2, 3, 17] + [r.randint(1, 300) for _ in range(56)] + [20000]
        for t, n in enumerate(sizes):
            if t == 7:
                ks, vs = export_cases.embedded_case()
            else:
                ks = [C._rk(r) for _ in range(n)]
                vs = [bytes([r.randrange(1, 0x80)]) if (t + i) % 5 == 0 else C.storage_value(r) for i in range(n)]
            kv = dict(zip(ks, vs))
            extra = [C._rk(r) for _ in range(min(n, 5))]  # put by the first commit, deleted by the second
            self.first += [(t, k, v) for k, v in kv.items()] + [(t, k, C.storage_value(r)) for k in extra]
            self.second_del += [(t, k) for k in extra]
            # ... which also rewrites a few values (not in trie 7: a re-put under its depth-63
            # branches makes khipu's value-only branch, which trie() below, built from puts of
            # distinct keys, would not have; test_value_only_branch_round_trip covers it)
            for k in ([] if t == 7 else ks[:3]):
                kv[k] = C.storage_value(r)
                self.second_up.append((t, k, kv[k]))
            self.kv[t] = kv
        self.ids = list(self.kv)
        self.want, self.roots = {}, {}
        for t in self.ids:
            o = self.trie(t)
            self.want[t] = o.reachable()
            self.roots[t] = o.root_hash()
        self.nkeys = sum(len(kv) for kv in self.kv.values())

    def trie(self, t):
        """A fresh oracle trie holding trie t's final keys, its log empty."""
        o = self.oracle.Trie()
        for k, v in self.kv[t].items():
            o.put(k, v)
        return o.persist().reopen()

    def store(self, ids):
        s = {}
        for t in ids:
            s.update(self.want[t])
        return s

    def build(self, ctx, ids=None, emit=False):
        """A forest holding tries `ids` built by commits (upserts, then deletes and rewrites)."""
        from khipu_amd.device import ResidentForest
        ids = set(self.ids if ids is None else ids)
        f = ResidentForest(ctx, emit=emit)
        f.commit([u for u in self.first if u[0] in ids])
        got = f.commit([u for u in self.second_up if u[0] in ids], [d for d in self.second_del if d[0] in ids])
        assert got == {t: self.roots[t] for t in ids}
        return f


@pytest.fixture(scope="module")
def world(oracle):
    return World(oracle)


def _snapshot(f, world, ids):
    u = f.usage()
    q = [(t, k) for t in list(ids)[:5] for k in list(world.kv[t])[:10]]
    return f.roots(), u["records"], u["live_records"], u["map_slots"], len(f), f.get(q)


def _queries(world, ids, r, absent=200):
    q = [(t, k) for t in ids for k in world.kv[t]]
    want = [world.kv[t][k] for t, k in q]
    miss = [(r.choice(list(ids)), C._rk(r)) for _ in range(absent)]
    return q + miss, want + [None] * absent


def _batch(world, r, ids, new_id=None):
    """One further block over tries `ids`: updates, inserts and deletes; (upserts, deletes)."""
    ups, dels = [], []
    for t in ids:
        ks = list(world.kv[t])
        ups += [(t, k, C.storage_value(r)) for k in ([] if t == 7 else ks[:4])]  # (7: see World)
        ups += [(t, C._rk(r), C.storage_value(r)) for _ in range(3)]
        if len(ks) > 6:
            dels += [(t, ks[-1]), (t, ks[-2])]
    if new_id is not None:
        ups += [(new_id, C._rk(r), C.storage_value(r)) for _ in range(4)]
    return ups, dels


def _fold(world, ups, dels, alias=None):
    """The oracle tries after the batch (alias: {forest id: world id whose content it holds})."""
    alias = alias or {}
    out = {}
    for t in sorted({u[0] for u in ups} | {d[0] for d in dels}):
        src = alias.get(t, t)
        out[t] = world.trie(src) if src in world.kv else world.oracle.Trie()
    for t, k, v in ups:
        out[t].put(k, v)
    for t, k in dels:
        out[t].remove(k)
    return out


def test_round_trip(khst, oracle, world):
    """checkpoint() of a forest built by commits (deletes included), from_nodes, and everything
    read back equals the original's and the oracle's; a further batch on both gives equal roots and
    the reloaded forest's write-back delta passes the write-back contract."""
    from khipu_amd.device import Ctx, ResidentForest
    ctx = Ctx(0)
    r = random.Random(1)
    A = world.build(ctx)
    roots, nodes = A.checkpoint()
    assert roots == world.roots and nodes == world.store(world.ids)
    B = ResidentForest.from_nodes(ctx, roots, nodes, emit=True)
    assert B.roots() == A.roots() == world.roots
    assert len(B) == len(A) == world.nkeys
    q, want = _queries(world, world.ids, r)
    assert B.get(q) == A.get(q) == want
    for t in world.ids:
        got = list(B.export_nodes(trie=t, verify=True))
        assert dict(got) == world.want[t] and len(got) == len(world.want[t]), t
    for t in (0, 7, 31, BIG):  # (A's nodes as a whole are `nodes`, compared above)
        assert dict(A.export_nodes(trie=t)) == world.want[t], t
    ups, dels = _batch(world, r, [0, 5, 7, 17], new_id=99)
    os_ = _fold(world, ups, dels)
    ra, rb = A.commit(ups, dels), B.commit(ups, dels)
    assert ra == rb == {t: o.root_hash() for t, o in os_.items()}
    W.check_delta(B.nodes(), list(os_.values()), nodes, "reloaded forest")
    # (the 20,000-slot trie in a commit of its own, compared by its root: the oracle's
    # reachable() of a trie this size, which check_delta calls, takes seconds)
    ups, dels = _batch(world, r, [BIG, 31])
    ra, rb = A.commit(ups, dels), B.commit(ups, dels)
    assert ra == rb == {t: o.root_hash() for t, o in _fold(world, ups, dels).items()}
    A.close()
    B.close()


@pytest.mark.parametrize("small", [False, True], ids=["hashed", "inline"])
def test_value_only_branch_round_trip(khst, oracle, small):
    """khipu's value-only branch (a re-put under a depth-63 branch), hashed and embedded in its
    parent: a forest holding one is checkpointed and loaded, after each block that reshapes it."""
    from khipu_amd.device import Ctx, ResidentForest
    from tests import proof_cases
    ctx = Ctx(0)
    ks, vs, blocks, (k1, _, _) = proof_cases.vb_case(small)
    o = oracle.Trie()
    for k, v in zip(ks, vs):
        o.put(k, v)
    A = ResidentForest(ctx)
    A.commit([(9, k, v) for k, v in zip(ks, vs)])
    for ups, dels in blocks[:4]:
        for k, v in ups:
            o.put(k, v)
        for k in dels:
            o.remove(k)
        assert A.commit([(9, k, v) for k, v in ups], [(9, k) for k in dels]) == {9: o.root_hash()}
        roots, nodes = A.checkpoint()
        B = ResidentForest.from_nodes(ctx, roots, nodes)
        assert B.roots() == {9: o.root_hash()} and len(B) == len(A)
        assert dict(B.export_nodes(verify=True)) == o.reachable()
        assert B.get([(9, k1), (9, ks[5])]) == [o.get(k1), o.get(ks[5])]
        B.close()
    A.close()


def test_load_beside_resident_tries(khst, oracle, world):
    """Tries 0-29 built by commits, 30-59 loaded beside them: the old ones untouched, one commit
    over old and loaded tries together, then ids that need more trie-id bits than any before."""
    from khipu_amd.device import Ctx
    ctx = Ctx(0)
    r = random.Random(2)
    old, new = list(range(30)), list(range(30, 60))
    F = world.build(ctx, old)
    before = {t: list(F.export_nodes(trie=t)) for t in old}
    F.load_nodes({t: world.roots[t] for t in new}, world.store(new))
    assert F.roots() == {t: world.roots[t] for t in old + new}
    assert len(F) == sum(len(world.kv[t]) for t in old + new)
    for t in old:  # (the same records in the same order)
        assert list(F.export_nodes(trie=t)) == before[t], t
    for t in new:
        assert dict(F.export_nodes(trie=t, verify=True)) == world.want[t], t
    q, want = _queries(world, old + new, r)
    assert F.get(q) == want
    ups, dels = _batch(world, r, [3, 7, 33, 58])
    assert F.commit(ups, dels) == {t: o.root_hash() for t, o in _fold(world, ups, dels).items()}
    # ids past the bits the handle's sort has used so far (the tid_bits redo path)
    hi = {70000: 1, (1 << 31) + 5: 2}
    F.load_nodes({t: world.roots[s] for t, s in hi.items()}, world.store(hi.values()))
    assert all(F.roots()[t] == world.roots[s] for t, s in hi.items())
    ups = [(t, C._rk(r), C.storage_value(r)) for t in hi for _ in range(3)]
    dels = [(t, next(iter(world.kv[s]))) for t, s in hi.items()]
    assert F.commit(ups, dels) == {t: o.root_hash() for t, o in _fold(world, ups, dels, hi).items()}
    assert dict(F.export_nodes(trie=12, verify=True)) == world.want[12]
    F.close()


def test_load_is_deterministic(khst, world):
    """The same load into two fresh forests, and into a third from the store in another order:
    the same records in the same order, so the same export sequence."""
    from khipu_amd.device import Ctx, ResidentForest
    ctx = Ctx(0)
    store = world.store(world.ids)
    encs = list(store.values())
    seqs = []
    for order in (encs, encs, random.Random(3).sample(encs, len(encs))):
        f = ResidentForest(ctx)
        f.load_nodes(world.roots, order)
        seqs.append(list(f.export_nodes()))
        f.close()
    assert seqs[0] == seqs[1] == seqs[2] and dict(seqs[0]) == store


def _depth2_node(world, t):
    """A node referenced by hash from a hash child of trie t's root, referenced nowhere else."""
    enc = world.want[t]
    root = enc[world.roots[t]]
    child = next(root[q:q + m] for l, q, m in export_cases._items(root)[:16] if not l and m == 32)
    grand = next(enc[child][q:q + m] for l, q, m in export_cases._items(enc[child])[:16] if not l and m == 32)
    assert sum(1 for e in world.store(world.ids).values() if grand in e) == 1
    return grand


def test_missing_nodes(khst, world):
    """KH_ENODE lists every missing reference of the round that met one, and the forest is as before."""
    from khipu_amd import _lib
    from khipu_amd.device import Ctx
    ctx = Ctx(0)
    F = world.build(ctx, range(10))
    snap = _snapshot(F, world, range(10))
    ids = [30, 31, 32, 33, 34, 35]
    store = world.store(ids)
    cut = {h: e for h, e in store.items() if h not in (world.roots[31], world.roots[34])}
    with pytest.raises(_lib.MPTNodeMissingException) as ei:
        F.load_nodes({t: world.roots[t] for t in ids}, cut)
    assert sorted(ei.value.missing) == [(31, world.roots[31]), (34, world.roots[34])]
    assert _snapshot(F, world, range(10)) == snap
    rc, nm, miss = F.load_nodes_raw(ids, [world.roots[t] for t in ids], list(cut.values()), miss_cap=1)
    assert rc == _lib.KH_ENODE and nm == 2 and len(miss) == 1
    assert miss[0] in [(1, world.roots[31]), (4, world.roots[34])]
    assert _snapshot(F, world, range(10)) == snap
    rc, nm, miss = F.load_nodes_raw(ids, [world.roots[t] for t in ids], list(cut.values()), miss_cap=0)
    assert rc == _lib.KH_ENODE and nm == 2 and miss == []
    # one node two rounds down (the rounds above it had written records: all of them gone again)
    grand = _depth2_node(world, BIG)
    big = world.store([BIG])
    with pytest.raises(_lib.MPTNodeMissingException) as ei:
        F.load_nodes({BIG: world.roots[BIG], 30: world.roots[30]},
                     {h: e for h, e in {**big, **store}.items() if h != grand})
    assert ei.value.missing == [(BIG, grand)]
    assert _snapshot(F, world, range(10)) == snap
    F.load_nodes({t: world.roots[t] for t in ids + [BIG]}, {**big, **store})  # the complete store loads
    assert F.roots() == {t: world.roots[t] for t in list(range(10)) + ids + [BIG]}
    assert dict(F.export_nodes(trie=BIG, verify=True)) == world.want[BIG]
    F.close()


def test_refusals_leave_the_forest_unchanged(khst, oracle, world):
    from khipu_amd import _lib
    from khipu_amd._lib import lib
    from khipu_amd.device import Ctx, ResidentTrie
    ctx = Ctx(0)
    F = world.build(ctx, range(10))
    snap = _snapshot(F, world, range(10))
    store = world.store(range(40, 44))
    with pytest.raises(_lib.MPTException):  # a resident id
        F.load_nodes({40: world.roots[40], 3: world.roots[3]}, {**store, **world.store([3])})
    assert _snapshot(F, world, range(10)) == snap
    rc, _, _ = F.load_nodes_raw([40, 41, 40], [world.roots[t] for t in (40, 41, 40)], list(store.values()))
    assert rc == _lib.KH_EINVAL  # a repeated id
    assert _snapshot(F, world, range(10)) == snap
    # a malformed node: a leaf whose path runs past nibble 64, as trie 41's root
    bad = bytes([0xF8, 34 + 41, 0xA1, 0x31]) + b"\x11" * 32 + bytes([0xA8]) + b"\x09" * 40
    with pytest.raises(_lib.MPTException):
        F.load_nodes({40: world.roots[40], 41: oracle.kec256(bad)}, list(store.values()) + [bad])
    assert _snapshot(F, world, range(10)) == snap
    # ... and a branch with a value at depth 0
    h = b"\xa0" + b"\x77" * 32
    bv = bytes([0xF8, 66 + 14 + 41]) + h + h + b"\x80" * 14 + bytes([0xA8]) + b"v" * 40
    with pytest.raises(_lib.MPTException):
        F.load_nodes({41: oracle.kec256(bv)}, [bv])
    assert _snapshot(F, world, range(10)) == snap
    F.load_nodes({42: EMPTY}, store)  # the empty trie's root: nothing to load, no error
    F.load_nodes({}, store)
    assert _snapshot(F, world, range(10)) == snap
    # a handle that is not a forest
    t = ResidentTrie(ctx, list(world.kv[2]), list(world.kv[2].values()), emit=False)
    ids = np.asarray([40], np.uint32)
    rb = np.frombuffer(world.roots[40], np.uint8).copy()
    n = ctypes.c_uint64()
    assert lib().kh_forest_load_nodes(t.h, ids.ctypes.data, rb.ctypes.data, 1, None, None, 0, None, None, 0,
                                      ctypes.byref(n), None) == _lib.KH_EINVAL
    assert lib().kh_forest_roots(t.h, None, None, 0, ctypes.byref(n)) == _lib.KH_EINVAL
    assert lib().kh_forest_evict(t.h, ids.ctypes.data, 1, ctypes.byref(n)) == _lib.KH_EINVAL
    assert t.get_root() == world.roots[2]
    t.close()
    F.load_nodes({t: world.roots[t] for t in range(40, 44)}, store)  # and the forest still loads
    assert F.roots() == {t: world.roots[t] for t in list(range(10)) + list(range(40, 44))}
    F.close()


@pytest.mark.parametrize("big", [False, True], ids=["journaled_inserts", "map_rebuilt"])
def test_load_under_a_savepoint_rolls_back(khst, world, big):
    """savepoint -> load -> commit on a loaded trie -> rollback: the loaded tries are not resident
    any more and the forest is the one of the savepoint; with a load that grows the anchor map the
    rollback is the map rebuild."""
    from khipu_amd.device import Ctx
    ctx = Ctx(0)
    r = random.Random(6)
    base = list(range(4, 14))
    F = world.build(ctx, base)
    pre = list(F.export_nodes())
    snap = _snapshot(F, world, base)
    # tries of 1, 2 and 3 keys: a dozen records, far from what makes the map grow; with the
    # 20,000-key trie it has to
    new = [0, 1, 2] + ([BIG] if big else [])
    F.savepoint()
    F.load_nodes({t: world.roots[t] for t in new}, world.store(new))
    assert (F.usage()["map_slots"] > snap[3]) == big
    assert F.roots() == {t: world.roots[t] for t in base + new}
    ups, dels = _batch(world, r, [1, 4])
    assert F.commit(ups, dels) == {t: o.root_hash() for t, o in _fold(world, ups, dels).items()}
    F.rollback()
    assert F.roots() == {t: world.roots[t] for t in base}
    k1, k4 = next(iter(world.kv[1])), next(iter(world.kv[4]))
    assert F.get([(1, k1), (4, k4)]) == [None, world.kv[4][k4]]
    got = _snapshot(F, world, base)
    assert got[:3] == snap[:3] and got[4:] == snap[4:]  # (a rebuilt map keeps its new size)
    assert list(F.export_nodes()) == pre
    # the forest goes on: the same tries load again and commit
    F.load_nodes({t: world.roots[t] for t in new}, world.store(new))
    assert F.commit(ups, dels) == {t: o.root_hash() for t, o in _fold(world, ups, dels).items()}
    F.close()


def test_load_under_a_savepoint_released_and_cursor(khst, world):
    from khipu_amd import _lib
    from khipu_amd.device import Ctx
    ctx = Ctx(0)
    r = random.Random(7)
    base, new = list(range(10)), [30, 31, 32]
    F = world.build(ctx, base)
    cur = F.export_cursor()
    F.export_chunk(cur, node_cap=3, rlp_cap=2000)
    F.savepoint()
    F.load_nodes({t: world.roots[t] for t in new}, world.store(new))
    with pytest.raises(_lib.MPTException):  # a cursor from before the load
        F.export_chunk(cur, node_cap=3, rlp_cap=2000)
    F.release()
    assert F.savepoint_depth() == 0
    ups, dels = _batch(world, r, [31, 4])
    assert F.commit(ups, dels) == {t: o.root_hash() for t, o in _fold(world, ups, dels).items()}
    want = {t: world.roots[t] for t in base + new}
    want.update({t: o.root_hash() for t, o in _fold(world, ups, dels).items()})
    assert F.roots() == want
    F.close()


def test_evict(khst, world):
    from khipu_amd import _lib
    from khipu_amd.device import Ctx, ResidentForest
    ctx = Ctx(0)
    r = random.Random(8)
    ids = list(range(60))
    F = ResidentForest.from_nodes(ctx, {t: world.roots[t] for t in ids}, world.store(ids))
    ev, keep = ids[0::2], ids[1::2]
    G = ResidentForest.from_nodes(ctx, {t: world.roots[t] for t in ev}, world.store(ev))
    g_live = G.usage()["live_records"]
    G.close()
    live0 = F.usage()["live_records"]
    before = {t: list(F.export_nodes(trie=t)) for t in keep}
    assert F.evict(ev + [123456]) == len(ev)  # (an id that is not resident is skipped)
    assert F.roots() == {t: world.roots[t] for t in keep}
    q, _ = _queries(world, ev, r, absent=0)
    assert F.get(q) == [None] * len(q)
    u = F.usage()
    assert u["live_records"] == live0 - g_live and u["records"] > u["live_records"]
    assert len(F) == sum(len(world.kv[t]) for t in keep)
    for t in keep:
        assert list(F.export_nodes(trie=t)) == before[t], t
    assert dict(F.export_nodes()) == world.store(keep)
    assert F.evict(ev) == 0
    F.compact()
    u = F.usage()
    assert u["records"] == u["live_records"] == live0 - g_live
    F.load_nodes({t: world.roots[t] for t in ev}, world.store(ev))  # the earlier checkpoint again
    assert F.roots() == {t: world.roots[t] for t in ids}
    ups, dels = _batch(world, r, [2, 3, 40, 41])
    assert F.commit(ups, dels) == {t: o.root_hash() for t, o in _fold(world, ups, dels).items()}
    F.savepoint()
    with pytest.raises(_lib.MPTException):
        F.evict([5])
    F.rollback()
    assert F.evict([5]) == 1
    F.close()


def test_block_commit_over_loaded_tries(khst, oracle):
    """tests/blocks.py's block at its smallest size: the state trie reopened with
    ResidentTrie.from_nodes and the storage forest with ResidentForest.from_nodes give the state
    root and storage roots of the handles built by commits, and of the oracle."""
    import torch
    from khipu_amd.device import Ctx, ResidentForest, ResidentTrie, block_commit
    from tests.blocks import BlockWorkload
    ctx = Ctx(0)
    nc, ns, n = 8, 12, 200
    w = BlockWorkload(ctx, n, 1, seed=5, nc=nc, ns=ns, dirty=40)
    sroot, snodes = w.state.checkpoint()
    froots, fnodes = w.forest.checkpoint()
    assert sorted(froots) == list(range(nc))
    state2 = ResidentTrie.from_nodes(ctx, sroot, snodes, emit=False)
    forest2 = ResidentForest.from_nodes(ctx, froots, fnodes, hash_keys=True)
    ops = w.prepare(0)
    s_tid, s_keys, s_vals, s_voff, d_tid, d_keys, a_keys, a_vals, a_voff, a_tid, a_del = ops
    a_vals2 = a_vals.clone()
    root1 = w.commit_prepared(ops)
    root2 = block_commit(state2, forest2, s_tid, s_keys, s_vals, s_voff, s_tid.numel(), d_tid, d_keys, d_tid.numel(),
                         a_keys, a_vals2, a_voff, a_tid, a_tid.numel(), a_del, a_del.numel() // 32)
    assert root2 == root1
    assert forest2.last_roots() == w.forest.last_roots() and forest2.roots() == w.forest.roots()
    assert torch.equal(a_vals2, a_vals)  # (the same storage roots written into the contract bodies)

    # the oracle: every storage trie, then the state trie over the committed bodies
    def rows(keys, cnt):
        return [bytes(x) for x in keys[:32 * cnt].view(cnt, 32).cpu().numpy()]

    def spans(vals, voff, cnt):
        v, o = vals.cpu().numpy(), voff.cpu().numpy()
        return [v[o[i]:o[i + 1]].tobytes() for i in range(cnt)]
    st = {c: oracle.Trie() for c in range(nc)}
    for tid, keys, vals, voff in w.slot_ups:
        cnt = tid.numel()
        for t, k, v in zip(tid.cpu().tolist(), rows(keys, cnt), spans(vals, voff, cnt)):
            st[t].put(oracle.kec256(k), v)
    for t, k in zip(d_tid.cpu().tolist(), rows(d_keys, d_tid.numel())):
        st[t].remove(oracle.kec256(k))
    sroots = {c: o.root_hash() for c, o in st.items()}
    assert forest2.roots() == sroots
    acc = oracle.Trie()
    for k, v in zip(rows(w.keys, n), spans(w.vals, w.voff, n)):
        acc.put(k, v)
    for keys, vals, voff, cnt in w.ups:
        for k, v in zip(rows(keys, cnt), spans(vals, voff, cnt)):
            acc.put(k, v)
    for k in rows(a_del, a_del.numel() // 32):
        acc.remove(k)
    assert acc.root_hash() == root2
    bodies = spans(a_vals2, a_voff, nc)  # a_tid[c] = c: the contracts come first
    assert [b[-65:-33] for b in bodies] == [sroots[c] for c in range(nc)]
    state2.close()
    forest2.close()


def test_load_roots_evict_through_the_jni_shim(khst, world, tmp_path):
    """forestLoadNodes (with its MPTNodeMissingException path), forestRoots and forestEvict through
    the in-process JNIEnv of tests/jni_stub."""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    stub = os.path.join(ROOT, "tests", "jni_stub")
    exe = tmp_path / "jni_load_driver"
    rc = subprocess.run([cc, "-std=gnu99", "-O1", "-Wall", "-Werror", "-I", stub, "-I", os.path.join(ROOT, "include"),
                         "-o", str(exe), os.path.join(stub, "jni_load_driver.c"), os.path.join(stub, "fake_env.c"),
                         os.path.join(ROOT, "jni", "khst_jni.c"), "-L", os.path.join(ROOT, "khipu_amd"), "-lkhst",
                         "-Wl,-rpath," + os.path.join(ROOT, "khipu_amd"), "-Wl,-rpath-link,/opt/rocm/lib"],
                        capture_output=True, text=True)
    assert rc.returncode == 0, rc.stderr
    ids = [11, 12, 13, (1 << 31) + 7]
    src = {11: 11, 12: 12, 13: 13, (1 << 31) + 7: 14}
    store = world.store(src.values())
    last = world.roots[12]  # the node the first call lacks: the root of the trie listed second
    encs = [e for h, e in store.items() if h != last] + [store[last]]
    off = np.zeros(len(encs) + 1, np.uint64)
    off[1:] = np.cumsum([len(e) for e in encs])
    p = tmp_path / "in.bin"
    with open(p, "wb") as f:
        f.write(np.uint64(len(ids)).tobytes())
        for t in ids:
            f.write(np.uint32(t).tobytes() + world.roots[src[t]])
        f.write(np.uint64(len(encs)).tobytes() + off.tobytes() + b"".join(encs))
    rc = subprocess.run([str(exe), str(p)], capture_output=True, text=True, timeout=120)
    assert rc.returncode == 0, rc.stderr
    lines = [ln.split() for ln in rc.stdout.split("\n")[:-1]]
    assert lines[0] == ["X", "1", "khipu/trie/MerklePatriciaTrie$MPTNodeMissingException", "1", last.hex(), "1", "1",
                        last.hex()], lines[0]
    assert not [x for x in lines if x[0] == "Q"] and ["L", "0"] in lines
    want = sorted((t, world.roots[s].hex()) for t, s in src.items())
    assert [(int(x[1]), x[2]) for x in lines if x[0] == "R"] == want
    assert ["V", "1"] in lines
    assert [(int(x[1]), x[2]) for x in lines if x[0] == "S"] == [w for w in want if w[0] != 11]
    assert lines[-1] == ["E", "0"], lines[-1]
