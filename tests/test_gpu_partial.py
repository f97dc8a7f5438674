"""GPU: partial resident tries -- opened from a witness (kh_trie_open_partial,
kh_forest_load_partial), committed along the resident paths, refused with KH_ENODE where the
reference would throw MPTNodeMissingException (kh_trie_missing), and filled (kh_trie_fill_nodes).
Every expectation is the oracle's (oracle.Trie), tests/proof_ref.expected_proof, or read off the
node encodings (tests/partial_cases); the shapes are the smallest at which each path can go wrong."""
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

from khipu_amd import codec
from tests import cases as C
from tests import partial_cases as P
from tests import proof_cases, proof_ref
from tests import writeback as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMPTY = W.EMPTY_TRIE_HASH


def _trie(oracle, keys, vals):
    o = oracle.Trie()
    for k, v in zip(keys, vals):
        o.put(k, v)
    return o


def _missing(khst, call):
    """call() must raise MPTNodeMissingException (KH_ENODE)."""
    with pytest.raises(khst.MPTNodeMissingException) as e:
        call()
    assert e.value.code == -4
    return e.value


@pytest.fixture(scope="module")
def two(oracle):
    """Two keys under a root branch (hashed leaves: 40-byte values), a third for an empty slot."""
    A, B, Cc = b"\x11" + b"\xaa" * 31, b"\x52" + b"\xbb" * 31, b"\x93" + b"\xcc" * 31
    vA, vB = b"a" * 40, b"b" * 44
    o = _trie(oracle, [A, B], [vA, vB])
    nodes = o.reachable()
    root = o.root_hash()
    hA, hB = P.path_hashes(nodes, root, A)[0][-1], P.path_hashes(nodes, root, B)[0][-1]
    assert len(nodes) == 3 and hA != hB and sorted(P.hash_children(nodes[root])) == sorted([hA, hB])
    return dict(A=A, B=B, C=Cc, vA=vA, vB=vB, nodes=nodes, root=root, hA=hA, hB=hB)


def test_root_only_witness_commits_into_an_empty_slot(khst, oracle, two):
    from khipu_amd.device import Ctx, ResidentTrie
    w = two
    t = ResidentTrie.from_witness(Ctx(0), w["root"], {w["root"]: w["nodes"][w["root"]]})
    assert t.stubs == 2 and len(t) == 0 and t.missing() == []
    _missing(khst, lambda: t.commit({w["A"]: b"x" * 41}))
    assert set(t.missing()) == {(0, w["hA"])}
    assert t.get_root() == w["root"] and t.stubs == 2
    assert t.need([w["A"], w["B"], w["C"]]) == [w["hA"], w["hB"], None]
    o = _trie(oracle, [w["A"], w["B"]], [w["vA"], w["vB"]])
    o.put(w["C"], b"c" * 48)
    assert t.commit({w["C"]: b"c" * 48}) == o.root_hash()  # no fetch: the siblings stay stubs
    assert t.stubs == 2 and len(t) == 1 and t.missing() == []
    assert t.fill({w["hA"]: w["nodes"][w["hA"]]}) == 1
    assert t.stubs == 1 and len(t) == 2
    o.put(w["A"], b"x" * 41)
    assert t.commit({w["A"]: b"x" * 41}) == o.root_hash()
    assert t.stubs == 1 and t.get([w["A"], w["C"]]) == [b"x" * 41, b"c" * 48]
    t.close()


def test_a_delete_that_would_move_a_stub_is_refused_unchanged(khst, oracle, two):
    from khipu_amd.device import Ctx, ResidentTrie
    w = two
    wit = {h: w["nodes"][h] for h in (w["root"], w["hA"])}
    t = ResidentTrie.from_witness(Ctx(0), w["root"], wit)
    assert t.stubs == 1 and len(t) == 1
    before = list(t.export_nodes(verify=True))
    assert dict(before) == wit
    cur = t.export_cursor()
    t.export_chunk(cur, node_cap=1)  # a cursor in flight
    _missing(khst, lambda: t.commit(deletes=[w["A"]]))  # the collapse: fix would load leaf B
    assert set(t.missing()) == {(0, w["hB"])}
    assert t.get_root() == w["root"] and t.get([w["A"]]) == [w["vA"]] and t.stubs == 1 and len(t) == 1
    assert list(t.export_nodes(verify=True)) == before  # byte-identical, in the same order
    # the epoch rule of a refused commit: the cursor from before it has ended
    with pytest.raises(khst.MPTException):
        t.export_chunk(cur)
    # root_of is refused the same way and lists the same node
    _missing(khst, lambda: t.root_of(deletes=[w["A"]]))
    assert set(t.missing()) == {(0, w["hB"])}
    assert t.fill([w["nodes"][w["hB"]]]) == 1 and t.stubs == 0
    o = _trie(oracle, [w["B"]], [w["vB"]])
    assert t.commit(deletes=[w["A"]]) == o.root_hash()
    assert t.missing() == [] and dict(t.export_nodes(verify=True)) == o.reachable()
    t.close()


def test_extension_whose_branch_is_missing(khst, oracle):
    from khipu_amd.device import UNKNOWN, Ctx, ResidentTrie
    ek, ev, queries = proof_cases.ext_case()
    o = _trie(oracle, ek, ev)
    nodes, root = o.reachable(), o.root_hash()
    (branch,) = P.hash_children(nodes[root])
    ctx = Ctx(0)
    t = ResidentTrie.from_witness(ctx, root, {root: nodes[root]})
    assert t.stubs == 1 and len(t) == 0
    assert dict(t.export_nodes(verify=True)) == {root: nodes[root]}
    for call in (lambda: t.commit({ek[0]: b"n" * 40}), lambda: t.commit(deletes=[ek[3]]),
                 lambda: t.commit({queries[0]: b"n" * 40}, [ek[5]])):  # any op through the extension
        _missing(khst, call)
        assert set(t.missing()) == {(0, branch)} and t.get_root() == root
    assert t.need([ek[0], queries[0]]) == [branch, None]
    # a key that leaves the path inside the extension splits it over the branch's hash: no fetch
    for q in queries:
        o.put(q, b"n" * 40)
        assert t.commit({q: b"n" * 40}) == o.root_hash()
        assert t.stubs == 1 and set(h for h, _ in t.export_nodes(verify=True)) <= set(o.reachable())
    assert t.get(queries + [ek[0]]) == [b"n" * 40] * 3 + [UNKNOWN]
    _missing(khst, lambda: t.commit({ek[0]: b"n" * 40}))
    assert set(t.missing()) == {(0, branch)}
    # deleting them again merges the pieces back into one extension, still without the branch
    for q in queries:
        o.remove(q)
    assert t.commit(deletes=queries) == root == o.root_hash() and t.stubs == 1
    assert dict(t.export_nodes(verify=True)) == {root: nodes[root]}
    assert t.fill(nodes) == len(nodes) - 1 and t.stubs == 0 and len(t) == len(ek)
    o.put(queries[0], b"n" * 40)
    assert t.commit({queries[0]: b"n" * 40}) == o.root_hash()
    t.close()
    # a missing root: KH_ENODE from the open, with its hash; nothing is opened
    e = _missing(khst, lambda: ResidentTrie.from_witness(ctx, root, {}))
    assert e.missing == root
    e = _missing(khst, lambda: ResidentTrie.from_witness(ctx, root, [nodes[branch]]))
    assert e.missing == root


@pytest.fixture(scope="module")
def rnd300(oracle):
    r = random.Random(300)
    ks = [C._rk(r) for _ in range(300)]
    vs = [C.account_value(r) for _ in ks]
    o = _trie(oracle, ks, vs)
    return dict(keys=ks, vals=vs, nodes=o.reachable(), root=o.root_hash(), r=r)


def test_a_block_over_its_witness_commits_at_the_first_attempt(khst, oracle, rnd300):
    from khipu_amd.device import Ctx, ResidentTrie
    w = rnd300
    r = random.Random(4)
    ctx = Ctx(0)
    full = ResidentTrie(ctx, w["keys"], w["vals"])
    assert full.root == w["root"]
    present, absent = r.sample(w["keys"], 20), [C._rk(r) for _ in range(10)]
    found, _, table = full.prove(present + absent, shared=True)
    assert found == [True] * 20 + [False] * 10
    t = ResidentTrie.from_witness(ctx, w["root"], table.nodes, emit=True)
    assert t.stubs > 0 and len(t) == 20
    o = _trie(oracle, w["keys"], w["vals"]).persist().reopen()
    ups = [(k, C.account_value(r)) for k in present + absent]
    for k, v in ups:
        o.put(k, v)
    assert t.commit(ups) == o.root_hash() and t.missing() == []
    assert len(t) == 30
    new = o.reachable()
    got = dict(t.export_nodes(verify=True))
    assert all(new.get(h) == e for h, e in got.items())  # every exported node is the oracle's
    for k, _ in ups:  # and every node on the 30 paths of the new trie is there
        for e in proof_ref.expected_proof(new, o.root_hash(), k)[0]:
            assert got.get(proof_ref.kec(e)) == e
    W.check_delta(t.nodes(), [o], w["nodes"], "witness block")
    full.close()
    t.close()


@pytest.mark.parametrize("sc", C.commit_scenarios(), ids=lambda s: s[0])
def test_fetch_loop(khst, oracle, sc):
    """Opened with its root node only, every batch is committed by the reference's retry loop: on
    KH_ENODE exactly the listed nodes are supplied and the commit is tried again."""
    from khipu_amd.device import Ctx, ResidentTrie
    name, ks, vs, batches = sc
    o = _trie(oracle, ks, vs)
    root = o.root_hash()
    pre = W.reachable(o)
    t = ResidentTrie.from_witness(Ctx(0), root, {root: pre[root]} if pre else {})
    supplied = set()
    for i, (ups, dels) in enumerate(batches):
        pre, root = W.reachable(o), o.root_hash()
        allowed = P.fetchable(pre, root, [k for k, _ in ups] + list(dels))
        for k, v in ups:
            o.put(k, v)
        for k in dels:
            o.remove(k)
        for rounds in range(131):
            try:
                got = t.commit(ups, dels)
                break
            except khst.MPTNodeMissingException:
                miss = t.missing()
                assert miss and all(tid == 0 for tid, _ in miss), (name, i, rounds)
                hs = {h for _, h in miss}
                assert len(hs) == len(miss) and not hs & supplied, (name, i, rounds)
                assert hs <= allowed, (name, i, rounds, len(hs - allowed))
                assert t.get_root() == root
                assert t.fill({h: pre[h] for h in hs}) == len(hs)
                supplied |= hs
        else:
            raise AssertionError((name, i, "more than 130 rounds"))
        assert got == o.root_hash(), (name, i)
        assert t.missing() == []
    t.close()


def test_reads_on_a_partial_handle(khst, oracle, rnd300):
    from khipu_amd import _lib
    from khipu_amd.device import UNKNOWN, Ctx, ResidentTrie, verify_proofs
    w = rnd300
    r = random.Random(6)
    nodes, root = w["nodes"], w["root"]
    some = r.sample(w["keys"], 25)
    wit = {}
    for k in some:
        for e in proof_ref.expected_proof(nodes, root, k)[0]:
            wit[proof_ref.kec(e)] = e
    have, stubs = P.held(wit, root)
    assert stubs and have == set(wit)
    t = ResidentTrie.from_witness(Ctx(0), root, wit)
    assert t.stubs == len(stubs) and len(t) == 25
    qs = w["keys"] + [C._rk(r) for _ in range(60)] + proof_cases.near_misses(r, some)
    kv = dict(zip(w["keys"], w["vals"]))
    want_get, want_found, want_proof, want_need = [], [], [], []
    for k in qs:
        hs, val = P.path_hashes(nodes, root, k)
        lack = [h for h in hs if h not in have]
        assert val == kv.get(k)
        want_get.append(UNKNOWN if lack else val)
        want_found.append(2 if lack else val is not None)
        want_proof.append([nodes[h] for h in hs[:hs.index(lack[0])]] if lack else [nodes[h] for h in hs])
        want_need.append(lack[0] if lack else None)
    assert any(x is UNKNOWN for x in want_get) and any(x is None for x in want_get)
    assert t.get(qs) == want_get
    assert t.need(qs) == want_need
    found, proofs = t.prove(qs)
    assert found == want_found and proofs == want_proof
    status, _ = verify_proofs(root, qs, proofs)
    for f, s in zip(want_found, status):
        assert s == (_lib.KH_PROOF_SHORT if f == 2 else _lib.KH_PROOF_VALUE if f else _lib.KH_PROOF_ABSENT)
    # a stub never answers for the hashes it carries
    ask = sorted(set(stubs))[:40] + sorted(have)[:5]
    assert t.nodes_by_hash(ask) == [None] * (len(ask) - 5) + [nodes[h] for h in sorted(have)[:5]]
    assert dict(t.export_nodes(verify=True)) == wit
    t.close()


# ---- a forest of storage tries and a block over a partial state trie
class Block:
    """60 storage tries of 1-300 slots (two ids with one root, ids past the op sort's trie-id bits),
    a state trie of 200 accounts, and one block: slot upserts and deletes in 12 tries, their
    accounts rewritten with the new storage roots, a few plain account upserts."""

    def __init__(self, oracle):
        r = random.Random(77)
        self.oracle = oracle
        ids = list(range(1, 55)) + [(1 << 31) + 5, (1 << 32) - 2, (1 << 24) + 3, 70, 71, 72]
        self.kv = {}
        for j, t in enumerate(ids):
            n = [1, 2, 3, 17][j] if j < 4 else r.randint(1, 300)
            self.kv[t] = {C._rk(r): (C.storage_value(r) if (j + i) % 4 else b"v" * 33) for i in range(n)}
        self.kv[71] = dict(self.kv[70])  # two ids, one root
        self.ids = ids
        self.st = {t: self.trie(t) for t in ids}
        self.roots = {t: o.root_hash() for t, o in self.st.items()}
        self.store = {}
        for o in self.st.values():
            self.store.update(o.reachable())
        # the state trie: account j owns storage trie ids[j] for j < 60
        self.akeys = [C._rk(r) for _ in range(200)]
        self.avals = [codec.account_rlp(j, 10 ** 18 + j, state_root=self.roots[ids[j]] if j < 60 else EMPTY)
                      for j in range(200)]
        self.state = _trie(oracle, self.akeys, self.avals)
        self.aroot, self.anodes = self.state.root_hash(), self.state.reachable()
        # the block
        self.touched = [ids[j] for j in (0, 3, 7, 12, 20, 33, 54, 55, 56, 57, 58, 41)]
        self.s_up, self.s_del = [], []
        for t in self.touched:
            ks = list(self.kv[t])
            self.s_up += [(t, k, C.storage_value(r)) for k in ks[:2]] + [(t, C._rk(r), b"n" * 34) for _ in range(2)]
            if len(ks) > 4:
                self.s_del += [(t, ks[-1])]
        self.a_up = [(self.akeys[ids.index(t)], codec.account_rlp(9, 5, state_root=b"\0" * 32), t) for t in self.touched]
        self.a_up += [(self.akeys[150 + j], codec.account_rlp(1, j), None) for j in range(5)]
        self.a_up += [(C._rk(r), codec.account_rlp(2, 2), None) for _ in range(3)]
        # what the block needs from the stores: the paths of its keys and the children of their nodes
        self.swit = {}
        for t in self.touched:
            keys = [k for tt, k, _ in self.s_up if tt == t] + [k for tt, k in self.s_del if tt == t]
            for h in P.fetchable(self.st[t].reachable(), self.roots[t], keys) | {self.roots[t]}:
                self.swit[h] = self.store[h]
        for t in ids:  # (every listed trie needs its root node)
            self.swit[self.roots[t]] = self.store[self.roots[t]]
        self.awit = {h: self.anodes[h] for h in P.fetchable(self.anodes, self.aroot, [k for k, _, _ in self.a_up])}
        # the oracle's storage roots after the block
        self.new_roots = {}
        for t in self.touched:
            o = self.trie(t)
            for tt, k, v in self.s_up:
                if tt == t:
                    o.put(k, v)
            for tt, k in self.s_del:
                if tt == t:
                    o.remove(k)
            self.new_roots[t] = o.root_hash()
        s2 = _trie(oracle, self.akeys, self.avals)
        for k, body, t in self.a_up:
            s2.put(k, body if t is None else body[:-65] + self.new_roots[t] + body[-33:])
        self.new_aroot = s2.root_hash()

    def trie(self, t):
        return _trie(self.oracle, list(self.kv[t]), list(self.kv[t].values()))

    def run(self, state, forest):
        from khipu_amd import _lib
        from khipu_amd.device import block_commit_host

        def pk(items):
            return np.frombuffer(b"".join(items) + b"\0" * 8, np.uint8).copy()

        def off(items):
            o = np.zeros(len(items) + 1, np.uint64)
            o[1:] = np.cumsum([len(x) for x in items])
            return o
        sv = [v for _, _, v in self.s_up]
        av = [b for _, b, _ in self.a_up]
        return block_commit_host(
            state, forest, np.array([t for t, _, _ in self.s_up], np.uint32), pk([k for _, k, _ in self.s_up]), pk(sv),
            off(sv), np.array([t for t, _ in self.s_del], np.uint32), pk([k for _, k in self.s_del]),
            pk([k for k, _, _ in self.a_up]), pk(av), off(av),
            np.array([_lib.KH_NO_TRIE if t is None else t for _, _, t in self.a_up], np.uint32), None)


@pytest.fixture(scope="module")
def block(oracle):
    return Block(oracle)


def test_forest_partial_load_and_block_commit(khst, oracle, block):
    from khipu_amd.device import Ctx, ResidentForest, ResidentTrie
    b = block
    ctx = Ctx(0)
    # the same block on full handles: the oracle's roots
    fs = ResidentTrie.from_nodes(ctx, b.aroot, b.anodes, emit=False)
    ff = ResidentForest.from_nodes(ctx, b.roots, b.store)
    assert b.run(fs, ff) == b.new_aroot and ff.last_roots() == b.new_roots
    # partial handles from the witnesses
    ps = ResidentTrie.from_witness(ctx, b.aroot, b.awit, emit=False)
    pf = ResidentForest(ctx)
    pf.load_partial(b.roots, b.swit)
    assert ps.stubs > 0 and pf.stubs > 0 and pf.roots() == b.roots
    nstub = pf.stubs
    with pytest.raises(khst.MPTException):  # a resident id
        pf.load_partial({b.ids[3]: b.roots[b.ids[3]]}, b.swit)
    assert pf.stubs == nstub and pf.roots() == b.roots
    # one storage witness node withheld: KH_ENODE, both handles byte-identical, the forest's list only
    t0 = max(b.touched, key=lambda t: len(b.kv[t]))  # (the largest: its paths pass a node below the root)
    k0 = next(k for t, k, _ in b.s_up if t == t0)
    hs, _ = P.path_hashes(b.st[t0].reachable(), b.roots[t0], k0)
    assert len(hs) >= 2
    gone = hs[1]
    qs = ResidentTrie.from_witness(ctx, b.aroot, b.awit, emit=False)
    qf = ResidentForest(ctx)
    qf.load_partial(b.roots, {h: e for h, e in b.swit.items() if h != gone})
    before = (list(qs.export_nodes()), list(qf.export_nodes()), qs.get_root(), qf.roots(), qs.stubs, qf.stubs)
    _missing(khst, lambda: b.run(qs, qf))
    assert (list(qs.export_nodes()), list(qf.export_nodes()), qs.get_root(), qf.roots(), qs.stubs, qf.stubs) == before
    assert set(qf.missing()) == {(t0, gone)} and qs.missing() == []
    t1 = next(t for t in b.touched if t != t0)
    assert qf.need([(t0, k0), (t1, next(k for t, k, _ in b.s_up if t == t1))]) == [gone, None]
    assert qf.fill(b.swit) >= 1  # (the withheld node and what hangs under it in the witness)
    assert b.run(qs, qf) == b.new_aroot and qf.last_roots() == b.new_roots
    # the block at the first attempt on the full witnesses
    assert b.run(ps, pf) == b.new_aroot and pf.last_roots() == b.new_roots
    assert ps.missing() == [] and pf.missing() == []
    assert pf.stubs == nstub  # a successful commit never creates, kills or moves a stub
    # eviction drops a partially held trie's stubs with it
    idle = next(t for t in b.ids if t not in b.touched and len(b.kv[t]) > 40)
    held_, st_ = P.held(b.swit, b.roots[idle])
    assert held_ == {b.roots[idle]} and st_
    n0 = pf.stubs
    assert pf.evict([idle]) == 1 and pf.stubs == n0 - len(st_)
    for x in (fs, ff, ps, pf, qs, qf):
        x.close()


def test_versions_and_space_on_a_partial_handle(khst, oracle, block, rnd300):
    from khipu_amd.device import Ctx, ResidentForest, ResidentTrie
    b, w = block, rnd300
    ctx = Ctx(0)
    f = ResidentForest(ctx)
    first = {t: b.roots[t] for t in b.ids[:10]}
    f.load_partial(first, b.swit)
    s0, n0, r0 = f.stubs, len(f), f.roots()
    # a partial load under a savepoint, rolled back
    f.savepoint()
    f.load_partial({t: b.roots[t] for t in b.ids[10:30]}, b.swit)
    assert f.stubs > s0 and len(f.roots()) == 30
    with pytest.raises(khst.MPTException):  # fill under a savepoint
        f.fill(b.store)
    f.rollback()
    assert (f.stubs, len(f), f.roots()) == (s0, n0, r0)
    # commit + rollback, root_of, compact, copy on a partial single trie
    r = random.Random(8)
    some = r.sample(w["keys"], 12)
    wit = {}
    for k in some:
        for e in proof_ref.expected_proof(w["nodes"], w["root"], k)[0]:
            wit[proof_ref.kec(e)] = e
    t = ResidentTrie.from_witness(ctx, w["root"], wit)
    ns = t.stubs
    ups = [(k, C.account_value(r)) for k in some[:6]]
    o = _trie(oracle, w["keys"], w["vals"])
    for k, v in ups:
        o.put(k, v)
    assert t.root_of(ups) == o.root_hash() and t.get_root() == w["root"]
    t.savepoint()
    assert t.commit(ups) == o.root_hash()
    t.rollback()
    assert t.get_root() == w["root"] and t.stubs == ns and dict(t.export_nodes(verify=True)) == wit
    assert t.commit(ups) == o.root_hash()
    exp = dict(t.export_nodes(verify=True))
    c = t.copy()
    t.compact()
    assert t.stubs == ns and t.get_root() == o.root_hash() and dict(t.export_nodes(verify=True)) == exp
    o.remove(some[7])  # (its siblings' paths are in the witness: 12 keys of 300 share the top branch only)
    try:
        got = t.commit(deletes=[some[7]])
    except khst.MPTNodeMissingException:
        hs = {h for _, h in t.missing()}
        assert hs and t.fill({h: w["nodes"][h] for h in hs}) == len(hs)
        got = t.commit(deletes=[some[7]])
    assert got == o.root_hash()
    assert c.get_root() != got and c.stubs == ns and dict(c.export_nodes(verify=True)) == exp  # the copy is independent
    for x in (f, t, c):
        x.close()


def test_fill_past_half_the_anchor_map(khst, oracle):
    """Root-only open of a 3,000-key trie, filled with the whole store: the fill appends far more
    records than the map of the one-record handle holds; the result is the full handle."""
    from khipu_amd.device import Ctx, ResidentTrie
    r = random.Random(3000)
    ks = [C._rk(r) for _ in range(3000)]
    vs = [C.account_value(r) for _ in ks]
    o = _trie(oracle, ks, vs)
    nodes, root = o.reachable(), o.root_hash()
    ctx = Ctx(0)
    t = ResidentTrie.from_witness(ctx, root, {root: nodes[root]})
    assert t.stubs == 16 and len(t) == 0
    assert t.fill(nodes) == len(nodes) - 1
    full = ResidentTrie.from_nodes(ctx, root, nodes)
    assert t.stubs == 0 and len(t) == len(full) == 3000 and t.get_root() == full.get_root() == root
    assert dict(t.export_nodes(verify=True)) == dict(full.export_nodes()) == nodes
    q = r.sample(ks, 50) + [C._rk(r) for _ in range(5)]
    assert t.get(q) == full.get(q)
    t.close()
    full.close()


def test_partial_calls_through_the_jni_shim(khst, oracle, two, tmp_path):
    """openPartial, apply refused with MPTNodeMissingException (its hash from missing()), need,
    fillNodes and apply again, through the in-process JNIEnv of tests/jni_stub."""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    stub = os.path.join(ROOT, "tests", "jni_stub")
    exe = tmp_path / "jni_partial_driver"
    rc = subprocess.run([cc, "-std=gnu99", "-O1", "-Wall", "-Werror", "-I", stub, "-I", os.path.join(ROOT, "include"),
                         "-o", str(exe), os.path.join(stub, "jni_partial_driver.c"), os.path.join(stub, "fake_env.c"),
                         os.path.join(ROOT, "jni", "khst_jni.c"), "-L", os.path.join(ROOT, "khipu_amd"), "-lkhst",
                         "-Wl,-rpath," + os.path.join(ROOT, "khipu_amd"), "-Wl,-rpath-link,/opt/rocm/lib"],
                        capture_output=True, text=True)
    assert rc.returncode == 0, rc.stderr
    w = two
    val = b"z" * 50
    encs = [w["nodes"][w["root"]], w["nodes"][w["hA"]], w["nodes"][w["hB"]]]
    off = np.zeros(len(encs) + 1, np.uint64)
    off[1:] = np.cumsum([len(e) for e in encs])
    p = tmp_path / "in.bin"
    with open(p, "wb") as f:
        f.write(w["root"] + w["A"] + np.uint64(len(val)).tobytes() + val)
        f.write(np.uint64(len(encs)).tobytes() + off.tobytes() + b"".join(encs))
    rc = subprocess.run([str(exe), str(p)], capture_output=True, text=True, timeout=120)
    assert rc.returncode == 0, rc.stderr
    lines = [ln.split() for ln in rc.stdout.split("\n")[:-1]]
    o = _trie(oracle, [w["A"], w["B"]], [w["vA"], w["vB"]])
    o.put(w["A"], val)
    assert lines == [["O", "1", "0", "2"],
                     ["A", "1", "khipu/trie/MerklePatriciaTrie$MPTNodeMissingException", "1", w["hA"].hex()],
                     ["M", "0", w["hA"].hex()],
                     ["N", "1", w["hA"].hex()],
                     ["F", "2", "0", "0"],
                     ["C", "0", o.root_hash().hex()],
                     ["E", "0"]], lines


@pytest.mark.parametrize("sc", C.commit_scenarios(), ids=lambda s: s[0])
def test_full_store_through_the_partial_open_is_a_full_handle(khst, oracle, sc):
    """The regression guard: kh_trie_open_partial over a full store leaves no stub, and every
    scenario gives the roots and the write-back sets of a from_nodes handle."""
    from khipu_amd.device import Ctx, ResidentTrie
    name, ks, vs, batches = sc
    o = _trie(oracle, ks, vs)
    nodes, root = W.reachable(o), o.root_hash()
    ctx = Ctx(0)
    a = ResidentTrie.from_witness(ctx, root, nodes)
    b = ResidentTrie.from_nodes(ctx, root, nodes)
    assert a.stubs == 0 and b.stubs == 0 and len(a) == len(b) == len(set(ks))
    assert dict(a.export_nodes()) == dict(b.export_nodes()) == nodes  # (the two opens order their records differently)
    for i, (ups, dels) in enumerate(batches):
        for k, v in ups:
            o.put(k, v)
        for k in dels:
            o.remove(k)
        ra, rb = a.commit(ups, dels), b.commit(ups, dels)
        assert ra == rb == o.root_hash(), (name, i)
        assert a.nodes() == b.nodes(), (name, i)
        assert a.missing() == [] and a.stubs == 0
    a.close()
    b.close()
