"""GPU: subtrees of a resident trie evicted to stubs by nibble path (kh_trie_evict_subtrees).
Every expectation is the reference's (tests/evict_ref.py over the oracle's node sets), the oracle's
(oracle.Trie), or the answers of a handle opened from the same witness (kh_trie_open_partial); the
shapes are the smallest at which each path can go wrong."""
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

from khipu_amd import codec
from tests import cases as C
from tests import evict_ref as E
from tests import export_cases, hostprog, path_ref, proof_cases, proof_ref
from tests import partial_cases as P
from tests import writeback as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMPTY = W.EMPTY_TRIE_HASH


def _trie(oracle, keys, vals):
    o = oracle.Trie()
    for k, v in zip(keys, vals):
        o.put(k, v)
    return o


def _state(t):
    """What a refusal, or an eviction that evicts nothing, leaves exactly as it was."""
    root = t.get_root() if hasattr(t, "get_root") else t.roots()
    return root, list(t.export_nodes()), t.stubs, len(t)


def _outcome(call):
    from khipu_amd import _lib
    try:
        return ("page",) + tuple(call())
    except _lib.MPTNodeMissingException as e:
        return ("missing", e.missing)


def _evict_checked(t, nodes, root, chosen, nkeys):
    """One evict_subtrees call on handle t, which holds the set `nodes` and nkeys keys, checked
    against the reference: statuses, hashes, counters, root, export set, stubs and size.  Returns
    (the reference's answer, the set held afterwards)."""
    ev = E.evict(nodes, root, chosen)
    assert not (ev["held"] & ev["removed"]), "a withheld hash is reachable elsewhere in the state"
    stubs0 = len(P.held(nodes, root)[1]) if nodes else 0
    res, cnt = t.evict_subtrees(chosen)
    assert res == ev["status"]
    assert cnt == {"evicted": ev["evicted"], "keys": len(ev["keys"]), "records": ev["records"]}
    assert t.get_root() == root
    part = {h: nodes[h] for h in ev["held"]}
    assert dict(t.export_nodes(verify=True)) == part
    assert t.stubs == len(ev["stubs"]) == stubs0 + ev["evicted"] - ev["stubs_died"]
    assert len(t) == nkeys - len(ev["keys"])
    return ev, part


def _draw(r, nodes, root, n=30, first=4):
    """An antichain of prefixes over every kind of query: an embedded node's path where the state
    has one, then a few hung ones, first."""
    q = E.queries(nodes, root, seed=r.randrange(1 << 30))
    hung = list(q["hung"])
    r.shuffle(hung)
    pool = [p for k in sorted(q) for p in q[k]]
    r.shuffle(pool)
    return E.antichain(sorted(q["embedded"])[:1] + hung[:first] + pool)[:n], q


def _equivalence(khst, ctx, r, nodes, root, live, name):
    """Group 1 on one state: evict a drawn set, then compare with a handle opened from what is left."""
    from khipu_amd.device import UNKNOWN, ResidentTrie
    if root == EMPTY:
        t = ResidentTrie(ctx, [], [])
        assert t.evict_subtrees([(1,), (2, 3)]) == ([(E.NONE, None)] * 2, {"evicted": 0, "keys": 0, "records": 0})
        t.close()
        return {E.NONE}
    t = ResidentTrie.from_nodes(ctx, root, nodes)
    chosen, q = _draw(r, nodes, root)
    ev, part = _evict_checked(t, nodes, root, chosen, len(live))
    seen = {st for st, _ in ev["status"]}
    assert (E.EMBEDDED in seen) == bool(q["embedded"])
    done = [p for p, (st, _) in zip(chosen, ev["status"]) if st == E.DONE]
    gone = list(done)
    if done:
        # again: the evicted prefixes are stubs now, below them hangs nothing, one more is evicted
        more = [p for p in q["hung"] if len(E.antichain(done + [p])) == len(done) + 1][:1]
        again = done[:3] + [p + (5,) for p in done[3:5] if len(p) < 64] + more
        ev2, part = _evict_checked(t, part, root, again, len(live) - len(ev["keys"]))
        assert [st for st, _ in ev2["status"][:len(done[:3])]] == [E.STUB] * len(done[:3])
        seen |= {st for st, _ in ev2["status"]}
        gone += [p for p, (st, _) in zip(again, ev2["status"]) if st == E.DONE]
    w = ResidentTrie.from_witness(ctx, root, part)
    assert (w.stubs, len(w)) == (t.stubs, len(t))
    keys = sorted(live) + [C._rk(r) for _ in range(30)]
    # (a key under an evicted prefix walks into the stub, whether the trie holds it or not)
    under = [any(tuple(proof_ref.nibbles(k)[:len(p)]) == p for p in gone) for k in keys]
    assert t.get(keys) == w.get(keys) == [UNKNOWN if u else live.get(k) for k, u in zip(keys, under)], name
    assert t.need(keys) == w.need(keys)
    ft, pt, tt = t.prove(keys, shared=True)
    fw, pw, tw = w.prove(keys, shared=True)
    assert (ft, pt) == (fw, pw) and sorted(tt.nodes) == sorted(tw.nodes)
    assert [f == 2 for f in ft] == under
    for origin in [None] + r.sample(keys, min(8, len(keys))):
        for mx in (7, 1024):
            assert _outcome(lambda: t.range(origin, None, mx)) == _outcome(lambda: w.range(origin, None, mx)), name
    t.close()
    w.close()
    return seen


@pytest.mark.parametrize("sc", C.commit_scenarios(), ids=lambda s: s[0])
def test_eviction_equals_a_partial_open(khst, oracle, sc):
    from khipu_amd.device import Ctx
    name, ks, vs, batches = sc
    r = random.Random(len(ks) + 17)
    ctx = Ctx(0)
    o = _trie(oracle, ks, vs)
    live = dict(zip(ks, vs))
    seen = _equivalence(khst, ctx, r, W.reachable(o), o.root_hash(), live, (name, 0))
    for i, (ups, dels) in enumerate(batches):
        for k, v in ups:
            o.put(k, v)
            live[k] = v
        for k in dels:
            o.remove(k)
            live.pop(k, None)
        seen |= _equivalence(khst, ctx, r, W.reachable(o), o.root_hash(), live, (name, i + 1))
    want = {"deep": {E.NONE, E.DONE, E.STUB, E.EMBEDDED}, "from_empty": {E.NONE}}
    assert seen >= want.get(name, {E.NONE, E.DONE, E.STUB} if len(ks) > 1 else {E.NONE}), (name, seen)


@pytest.fixture(scope="module")
def rnd300(oracle):
    r = random.Random(300)
    ks = [C._rk(r) for _ in range(300)]
    vs = [C.account_value(r) for _ in ks]
    o = _trie(oracle, ks, vs)
    return dict(keys=ks, vals=vs, nodes=o.reachable(), root=o.root_hash())


def test_eviction_equals_a_partial_open_random_300(khst, oracle, rnd300):
    from khipu_amd.device import Ctx
    w = rnd300
    seen = _equivalence(khst, Ctx(0), random.Random(9), w["nodes"], w["root"], dict(zip(w["keys"], w["vals"])), "rnd300")
    assert seen >= {E.NONE, E.DONE, E.STUB}


# ---- shapes
def test_a_leaf_as_the_anchor(khst, oracle):
    from khipu_amd.device import UNKNOWN, Ctx, ResidentTrie
    A, B = b"\x11" + b"\xaa" * 31, b"\x52" + b"\xbb" * 31
    o = _trie(oracle, [A, B], [b"a" * 40, b"b" * 44])
    nodes, root = o.reachable(), o.root_hash()
    hA = P.path_hashes(nodes, root, A)[0][-1]
    t = ResidentTrie.from_nodes(Ctx(0), root, nodes)
    ev, part = _evict_checked(t, nodes, root, [(1,), (9,), (5, 2)], 2)
    assert ev["status"] == [(E.DONE, hA), (E.NONE, None), (E.NONE, None)] and ev["cause"][2] == "in_leaf"
    assert set(part) == set(nodes) - {hA} and t.get([A, B]) == [UNKNOWN, b"b" * 44] and t.need([A]) == [hA]
    t.close()


def test_an_extension_with_its_branch_is_one_stub(khst, oracle):
    from khipu_amd.device import Ctx, ResidentTrie
    name, ks, _, _ = C.commit_scenarios()[2]
    assert name == "deep"
    o = _trie(oracle, ks, [bytes([i + 1]) * 40 for i in range(len(ks))])
    nodes, root = o.reachable(), o.root_hash()
    sp = dict(path_ref.stored_paths(nodes, root))
    ext_p = next(p for p in E.queries(nodes, root)["hung"] if path_ref.decode(nodes[sp[p]])[0] == "ext")
    target = ext_p + tuple(path_ref.decode(nodes[sp[ext_p]])[1])
    t = ResidentTrie.from_nodes(Ctx(0), root, nodes)
    # the branch's own path is not where the subtree hangs ...
    before = _state(t)
    off = ext_p + (target[len(ext_p)] ^ 1,)
    assert [E.locate(nodes, root, p)[2] for p in (target, off)] == ["ext_target", "off_ext"]
    assert t.evict_subtrees([target, off])[0] == [(E.NONE, None)] * 2 and _state(t) == before
    # ... the extension's is: one plain stub for both
    ev, _ = _evict_checked(t, nodes, root, [ext_p], len(ks))
    assert ev["status"][0] == (E.DONE, sp[ext_p]) and t.stubs == 1
    assert t.evict_subtrees([target])[0] == [(E.NONE, None)]  # (below the stub now)
    assert sp[target] in ev["removed"]
    t.close()


def test_embedded_nodes_are_never_stubs(khst, oracle):
    from khipu_amd.device import Ctx, ResidentTrie
    ks, vs = export_cases.embedded_case()
    o = _trie(oracle, ks, vs)
    nodes, root = o.reachable(), o.root_hash()
    emb = E.antichain(sorted(E.queries(nodes, root)["embedded"], key=len, reverse=True))
    assert emb and {len(p) for p in E.queries(nodes, root)["embedded"]} == {63, 64}
    t = ResidentTrie.from_nodes(Ctx(0), root, nodes)
    before = _state(t)
    for batch in (emb, E.antichain(sorted(E.queries(nodes, root)["embedded"], key=len))):
        res, cnt = t.evict_subtrees(batch)
        assert res == [(E.EMBEDDED, None)] * len(batch) and cnt == {"evicted": 0, "keys": 0, "records": 0}
        assert _state(t) == before
    t.close()


def test_value_only_branch(khst, oracle):
    from khipu_amd.device import Ctx, ResidentTrie
    o, nkeys = hostprog.vb_trie(oracle)
    nodes, root = o.reachable(), o.root_hash()
    hung = E.queries(nodes, root)["hung"]
    vb = [p for p in hung if len(p) == 64]
    assert vb  # khipu's value-only branch hangs at depth 64, referred to by hash
    t = ResidentTrie.from_nodes(Ctx(0), root, nodes)
    ev, part = _evict_checked(t, nodes, root, vb[:1], nkeys)
    assert len(ev["keys"]) == 1 and ev["records"] == 0
    # and a subtree that holds one
    t2 = ResidentTrie.from_nodes(Ctx(0), root, nodes)
    ev, _ = _evict_checked(t2, nodes, root, [vb[0][:1]], nkeys)
    assert E._key(list(vb[0])) in ev["keys"]
    t.close()
    t2.close()


@pytest.fixture(scope="module")
def witness300(rnd300):
    w = rnd300
    some = random.Random(6).sample(w["keys"], 25)
    wit = {}
    for k in some:
        for e in proof_ref.expected_proof(w["nodes"], w["root"], k)[0]:
            wit[proof_ref.kec(e)] = e
    return wit, some


def test_at_and_below_an_existing_stub(khst, oracle, rnd300, witness300):
    from khipu_amd.device import Ctx, ResidentTrie
    w, (wit, some) = rnd300, witness300
    sp = dict(path_ref.stored_paths(w["nodes"], w["root"]))
    missing = [p for p, h in sp.items() if h not in wit and p and sp.get(p[:-1]) in wit]
    assert len(missing) >= 2
    t = ResidentTrie.from_witness(Ctx(0), w["root"], wit)
    before = _state(t)
    ev, _ = _evict_checked(t, wit, w["root"], [missing[0], missing[1] + (3,)], 25)
    assert [st for st, _ in ev["status"]] == [E.STUB, E.NONE] and ev["cause"][1] == "below_stub"
    assert _state(t) == before
    t.close()


def test_a_subtree_that_contains_stubs(khst, oracle, rnd300, witness300):
    from khipu_amd.device import Ctx, ResidentTrie
    w, (wit, some) = rnd300, witness300
    t = ResidentTrie.from_witness(Ctx(0), w["root"], wit)
    n0 = t.stubs
    top = tuple(proof_ref.nibbles(some[0])[:1])
    ev, _ = _evict_checked(t, wit, w["root"], [top], 25)
    assert ev["status"][0][0] == E.DONE and ev["stubs_died"] >= 2 and t.stubs == n0 + 1 - ev["stubs_died"] < n0
    t.close()


def test_a_forest_evicts_in_the_listed_trie_only(khst, oracle, rnd300):
    """Two tries with one content (every prefix shared), one listed; an id the forest does not hold."""
    from khipu_amd.device import UNKNOWN, Ctx, ResidentForest
    w = rnd300
    f = ResidentForest.from_nodes(Ctx(0), {7: w["root"], 9: w["root"]}, w["nodes"])
    tops = E.queries(w["nodes"], w["root"])["hung"]
    a, b = [p for p in tops if len(p) == 1][:2]
    ev = E.evict(w["nodes"], w["root"], [a, b])
    res, cnt = f.evict_subtrees([(9, b), (5, a), (9, a)])
    assert res == [ev["status"][1], (E.NONE, None), ev["status"][0]]
    assert cnt == {"evicted": 2, "keys": len(ev["keys"]), "records": ev["records"]}
    assert f.stubs == 2 and len(f) == 600 - len(ev["keys"]) and f.roots() == {7: w["root"], 9: w["root"]}
    assert dict(f.export_nodes(trie=7, verify=True)) == w["nodes"]
    assert dict(f.export_nodes(trie=9, verify=True)) == {h: w["nodes"][h] for h in ev["held"]}
    k = next(k for k in w["keys"] if k in ev["keys"])
    assert f.get([(7, k), (9, k)]) == [dict(zip(w["keys"], w["vals"]))[k], UNKNOWN]
    f.close()


# ---- more than one block of records and of prefixes
def test_all_depth_2_prefixes_of_3000_hashed_accounts(khst, oracle):
    from khipu_amd.device import Ctx, ResidentTrie
    r = random.Random(3000)
    raw = [C._rk(r) for _ in range(3000)]
    vs = [C.account_value(r) for _ in raw]
    o = _trie(oracle, [proof_ref.kec(k) for k in raw], vs)
    nodes, root = o.reachable(), o.root_hash()
    t = ResidentTrie(Ctx(0), raw, vs, hash_keys=True)
    assert t.root == root
    # 2,048 depth-3 prefixes (eight blocks of prefixes) under the top nibbles 0..7 ...
    d3 = [(a, b, c) for a in range(8) for b in range(16) for c in range(16)]
    ev, part = _evict_checked(t, nodes, root, d3, 3000)
    assert {st for st, _ in ev["status"]} == {E.NONE, E.DONE}
    # ... then all 256 depth-2 prefixes: the reference decides each, the stubs of the first call die
    d2 = [(a, b) for a in range(16) for b in range(16)]
    ev2, part = _evict_checked(t, part, root, d2, 3000 - len(ev["keys"]))
    assert ev2["stubs_died"] == ev["evicted"] and ev2["evicted"] > 200
    above = {h for p, h in path_ref.stored_paths(nodes, root) if len(p) < 2}
    kept = {h for p, (st, _) in zip(d2, ev2["status"]) if st != E.DONE
            for q, h in path_ref.stored_paths(part, root) if q[:2] == p}
    assert set(part) == above | kept
    t.close()


# ---- what the stubs do afterwards
def test_stubs_of_an_eviction_behave_as_stubs(khst, oracle, rnd300):
    from khipu_amd.device import UNKNOWN, Ctx, ResidentTrie
    w = rnd300
    r = random.Random(12)
    nodes, root, kv = w["nodes"], w["root"], dict(zip(w["keys"], w["vals"]))
    ctx = Ctx(0)
    t = ResidentTrie(ctx, w["keys"], w["vals"])
    before = t.copy()
    tops = sorted(p for p in E.queries(nodes, root)["hung"] if len(p) == 1)
    chosen = [tops[1], tops[4], tops[9]]
    ev, part = _evict_checked(t, nodes, root, chosen, 300)
    hashes = [h for _, h in ev["status"]]
    assert all(st == E.DONE for st, _ in ev["status"]) and len(ev["removed"]) <= 400
    state = _state(t)
    # a commit of a key under an evicted prefix: KH_ENODE with that hash, the handle unchanged
    under = next(k for k in w["keys"] if proof_ref.nibbles(k)[0] == chosen[1][0])
    with pytest.raises(khst.MPTNodeMissingException):
        t.commit({under: b"q" * 40})
    assert t.missing() == [(0, hashes[1])] and _state(t) == state
    # a range that crosses an evicted subtree: KH_ENODE with the first one's hash
    assert _outcome(lambda: t.range()) == ("missing", hashes[0])
    # the diff against the copy taken before: equal hashes are skipped, the stub costs nothing
    assert t.diff(before) == ([], False, None) and before.diff(t) == ([], False, None)
    # compaction changes no answer and reclaims the dead records
    answers = (t.get(w["keys"]), t.need(w["keys"]))
    u0 = t.usage()
    t.compact()
    assert t.usage()["records"] < u0["records"] and _state(t)[0::2] == state[0::2]
    assert dict(t.export_nodes(verify=True)) == part and (t.get(w["keys"]), t.need(w["keys"])) == answers
    assert answers[0] == [UNKNOWN if k in ev["keys"] else kv[k] for k in w["keys"]]
    # a commit into a sibling subtree: the oracle's root, and the write-back contract
    o = _trie(oracle, w["keys"], w["vals"]).persist().reopen()
    sib = [k for k in w["keys"] if k not in ev["keys"]][:5]
    ups = [(k, C.account_value(r)) for k in sib] + [(bytes([tops[2][0] << 4 | 3]) + C._rk(r)[1:], b"n" * 40)]
    for k, v in ups:
        o.put(k, v)
    assert t.commit(ups) == o.root_hash() and t.missing() == [] and t.stubs == 3
    W.check_delta(t.nodes(), [o], nodes, "commit beside evicted subtrees")
    # the fill brings the subtrees back
    back = {h: nodes[h] for h in ev["removed"]}
    assert t.fill(back) == len(back)
    assert t.stubs == 0 and len(t) == 301 and dict(t.export_nodes(verify=True)) == o.reachable()
    t.close()
    before.close()


# ---- shrink to a block's witness
def test_shrink_to_the_witness_of_a_block(khst, oracle, rnd300):
    from khipu_amd.device import Ctx, ResidentTrie
    w = rnd300
    r = random.Random(4)
    nodes, root = w["nodes"], w["root"]
    ctx = Ctx(0)
    full = ResidentTrie(ctx, w["keys"], w["vals"])
    t = ResidentTrie(ctx, w["keys"], w["vals"])
    # (An absent key that leaves the path inside an extension proves the extension without its
    # branch.  That branch hangs at no prefix -- the extension's path is where the subtree hangs --
    # so an eviction cannot drop it alone: such keys are not drawn.)
    absent = []
    while len(absent) < 10:
        k = C._rk(r)
        if path_ref.decode(proof_ref.expected_proof(nodes, root, k)[0][-1])[0] != "ext":
            absent.append(k)
    block = r.sample(w["keys"], 20) + absent
    _, _, table = full.prove(block, shared=True)
    wit = {proof_ref.kec(e): e for e in table.nodes}
    on_path = set()
    for k in block:
        on_path |= set(P.path_hashes(nodes, root, k)[0])
    assert set(wit) == on_path
    # every hash-referenced child off the block keys' paths
    sp = dict(path_ref.stored_paths(nodes, root))
    off = E.antichain(sorted((p for p in E.queries(nodes, root)["hung"] if sp[p] not in on_path), key=len))
    ev, part = _evict_checked(t, nodes, root, off, 300)
    assert all(st == E.DONE for st, _ in ev["status"]) and part == wit
    assert 20 <= len(t) <= 30  # (the block's keys, and the leaf an absent key's path ends at)
    ups = [(k, C.account_value(r)) for k in block]
    want = full.commit(ups)
    o = _trie(oracle, w["keys"], w["vals"])
    for k, v in ups:
        o.put(k, v)
    assert t.commit(ups) == want == o.root_hash() and t.missing() == []
    full.close()
    t.close()


# ---- refusals
def test_refusals_leave_the_handle_as_it_was(khst, oracle, rnd300):
    from khipu_amd.device import Ctx, ResidentForest, ResidentTrie
    w = rnd300
    ctx = Ctx(0)
    t = ResidentTrie(ctx, w["keys"], w["vals"])
    f = ResidentForest.from_nodes(ctx, {3: w["root"]}, w["nodes"])
    tops = [p for p in E.queries(w["nodes"], w["root"])["hung"] if len(p) == 1]
    a, b = tops[0], tops[1]
    deep = next(p for p in E.queries(w["nodes"], w["root"])["hung"] if len(p) == 2 and p[:1] == a)
    st, sf = _state(t), _state(f)
    for bad in ([()], [a, ()], [tuple([1] * 65)], [a, b, a], [a, deep], [deep, b, a], [b, a + (0,) * 3, a + (0,)]):
        with pytest.raises(khst.MPTException):
            t.evict_subtrees(bad)
        assert _state(t) == st, bad
    with pytest.raises(khst.MPTException):
        f.evict_subtrees([(3, a)], tries=None)
    with pytest.raises(khst.MPTException):
        f.evict_subtrees([(3, a), (4, b), (3, deep)])
    assert _state(f) == sf
    t.savepoint()
    with pytest.raises(khst.MPTException):
        t.evict_subtrees([a])
    t.release()
    assert _state(t) == st
    # the same prefix in two tries is no duplicate; an empty list does nothing
    assert [s for s, _ in f.evict_subtrees([(3, a), (4, a)])[0]] == [E.DONE, E.NONE]
    assert t.evict_subtrees([]) == ([], {"evicted": 0, "keys": 0, "records": 0}) and _state(t) == st
    assert [s for s, _ in t.evict_subtrees([a, b])[0]] == [E.DONE, E.DONE]
    t.close()
    f.close()


# ---- the JNI shim
def test_evict_subtrees_through_the_jni_shim(khst, oracle, tmp_path):
    """evictSubtrees, its statuses, a refused apply, fillNodes and apply again, through the
    in-process JNIEnv of tests/jni_stub."""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    stub = os.path.join(ROOT, "tests", "jni_stub")
    exe = tmp_path / "jni_evict_driver"
    rc = subprocess.run([cc, "-std=gnu99", "-O1", "-Wall", "-Werror", "-I", stub, "-I", os.path.join(ROOT, "include"),
                         "-o", str(exe), os.path.join(stub, "jni_evict_driver.c"), os.path.join(stub, "fake_env.c"),
                         os.path.join(ROOT, "jni", "khst_jni.c"), "-L", os.path.join(ROOT, "khipu_amd"), "-lkhst",
                         "-Wl,-rpath," + os.path.join(ROOT, "khipu_amd"), "-Wl,-rpath-link,/opt/rocm/lib"],
                        capture_output=True, text=True)
    assert rc.returncode == 0, rc.stderr
    A, B = b"\x11" + b"\xaa" * 31, b"\x52" + b"\xbb" * 31
    o = _trie(oracle, [A, B], [b"a" * 40, b"b" * 44])
    nodes, root = o.reachable(), o.root_hash()
    hA = P.path_hashes(nodes, root, A)[0][-1]
    val = b"z" * 50
    prefixes = [(1,), (9,)]
    encs = list(nodes.values())
    off = np.zeros(len(encs) + 1, np.uint64)
    off[1:] = np.cumsum([len(e) for e in encs])
    p = tmp_path / "in.bin"
    with open(p, "wb") as fh:
        fh.write(root + A + np.uint64(len(val)).tobytes() + val)
        fh.write(np.uint64(len(prefixes)).tobytes() + bytes(len(q) for q in prefixes))
        fh.write(b"".join(codec.nibbles_to_path32(q) for q in prefixes))
        fh.write(np.uint64(len(encs)).tobytes() + off.tobytes() + b"".join(encs))
    rc = subprocess.run([str(exe), str(p)], capture_output=True, text=True, timeout=120)
    assert rc.returncode == 0, rc.stderr
    lines = [ln.split() for ln in rc.stdout.split("\n")[:-1]]
    o.put(A, val)
    assert lines == [["O", "1", "0", "0"],
                     ["V", "1", "0", "1"],
                     ["S", "1", hA.hex()],
                     ["S", "0", "00" * 32],
                     ["A", "1", "khipu/trie/MerklePatriciaTrie$MPTNodeMissingException", "1", hA.hex()],
                     ["F", "1", "0", "0"],
                     ["C", "0", o.root_hash().hex()],
                     ["E", "0"]], lines
