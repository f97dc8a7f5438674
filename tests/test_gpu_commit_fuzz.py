"""GPU: one resident trie, and one resident forest, driven through long random operation
sequences on dense keys (tests/fuzz_cases.py) with the model checked after every step: commits
(accepted and refused), savepoints, rollbacks, root_of, copies, compaction, export and reopen,
partial reopen with the fetch loop, proofs; in the forest also evict, load and partial load.

Every expectation is the model's: oracle.Trie folded batch by batch (roots, sizes, gets, refusals),
tests/writeback.check_delta over the oracle's Updated log (write-back sets),
tests/proof_ref.expected_proof over the oracle's nodes (proofs).  A failure names (seed, step,
operation); fuzz_cases.replay(seed, step + 1) gives the steps up to it as data.
tests/test_commit_fuzz_model.py holds the sequences to what they must reach."""
import pytest

from tests import fuzz_cases as F
from tests import proof_ref
from tests import writeback as W

pytestmark = pytest.mark.gpu
EMPTY = W.EMPTY_TRIE_HASH


def _paths_held(nodes, root, key, held):
    return root == EMPTY or all(proof_ref.kec(e) in held for e in proof_ref.expected_proof(nodes, root, key)[0])


def _check_gets(t, m, keys, held, safe, what, UNKNOWN):
    """get over keys against the oracle.  On a partial handle (held: an upper bound of the node
    hashes it holds) a key whose path leaves `held` gives UNKNOWN, a key the handle has put gives
    its value, and every other answer is the oracle's or UNKNOWN."""
    got = t.get(keys)
    nodes = m.nodes() if held is not None else None
    for k, g in zip(keys, got):
        want = m.t.get(k)
        if held is None or (k in safe and want is not None):
            assert g == want, (what, "get", k.hex())
        elif not _paths_held(nodes, m.root(), k, held):
            assert g is UNKNOWN, (what, "get under a stub", k.hex())
        else:
            assert g is UNKNOWN or g == want, (what, "get", k.hex())


def _check_state(t, m, step, safe, what, UNKNOWN):
    assert t.get_root() == step["root"] == m.root(), (what, "root")
    if step.get("held") is None:
        assert len(t) == step["len"], (what, "len")
    else:
        assert len(t) <= step["len"], (what, "len of a partial handle")
    _check_gets(t, m, step["probe"], step.get("held"), safe, what, UNKNOWN)


def _commit(khst, t, call, step, m, root0, can_fetch, what):
    """The reference's retry loop around one commit or root_of: (result or None when refused, nodes fetched)."""
    fetched = set()
    for _ in range(300):
        before = (len(t), t.stubs)
        try:
            return call(), fetched
        except khst.MPTNodeMissingException:
            assert can_fetch, (what, "a missing node on paths the handle holds")
            hs = {h for _, h in t.missing()}
            assert hs and not hs & fetched and hs <= step["allowed"], (what, "missing() outside the walk")
            assert t.get_root() == root0 and (len(t), t.stubs) == before, (what, "changed by a commit that lacked a node")
            assert t.fill({h: m.store[h] for h in hs}) == len(hs), (what, "fill")
            fetched |= hs
        except khst.MPTException:
            return None, fetched
    raise AssertionError((what, "more than 300 fetch rounds"))


@pytest.mark.parametrize("seed", F.TRIE_SEEDS)
def test_trie_sequence(khst, oracle, seed):
    from khipu_amd import _lib
    from khipu_amd.device import UNKNOWN, Ctx, ResidentTrie, verify_proofs
    ctx = Ctx(0)
    t = side = None
    root0 = EMPTY
    try:
        for i, step, m in F.trie_run(seed, oracle):
            op = step["op"]
            what = (seed, i, op)
            partial = step.get("held") is not None or op == "fill_all"
            if op == "open":
                t = ResidentTrie(ctx, [k for k, _ in step["ups"]], [v for _, v in step["ups"]])
            elif op == "commit":
                depth = step["depth"]
                got, fetched = _commit(khst, t, lambda: t.commit(step["ups"], step["dels"]), step, m, root0,
                                       "allowed" in step and not depth, what)
                if step["refused"]:
                    assert got is None, (what, "accepted a batch the reference refuses")
                else:
                    assert got is not None, (what, "refused")
                    assert got == step["root"], (what, "root")
                    assert fetched or not step.get("must_fetch"), (what, "committed through a node it cannot hold")
                    W.check_delta(t.nodes(), [m.t], m.store, what)
            elif op == "root_of":
                got, _ = _commit(khst, t, lambda: t.root_of(step["ups"], step["dels"]), step, m, root0,
                                 "allowed" in step and not step["depth"], what)
                assert got == step["want"], (what, "speculative root")
            elif op == "savepoint":
                assert t.savepoint() == step["depth"], what
            elif op == "rollback":
                t.rollback()
                if step["wb"] is not None:  # the write-back set is the savepoint's: within the oracle's bounds for it
                    must, may = step["wb"]
                    got = t.nodes()
                    assert all(got.get(h) == e for h, e in must.items()), (what, "write-back set: a node lost")
                    assert all(may.get(h) == e for h, e in got.items()), (what, "write-back set: a node too many")
            elif op == "release":
                t.release()
            elif op == "copy":
                c = t.copy()
                if step["mode"] == "switch":
                    t.close()
                    t = c
                elif step["mode"] == "stay":
                    c.close()
                else:  # both live on: the copy takes a batch of its own and is looked at again five steps on
                    if side:
                        side[0].close()
                    sm = step["side"]
                    got, _ = _commit(khst, c, lambda: c.commit(step["ups"], step["dels"]), step, m, root0, True, what)
                    assert (got is None) == step["side_refused"], (what, "the copy's commit")
                    assert c.get_root() == step["side_root"], (what, "the copy's root")
                    side = (c, sm, step, i + 5, partial)
            elif op == "compact":
                if step["refused"]:
                    with pytest.raises(khst.MPTException):
                        t.compact()
                else:
                    t.compact()
            elif op == "export":
                got = dict(t.export_nodes(verify=True))
                assert got == step["want"], (what, "export")
                t.close()
                t = ResidentTrie.from_nodes(ctx, step["root"], step["want"])
            elif op == "partial":
                t.close()
                t = ResidentTrie.from_witness(ctx, step["root"], step["witness"])
                assert dict(t.export_nodes(verify=True)) == step["witness"], (what, "the witness held")
            elif op == "fill_all":
                t.fill(m.nodes())
                assert t.stubs == 0, (what, "stubs after a fill of the whole store")
            elif op == "prove":
                keys = step["keys"]
                nodes = m.nodes()
                found, proofs = t.prove(keys)
                for k, f, p in zip(keys, found, proofs):
                    want, val = proof_ref.expected_proof(nodes, m.root(), k)
                    if f == 2:
                        assert partial and p == want[:len(p)] and len(p) < len(want), (what, "proof to a stub", k.hex())
                    else:
                        assert f == (val is not None) and p == want, (what, "proof", k.hex())
                status, vals = verify_proofs(m.root(), keys, proofs)
                for k, f, s, v in zip(keys, found, status, vals):
                    val = m.t.get(k)
                    want = _lib.KH_PROOF_SHORT if f == 2 else _lib.KH_PROOF_VALUE if val is not None else _lib.KH_PROOF_ABSENT
                    assert s == want and (s != _lib.KH_PROOF_VALUE or v == val), (what, "verify_proofs", k.hex())
            _check_state(t, m, step, step.get("safe", set()), what, UNKNOWN)
            assert t.savepoint_depth() == step["depth"], (what, "savepoint depth")
            if side and (i >= side[3] or i == F.NSTEPS):
                c, sm, st, _, was_partial = side
                assert c.get_root() == st["side_root"] == sm.root(), (what, "the copy, five steps on")
                if not was_partial:
                    assert len(c) == st["side_len"], (what, "the copy's len")
                for k, g in zip(st["side_probe"], c.get(st["side_probe"])):
                    assert g == sm.t.get(k) or (was_partial and g is UNKNOWN), (what, "the copy's get", k.hex())
                c.close()
                side = None
            root0 = step["root"]
        assert i == F.NSTEPS and side is None
    finally:
        for h in (t, side[0] if side else None):
            if h is not None:
                h.close()
        ctx.close()


@pytest.mark.parametrize("seed", F.FOREST_SEEDS)
def test_forest_sequence(khst, oracle, seed):
    from khipu_amd import _lib
    from khipu_amd.device import UNKNOWN, Ctx, ResidentForest, verify_proofs
    ctx = Ctx(0)
    f = ResidentForest(ctx, emit=True)
    try:
        roots0 = {}
        for i, step, ms, resident in F.forest_run(seed, oracle):
            op = step["op"]
            what = (seed, i, op)
            if op == "commit":
                try:
                    got = f.commit(step["ups"], step["dels"])
                except khst.MPTException:
                    got = None
                if step["refused"]:
                    assert got is None, (what, "accepted a batch the reference refuses")
                else:
                    assert got is not None, (what, "refused")
                    assert got == {t: ms[t].root() for t in step["touched"]}, (what, "roots of the commit")
                    store = {}
                    for t in step["touched"]:
                        store.update(ms[t].store)
                    W.check_delta(f.nodes(), [ms[t].t for t in step["touched"]], store, what)
            elif op == "savepoint":
                assert f.savepoint() == step["depth"], what
            elif op == "rollback":
                f.rollback()
            elif op == "release":
                f.release()
            elif op == "compact":
                if step["refused"]:
                    with pytest.raises(khst.MPTException):
                        f.compact()
                else:
                    f.compact()
            elif op == "evict":
                n = f.evict(step["ids"])  # (a trie emptied by a commit may or may not still count as one)
                assert sum(1 for t in step["ids"] if ms[t].live) <= n <= len(step["ids"]), (what, "tries dropped")
            elif op == "load":
                store = {}
                for t in step["ids"]:
                    store.update(ms[t].nodes())
                f.load_nodes({t: ms[t].root() for t in step["ids"]}, store)
            elif op == "load_partial":
                t, m = step["id"], ms[step["id"]]
                f.load_partial({t: m.root()}, step["witness"])
                assert dict(f.export_nodes(trie=t, verify=True)) == step["witness"], (what, "the witness held")
                nodes = m.nodes()
                q = [k for x, k in step["probe"] if x == t]
                for k, g in zip(q, f.get([(t, k) for k in q])):
                    if all(h in step["held"] for h in F.path_set(nodes, m.root(), [k])):
                        assert g == m.t.get(k), (what, "get on held paths", k.hex())
                    else:
                        assert g is UNKNOWN, (what, "get under a stub", k.hex())
                assert f.stubs > 0 or set(nodes) == set(step["witness"]), (what, "stubs")
                f.fill(nodes)
                assert f.stubs == 0, (what, "stubs after the fill")
            # after every step
            want = {t: ms[t].root() for t in resident if ms[t].live}
            got = f.roots()
            assert {t: r for t, r in got.items() if r != EMPTY} == want, (what, "roots()")
            assert all(t in F.FOREST_IDS for t in got), (what, "roots() names an unknown trie")
            assert len(f) == sum(len(ms[t]) for t in resident), (what, "len")
            assert f.savepoint_depth() == step["depth"], (what, "savepoint depth")
            q = step["probe"]
            assert f.get(q) == [ms[t].t.get(k) if t in resident else None for t, k in q], (what, "get")
            if op == "prove":
                q = [(t, k) for t, k in q if t in resident]
                found, proofs = f.prove(q)
                want = [proof_ref.expected_proof(ms[t].nodes(), ms[t].root(), k) for t, k in q]
                assert found == [v is not None for _, v in want] and proofs == [p for p, _ in want], (what, "proofs")
                status, vals = verify_proofs([ms[t].root() for t, _ in q], [k for _, k in q], proofs)
                assert status == [_lib.KH_PROOF_VALUE if v is not None else _lib.KH_PROOF_ABSENT for _, v in want]
                assert vals == [v for _, v in want], (what, "verify_proofs")
        assert i == F.NSTEPS
    finally:
        f.close()
        ctx.close()
