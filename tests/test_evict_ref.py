"""CPU: the subtree-eviction reference (tests/evict_ref.py) checks itself against the oracle's
reachable() node sets and key sets, and its query generator yields every status and every cause of
NONE on the inputs chosen for it."""
import random

import pytest

from tests import cases as C
from tests import evict_ref as E
from tests import export_cases, hostprog, partial_cases, path_ref, proof_cases, proof_ref

KIND_STATUS = {"hung": (E.DONE, None), "empty_slot": (E.NONE, "empty_slot"), "inside_ext": (E.NONE, "in_ext"),
               "ext_target": (E.NONE, "ext_target"), "below_leaf": (E.NONE, "in_leaf"), "embedded": (E.EMBEDDED, None)}


def _check_state(o, live):
    root = o.root_hash()
    nodes = o.reachable() if root != path_ref.EMPTY_ROOT else {}
    q = E.queries(nodes, root, seed=len(nodes))
    # every kind of query gets the status it was drawn for, and a hung prefix its node's hash
    at = dict(path_ref.stored_paths(nodes, root))
    for kind, ps in q.items():
        for p in ps:
            st, h, why, _ = E.locate(nodes, root, p)
            assert (st, why) == KIND_STATUS[kind], (kind, p)
            assert h == (at[p] if kind == "hung" else None)
    # one eviction of a drawn antichain over all kinds
    r = random.Random(len(nodes))
    pool = [p for ps in q.values() for p in ps]
    r.shuffle(pool)
    chosen = E.antichain(pool)[:40]
    ev = E.evict(nodes, root, chosen)
    done = [p for p, (st, _) in zip(chosen, ev["status"]) if st == E.DONE]
    assert ev["evicted"] == len(done)
    # the keys evicted are the keys of the state under a DONE prefix
    under = {k for k in live if any(tuple(proof_ref.nibbles(k)[:len(p)]) == p for p in done)}
    assert ev["keys"] == under
    # the nodes: the evicted subtrees are the oracle's node set minus what the rest still reaches
    for p, (st, h) in zip(chosen, ev["status"]):
        if st == E.DONE:
            assert partial_cases.subtree(nodes, h) <= ev["removed"]
    assert ev["held"] | ev["removed"] == set(nodes)
    if not (ev["held"] & ev["removed"]):  # (no evicted node is also referred to from what stays)
        assert ev["stubs"] == sorted(h for st, h in ev["status"] if st == E.DONE)
    assert ev["stubs_died"] == 0
    # a second eviction over the reduced set: the same prefixes are stubs, below them there is nothing
    part = {h: nodes[h] for h in ev["held"]}
    for p, (st, h) in zip(chosen, ev["status"]):
        if st == E.DONE:
            assert E.locate(part, root, p)[:3] == (E.STUB, h, None)
            if len(p) < 64:
                assert E.locate(part, root, p + (0,))[:3] == (E.NONE, None, "below_stub")


@pytest.mark.parametrize("i", range(len(C.commit_scenarios())), ids=[s[0] for s in C.commit_scenarios()])
def test_reference_on_commit_scenarios(oracle, i):
    name, ks, vs, batches = C.commit_scenarios()[i]
    o = hostprog.trie(oracle, ks, vs)
    live = set(ks)
    _check_state(o, live)
    for ups, dels in batches:
        for k, v in ups:
            o.put(k, v)
            live.add(k)
        for k in dels:
            o.remove(k)
            live.discard(k)
        _check_state(o, live)


def test_records_and_inner_stubs(oracle):
    """The record count of a subtree (a leaf, a branch with its extension, a stub: one each) and
    the stubs that die inside one."""
    r = random.Random(300)
    ks = [C._rk(r) for _ in range(300)]
    o = hostprog.trie(oracle, ks, [C.account_value(r) for _ in ks])
    root, nodes = o.root_hash(), o.reachable()
    hung = E.queries(nodes, root)["hung"]
    deep = max(hung, key=len)       # a leaf two or more branches down
    top = deep[:1]
    assert len(deep) >= 2 and top in hung
    leaves = [k for k in ks if proof_ref.nibbles(k)[0] == top[0]]
    ev = E.evict(nodes, root, [top])
    hs, keys, stubs, recs = E.subtree_stats(nodes, ("hash", ev["status"][0][1]), top)
    assert sorted(keys) == sorted(leaves) and not stubs
    # (accounts: no node is embedded) every node but an extension is a record
    exts = sum(1 for h in hs if path_ref.decode(nodes[h])[0] == "ext")
    assert recs == len(hs) - exts and ev["records"] == recs - 1
    # with the deep leaf withheld first, the top subtree holds one stub, and it dies with it
    part = {h: e for h, e in nodes.items() if h != dict(path_ref.stored_paths(nodes, root))[deep]}
    ev2 = E.evict(part, root, [top])
    assert ev2["stubs_died"] == 1 and ev2["records"] == ev["records"] and len(ev2["keys"]) == len(leaves) - 1
    assert ev2["stubs"] == [ev["status"][0][1]]


def test_kinds_occur(oracle):
    """Every status and every cause of NONE is present on the inputs chosen for it."""
    seen = set()

    def run(o, extra=()):
        root, nodes = o.root_hash(), o.reachable()
        q = E.queries(nodes, root)
        for ps in list(q.values()) + [list(extra)]:
            for p in ps:
                st, _, why, _ = E.locate(nodes, root, p)
                seen.add((st, why))
        return q, nodes, root

    ks, vs = export_cases.embedded_case()
    q, _, _ = run(hostprog.trie(oracle, ks, vs))
    assert q["embedded"]
    ek, ev, queries = proof_cases.ext_case()
    o = hostprog.trie(oracle, ek, ev)
    # off the extension: its target with the last nibble changed; off a leaf: a hung leaf's path
    # with one more, wrong nibble
    ext_t = E.queries(o.reachable(), o.root_hash())["ext_target"]
    q, nodes, root = run(o, [p[:-1] + (p[-1] ^ 1,) for p in ext_t])
    assert q["inside_ext"] and q["ext_target"]
    # an extension that hangs under a branch is evicted with its branch, as one stub
    name, ks, vs, _ = C.commit_scenarios()[2]
    assert name == "deep"
    o = hostprog.trie(oracle, ks, [bytes([i + 1]) * 40 for i in range(len(ks))])
    nodes, root = o.reachable(), o.root_hash()
    hung_ext = [p for p in E.queries(nodes, root)["hung"]
                if path_ref.decode(nodes[dict(path_ref.stored_paths(nodes, root))[p]])[0] == "ext"]
    assert hung_ext
    r = random.Random(300)
    ks = [C._rk(r) for _ in range(300)]
    o = hostprog.trie(oracle, ks, [C.account_value(r) for _ in ks])
    nodes, root = o.reachable(), o.root_hash()
    leaf_p = next(p for p, h in path_ref.stored_paths(nodes, root) if p and path_ref.decode(nodes[h])[0] == "leaf")
    leaf_nib = path_ref.decode(nodes[dict(path_ref.stored_paths(nodes, root))[leaf_p]])[1]
    q, _, _ = run(o, [leaf_p + (leaf_nib[0] ^ 1,)])
    assert q["empty_slot"] and q["below_leaf"] and q["hung"]
    # a stub, below a stub, and a trie that is not held
    h = dict(path_ref.stored_paths(nodes, root))[leaf_p[:1]]
    part = {k: v for k, v in nodes.items() if k != h}
    for p in (leaf_p[:1], leaf_p[:2]):
        st, _, why, _ = E.locate(part, root, p)
        seen.add((st, why))
    seen.add(E.locate({}, None, (1,))[0:3:2])
    o, _ = hostprog.vb_trie(oracle)
    run(o)
    assert {s for s, _ in seen} == {E.NONE, E.DONE, E.STUB, E.EMBEDDED}
    assert {w for s, w in seen if s == E.NONE} == set(E.CAUSES)


def test_held_extension_of_a_missing_branch_is_a_stub(oracle):
    ek, ev, _ = proof_cases.ext_case()
    # ext_case's extension is the root; put it under a branch with a second top nibble
    other = bytes([ek[0][0] ^ 0x80]) + b"\x33" * 31
    o = hostprog.trie(oracle, list(ek) + [other], list(ev) + [b"z" * 40])
    nodes, root = o.reachable(), o.root_hash()
    sp = dict(path_ref.stored_paths(nodes, root))
    ext_p = next(p for p, h in sp.items() if p and path_ref.decode(nodes[h])[0] == "ext")
    node = path_ref.decode(nodes[sp[ext_p]])
    assert node[2][0] == "hash"
    part = {k: v for k, v in nodes.items() if k != node[2][1]}
    assert E.locate(part, root, ext_p)[:3] == (E.STUB, node[2][1], None)
    assert E.locate(nodes, root, ext_p)[:3] == (E.DONE, sp[ext_p], None)
    assert E.locate(nodes, root, ext_p + tuple(node[1]))[:3] == (E.NONE, None, "ext_target")
