"""CPU: the partial load and the fill of khipu_amd/csrc/load.h (stubs: forest.h EL_STUB) replayed
on the host under AddressSanitizer and UBSan.  tests/partial_host/partial_check.cc (a stand-alone
program) replays the rounds into arrays of exactly the scanned sizes, builds an anchor map over the
records, re-encodes every non-stub record through export.h and runs the get, need and prove walks.
Every expectation is the oracle's: reachable() minus the subtrees withheld, the child items of the
nodes that are there, and tests/proof_ref.expected_proof."""
import random
import subprocess

import pytest

from tests import cases as C
from tests import export_cases, hostprog, proof_cases, proof_ref
from tests.hostprog import rlp_list as _lst
from tests.hostprog import rlp_str as _s
from tests.hostprog import trie as _trie
from tests.hostprog import vb_trie as _vb_trie
from tests.partial_cases import hash_children as _hash_children
from tests.partial_cases import subtree as _subtree

OK, MISSING, BAD, VALUE = 0, 1, 2, 3  # forest.h OPEN_*


prog = hostprog.prog_fixture("partial")


class Out:
    def __init__(self, lines, pfx):
        rows = [x for x in lines if x and x[0].startswith(pfx) and x[0][len(pfx):] in ("S", "B", "E")]
        s = next(x for x in rows if x[0] == pfx + "S")
        names = (("code", "rounds", "records", "keys", "heap", "decoded", "stubs") if pfx else
                 ("code", "rounds", "records", "keys", "heap", "n_missing", "stubs"))
        self.s = dict(zip(names, map(int, s[1:])))
        # stubs: (trie, anchor depth, depth of the missing node, rref, rbref)
        self.stubs = [(int(x[1]), int(x[2]), int(x[3]), bytes.fromhex(x[4]), bytes.fromhex(x[5]))
                      for x in rows if x[0] == pfx + "B"]
        self.nodes = {}
        for x in rows:
            if x[0] == pfx + "E":
                per = self.nodes.setdefault(int(x[1]), {})
                h = bytes.fromhex(x[2])
                assert h not in per, "a node emitted twice for one trie"
                per[h] = bytes.fromhex(x[3])


def _run(prog, tmp_path, store, tries, fill=None, queries=()):
    """-> (Out after the load, Out after the fill or None, [(idx, hash)] missing roots,
    [(found, need, [proof hashes])] per query, deterministic)"""
    lines = [f"N {e.hex()}" for e in store] + [f"T {t} {r.hex()}" for t, r in tries]
    lines += [f"Q {t} {k.hex()}" for t, k in queries]
    if fill is not None:
        lines += [f"F {e.hex()}" for e in fill] or ["F -"]
    p = tmp_path / "in.txt"
    p.write_text("\n".join(lines) + "\n")
    r = subprocess.run([prog, str(p)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])  # (a sanitizer report: a non-zero status)
    out = [ln.split() for ln in r.stdout.split("\n")[:-1]]
    miss = [(int(x[1]), bytes.fromhex(x[2])) for x in out if x[0] == "M"]
    g = [(int(x[2]), None if x[3] == "-" else bytes.fromhex(x[3]), [bytes.fromhex(h) for h in x[5:]])
         for x in out if x[0] == "G"]
    for x in out:
        if x[0] == "G":
            assert int(x[4]) == len(x[5:])
    det = [x for x in out if x[0] == "D"][0][1] == "1"
    after = Out(out, "F") if any(x[0] == "FS" for x in out) else None
    return Out(out, ""), after, miss, g, det


def _random_tries(oracle):
    """The construction of test_load_host.py::test_host_missing_nodes_are_listed_exactly."""
    r = random.Random(13)
    tr = []
    for n in (200, 150, 90):
        ks = [C._rk(r) for _ in range(n)]
        tr.append((_trie(oracle, ks, [C.account_value(r) for _ in ks]), ks))
    return tr


def test_host_one_depth2_node_withheld_then_filled(prog, tmp_path, oracle):
    tr = _random_tries(oracle)
    full = {}
    for o, _ in tr:
        full.update(o.reachable())
    tries = [(10 + j, o.root_hash()) for j, (o, _) in enumerate(tr)]
    o1, keys1 = tr[1]
    enc = o1.reachable()
    root = enc[o1.root_hash()]
    child = next(c for c in _hash_children(root))
    grand = next(c for c in _hash_children(enc[child]))
    assert sum(1 for e in full.values() if grand in e) == 1  # (referenced once)
    gone = _subtree(enc, grand)
    store = [e for h, e in full.items() if h != grand]
    # queries: every key of trie 1, and one absent key
    queries = [(11, k) for k in keys1] + [(11, b"\x5a" * 32)]
    a, b, miss, g, det = _run(prog, tmp_path, store, tries, fill=list(full.values()), queries=queries)
    assert a.s["code"] == OK and not miss and det
    assert a.s["stubs"] == 1 and [(t, rb) for t, _, _, _, rb in a.stubs] == [(11, grand)]
    t, ad, md, rref, rbref = a.stubs[0]
    assert ad == md == 2 and rref == rbref == grand
    assert a.nodes[10] == tr[0][0].reachable() and a.nodes[12] == tr[2][0].reachable()
    assert a.nodes[11] == {h: e for h, e in enc.items() if h not in gone}
    # keys: every leaf but those of the withheld subtree
    lost = [k for k in keys1 if any(proof_ref.kec(e) in gone for e in proof_ref.expected_proof(enc, o1.root_hash(), k)[0])]
    assert lost and a.s["keys"] == 200 + 150 + 90 - len(lost)
    # get / need / prove: unknown exactly where the oracle's walk needs a withheld node
    for (_, k), (found, need, proof) in zip(queries, g):
        want, val = proof_ref.expected_proof(enc, o1.root_hash(), k)
        wh = [proof_ref.kec(e) for e in want]
        if any(h in gone for h in wh):
            assert found == 2 and need == grand
            assert proof == wh[:wh.index(grand)]  # the resident prefix
        else:
            assert found == (1 if val is not None else 0) and need is None and proof == wh
    # after a fill with the full store: everything, and no stub
    assert b.s["code"] == OK and b.s["stubs"] == 0 and not b.stubs
    assert b.s["decoded"] == len(gone)
    assert b.nodes == {10: tr[0][0].reachable(), 11: enc, 12: tr[2][0].reachable()}
    assert b.s["keys"] == 200 + 150 + 90


def test_host_root_only_store(prog, tmp_path, oracle):
    o, _ = _random_tries(oracle)[0]
    enc = o.reachable()
    root = enc[o.root_hash()]
    a, _, miss, _, det = _run(prog, tmp_path, [root], [(4, o.root_hash())])
    assert a.s["code"] == OK and not miss and det and a.s["keys"] == 0
    kids = _hash_children(root)
    assert len(kids) == 16  # (200 random keys: a full root branch of hashed children)
    assert sorted(rb for _, _, _, _, rb in a.stubs) == sorted(kids)
    assert all(ad == md == 1 and rr == rb for _, ad, md, rr, rb in a.stubs)
    assert a.nodes == {4: {o.root_hash(): root}}
    # a fill with the second level only: each child resolved, its own children stubs again
    level2 = [enc[h] for h in kids]
    _, b, _, _, _ = _run(prog, tmp_path, [root], [(4, o.root_hash())], fill=level2)
    assert b.s["code"] == OK and b.s["decoded"] == 16
    want_stubs = sorted(c for h in kids for c in _hash_children(enc[h]))
    assert sorted(rb for _, _, _, _, rb in b.stubs) == want_stubs and b.s["stubs"] == len(want_stubs)
    assert b.nodes == {4: {h: enc[h] for h in [o.root_hash()] + kids}}


def test_host_missing_root_is_still_a_missing_node(prog, tmp_path, oracle):
    tr = _random_tries(oracle)
    full = {}
    for o, _ in tr:
        full.update(o.reachable())
    tries = [(10 + j, o.root_hash()) for j, (o, _) in enumerate(tr)]
    store = [e for h, e in full.items() if h != tr[2][0].root_hash()]
    a, _, miss, _, _ = _run(prog, tmp_path, store, tries)
    assert a.s["code"] == MISSING and a.s["records"] == 0 and a.s["keys"] == 0 and not a.nodes and not a.stubs
    assert miss == [(2, tr[2][0].root_hash())]


def test_host_extension_whose_branch_is_missing(prog, tmp_path, oracle):
    ek, ev, queries = proof_cases.ext_case()
    o = _trie(oracle, ek, ev)
    enc = o.reachable()
    root = enc[o.root_hash()]
    assert len(export_cases._items(root)) == 2  # the root extension
    (branch,) = _hash_children(root)
    q = [(0, ek[0]), (0, queries[0])]
    a, b, _, g, det = _run(prog, tmp_path, [root], [(0, o.root_hash())], fill=list(enc.values()), queries=q)
    assert a.s["code"] == OK and det and a.s["keys"] == 0
    assert a.stubs == [(0, 0, 10, o.root_hash(), branch)]  # one stub at anchor 0: rref the root, rbref the branch
    assert a.nodes == {0: {o.root_hash(): root}}  # (the stub still stands for the extension)
    # a key under the extension needs the branch; one leaving the path inside it is absent, as in
    # the oracle's walk (expected_proof lists the extension alone)
    assert proof_ref.expected_proof(enc, o.root_hash(), queries[0]) == ([root], None)
    assert [(f, n, p) for f, n, p in g] == [(2, branch, [o.root_hash()]), (0, None, [o.root_hash()])]
    assert b.s["code"] == OK and b.s["stubs"] == 0 and b.nodes == {0: enc} and b.s["keys"] == len(ek)


def test_host_embedded_nodes_are_never_stubs(prog, tmp_path, oracle):
    keys, vals = export_cases.embedded_case()
    o = _trie(oracle, keys, vals)
    want = o.reachable()
    assert export_cases.holds_embedded_child(want)
    a, b, miss, _, det = _run(prog, tmp_path, list(want.values()), [(7, o.root_hash())], fill=list(want.values()))
    assert a.s["code"] == OK and not miss and det and a.s["stubs"] == 0 and not a.stubs
    assert a.nodes == {7: want} and a.s["keys"] == len(set(keys))
    assert b.s["code"] == OK and b.s["decoded"] == 0 and b.nodes == {7: want} and b.s["records"] == a.s["records"]


def test_host_value_only_branch_leaves_no_stub(prog, tmp_path, oracle):
    o, nkeys = _vb_trie(oracle)
    want = o.reachable()
    a, _, _, _, det = _run(prog, tmp_path, list(want.values()), [(3, o.root_hash())])
    assert a.s["code"] == OK and det and a.s["keys"] == nkeys and a.s["stubs"] == 0
    assert a.nodes == {3: want}


def test_host_fill_with_a_malformed_node_two_rounds_down(prog, tmp_path, oracle):
    """The fill store resolves a stub, that node's child too, and below it holds a bad node: the two
    rounds before it had appended records; the handle is as before the fill."""
    o, _ = _random_tries(oracle)[0]
    enc = dict(o.reachable())
    root = enc[o.root_hash()]
    kid = _hash_children(root)[0]
    gkid = _hash_children(enc[kid])[0]
    node = enc[gkid]  # (a branch or a leaf two levels down; a branch is needed: take one that has children)
    cands = [(k, g) for k in _hash_children(root) for g in _hash_children(enc[k]) if _hash_children(enc[g])]
    kid, gkid = cands[0]
    node = enc[gkid]
    victim = _hash_children(node)[0]
    bad = _lst([_s(b"\x31" + b"\x11" * 32), _s(b"value" * 8)])  # a leaf whose path runs past nibble 64
    at = node.index(victim)
    node2 = node[:at] + oracle.kec256(bad) + node[at + 32:]
    par = enc[kid]
    at = par.index(gkid)
    par2 = par[:at] + oracle.kec256(node2) + par[at + 32:]
    at = root.index(kid)
    root2 = root[:at] + oracle.kec256(par2) + root[at + 32:]
    a, b, _, _, _ = _run(prog, tmp_path, [root2], [(0, oracle.kec256(root2))], fill=[par2, node2, bad])
    assert a.s["code"] == OK and a.s["stubs"] == 16
    assert b.s["code"] == BAD and b.s["rounds"] == 2
    assert b.s["stubs"] == 16 and b.s["records"] == a.s["records"] and b.s["keys"] == 0
    assert b.nodes == a.nodes and sorted(b.stubs) == sorted(a.stubs)


def test_host_two_partial_loads_of_a_shuffled_store_agree(prog, tmp_path, oracle):
    tr = _random_tries(oracle)
    full = {}
    for o, _ in tr:
        full.update(o.reachable())
    r = random.Random(21)
    store = [e for h, e in full.items() if r.random() < 0.6 or h in [o.root_hash() for o, _ in tr]]
    tries = [(10 + j, o.root_hash()) for j, (o, _) in enumerate(tr)]
    a, _, _, _, det = _run(prog, tmp_path, store, tries)
    r.shuffle(store)
    d1 = tmp_path / "b"
    d1.mkdir()
    b, _, _, _, det2 = _run(prog, d1, store, tries)
    assert a.s["code"] == OK and det and det2 and a.s["stubs"] > 0
    assert a.s == b.s and a.stubs == b.stubs and a.nodes == b.nodes  # (the same records in the same order)
    # what is held is a subset of the oracle's nodes, and every stub names a node that was withheld
    have = {proof_ref.kec(e) for e in store}
    for t, (o, _) in zip((10, 11, 12), tr):
        assert set(a.nodes[t]) <= set(o.reachable())
        assert all(e == o.reachable()[h] for h, e in a.nodes[t].items())
    assert all(rb not in have for _, _, _, _, rb in a.stubs)
