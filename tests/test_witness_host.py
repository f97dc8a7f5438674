"""CPU: the KH_HD bodies of khipu_amd/csrc/witness.h (the commit witness: the walk of an op, the
visited set, the deletes' set, the judgement of a visited branch) replayed on the host under
AddressSanitizer and UBSan.  tests/witness_host/witness_check.cc (a stand-alone program) loads the
records through load.h's rounds and runs the driver's passes into arrays of exactly the sizes the
library gives them.  Every expectation is tests/witness_ref.expected (node encodings and key sets
alone) or a hand-made answer of tests/witness_cases."""
import subprocess

import pytest

from tests import cases as C
from tests import fuzz_cases as F
from tests import hostprog
from tests import partial_cases as P
from tests import witness_cases as WC
from tests import witness_ref
from tests import writeback as W
from tests.hostprog import trie as _trie

prog = hostprog.prog_fixture("witness")


def _run(prog, tmp_path, store, tries, ups, dels):
    """ups / dels: [(trie id, key)] -> (witness [(trie, hash)] in table order or None,
    n_collapse, reached [(trie, hash)], moved [(trie, hash)])"""
    lines = [f"N {e.hex()}" for e in store] + [f"T {t} {r.hex()}" for t, r in tries]
    lines += [f"U {t} {k.hex()}" for t, k in ups] + [f"D {t} {k.hex()}" for t, k in dels]
    p = tmp_path / "in.txt"
    p.write_text("\n".join(lines) + "\n")
    r = subprocess.run([prog, str(p)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])  # (a sanitizer report: a non-zero status)
    out = [ln.split() for ln in r.stdout.split("\n")[:-1]]
    assert out[0] == ["S", "0"], out[0]

    def pairs(tag):
        return [(int(x[1]), bytes.fromhex(x[2])) for x in out if x[0] == tag]
    reached, moved = pairs("R"), pairs("M")
    c = next(x for x in out if x[0] == "C")
    return (None if reached or moved else pairs("W")), int(c[1]), reached, moved


def _check(prog, tmp_path, nodes, root, live, ups, dels, tag):
    """The replay's witness of the batch on the full store equals the reference's."""
    want, ncol = witness_ref.expected(nodes, root, live, [k for k, _ in ups], dels)
    got, n, reached, moved = _run(prog, tmp_path, list(nodes.values()), [(0, root)], [(0, k) for k, _ in ups],
                                  [(0, k) for k in dels])
    assert not reached and not moved, tag
    assert len(got) == len(set(got)), tag  # each node once
    assert {h for _, h in got} == want, tag
    assert n == ncol, tag
    return n


@pytest.mark.parametrize("case", WC.hand_cases(), ids=lambda c: c[0])
def test_host_hand_cases(prog, tmp_path, oracle, case):
    name, ks, vs, ups, dels, cover, ncol = case
    o = _trie(oracle, ks, vs)
    nodes, root = o.reachable(), o.root_hash()
    assert _check(prog, tmp_path, nodes, root, ks, ups, dels, name) == ncol
    got, *_ = _run(prog, tmp_path, list(nodes.values()), [(0, root)], [(0, k) for k, _ in ups], [(0, k) for k in dels])
    assert {h for _, h in got} == WC.want(nodes, root, cover)


@pytest.mark.parametrize("name", ["storage", "deep", "same_key_batch"])
def test_host_commit_scenarios(prog, tmp_path, oracle, name):
    _, ks, vs, batches = next(s for s in C.commit_scenarios() if s[0] == name)
    o = _trie(oracle, ks, vs)
    live = set(ks)
    for i, (ups, dels) in enumerate(batches):
        _check(prog, tmp_path, W.reachable(o), o.root_hash(), live, ups, dels, (name, i))
        for k, v in ups:
            o.put(k, v)
        for k in dels:
            o.remove(k)
        live = (live | {k for k, _ in ups}) - set(dels)


def test_host_dense_key_sequence(prog, tmp_path, oracle):
    pre, ncommit = None, 0
    for i, step, m in F.trie_run(F.TRIE_SEEDS[0], oracle, nsteps=30):
        if step["op"] == "commit" and not step["refused"] and pre[1] != W.EMPTY_TRIE_HASH:
            _check(prog, tmp_path, *pre, step["ups"], step["dels"], i)
            ncommit += 1
        pre = (dict(W.reachable(m.t)), m.root(), set(m.live))
    assert ncommit >= 3


def test_host_two_tries_and_an_absent_id(prog, tmp_path, oracle):
    """The same keys in two tries of one store: a node both hold is listed once per trie; an id the
    store does not list adds nothing; a key deleted in one trie only collapses that one."""
    o = _trie(oracle, [WC.A, WC.B], WC.V[:2])
    nodes, root = o.reachable(), o.root_hash()
    hA, hB = (P.path_hashes(nodes, root, k)[0][-1] for k in (WC.A, WC.B))
    got, n, *_ = _run(prog, tmp_path, list(nodes.values()), [(3, root), (9, root)],
                      [(9, WC.A), (5, WC.C)], [(3, WC.A), (5, WC.A)])
    assert sorted(got) == sorted([(3, root), (3, hA), (3, hB), (9, root), (9, hA)]) and n == 1


def test_host_partial_handles(prog, tmp_path, oracle):
    """Stubs: a walk that reaches one lists it (and nothing is judged); a collapse onto a stub of
    unknown kind lists it; onto the missing branch under a present extension it lists nothing and
    the extension is in the witness."""
    o = _trie(oracle, [WC.A, WC.B], WC.V[:2])
    nodes, root = o.reachable(), o.root_hash()
    hA, hB = (P.path_hashes(nodes, root, k)[0][-1] for k in (WC.A, WC.B))
    got, _, reached, moved = _run(prog, tmp_path, [nodes[root]], [(0, root)], [(0, WC.B)], [(0, WC.A), (0, WC.A2)])
    assert got is None and sorted(reached) == sorted([(0, hA), (0, hB)]) and not moved
    got, _, reached, moved = _run(prog, tmp_path, [nodes[root], nodes[hA]], [(0, root)], [], [(0, WC.A)])
    assert got is None and not reached and moved == [(0, hB)]
    got, n, reached, moved = _run(prog, tmp_path, [nodes[root], nodes[hA]], [(0, root)], [(0, WC.C)], [(0, WC.A)])
    assert {h for _, h in got} == {root, hA} and n == 0  # (the slot filled: no collapse)
    # the sibling an extension whose branch the store lacks
    _, ks, vs, *_ = next(c for c in WC.hand_cases() if c[0] == "sibling_extension")
    o = _trie(oracle, ks, vs)
    nodes, root = o.reachable(), o.root_hash()
    hA = P.path_hashes(nodes, root, WC.A)[0][-1]
    ext = P.path_hashes(nodes, root, WC.B)[0][1]
    got, n, reached, moved = _run(prog, tmp_path, [nodes[root], nodes[hA], nodes[ext]], [(0, root)], [], [(0, WC.A)])
    assert {h for _, h in got} == {root, hA, ext} and n == 1 and not reached and not moved
    # ... and with the extension withheld too: a stub of unknown kind
    got, n, reached, moved = _run(prog, tmp_path, [nodes[root], nodes[hA]], [(0, root)], [], [(0, WC.A)])
    assert got is None and moved == [(0, ext)]
