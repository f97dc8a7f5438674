"""GPU: Merkle proofs of a resident trie or forest (kh_trie_prove) and their verification
(kh_verify_proofs), bit-exact against tests/proof_ref.py over the oracle's reachable(): the proof
of a key is the list of nodes MerklePatriciaTrie.get visits, root first, restricted to the nodes a
node store holds."""
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

from tests import cases as C
from tests import export_cases, proof_cases
from tests import proof_ref as P

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMPTY = P.EMPTY_ROOT


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


def _check(t, o, keys, unique=False, tag=None):
    """prove(keys), plain and shared, against expected_proof over o; returns the proofs."""
    root, nodes = o.root_hash(), _nodes(o)
    want = [P.expected_proof(nodes, root, k)[0] for k in keys]
    found, proofs = t.prove(keys)
    assert proofs == want, tag
    assert found == [o.get(k) is not None for k in keys], tag
    found2, proofs2, table = t.prove(keys, shared=True)
    assert proofs2 == want and found2 == found, tag
    union = {e for p in want for e in p}
    assert set(table.nodes) == union, tag
    assert all(P.kec(e) == h for h, e in zip(table.hashes, table.nodes)), tag
    if unique:
        assert len(table.nodes) == len(union), tag
    return proofs


@pytest.mark.parametrize("i", range(len(C.commit_scenarios())), ids=[s[0] for s in C.commit_scenarios()])
def test_prove_after_commits(khst, oracle, i):
    from khipu_amd.device import Ctx, ResidentTrie
    name, ks, vs, batches = C.commit_scenarios()[i]
    r = random.Random(100 + i)
    o = _oracle(oracle, ks, vs)
    live = dict(zip(ks, vs))
    gone = []
    t = ResidentTrie(Ctx(0), ks, vs, emit=False)
    for b in range(len(batches) + 1):
        if b:
            ups, dels = batches[b - 1]
            _fold(o, ups, dels)
            assert t.commit(ups, dels) == o.root_hash(), (name, b)
            live.update(ups)
            for k in dels:
                live.pop(k, None)
                gone.append(k)
        present = r.sample(list(live), min(len(live), 40))
        keys = present + list(dict.fromkeys(gone)) + [C._rk(r) for _ in range(20)]
        if present:
            keys += proof_cases.near_misses(r, present)
        _check(t, o, keys, unique=name in ("accounts", "storage", "large_batch", "same_key_batch"), tag=(name, b))
    t.close()


@pytest.mark.parametrize("n", [1, 17, 257])
def test_prove_key_counts(khst, oracle, n):
    """Key counts across the 16-records-per-block and 256-threads-per-block edges of the kernels."""
    from khipu_amd.device import Ctx, ResidentTrie
    r = random.Random(300)
    ks = [C._rk(r) for _ in range(300)]
    vs = [C.account_value(r) for _ in ks]
    o = _oracle(oracle, ks, vs)
    t = ResidentTrie(Ctx(0), ks, vs, emit=False)
    _check(t, o, ks[:n], unique=True)
    t.close()


def test_prove_embedded_nodes(khst, oracle):
    from khipu_amd.device import Ctx, ResidentTrie
    ks, vs = export_cases.embedded_case()
    o = _oracle(oracle, ks, vs)
    assert export_cases.holds_embedded_child(o.reachable())
    t = ResidentTrie(Ctx(0), ks, vs, emit=False)
    r = random.Random(4)
    proofs = _check(t, o, ks + [k for k in proof_cases.near_misses(r, ks, 16) if k not in set(ks)])
    for k, p in zip(ks, proofs):  # the depth-64 leaf is embedded: the proof ends at the last hashed ancestor
        assert len(export_cases._items(p[-1])) == 17
        assert P.check_proof(o.root_hash(), k, p) == (P.VALUE, o.get(k))
    t.close()


@pytest.mark.parametrize("small", [False, True], ids=["hashed", "inline"])
def test_prove_value_only_branch(khst, oracle, small):
    from khipu_amd.device import Ctx, ResidentTrie, verify_proofs
    ks, vs, blocks, kk = proof_cases.vb_case(small)
    o = _oracle(oracle, ks, vs)
    t = ResidentTrie(Ctx(0), ks, vs, emit=False)
    for b, (ups, dels) in enumerate(blocks):
        _fold(o, ups, dels)
        assert t.commit(ups, dels) == o.root_hash(), b
        proofs = _check(t, o, list(kk), tag=b)
        st, vals = verify_proofs(o.root_hash(), kk, proofs)
        assert vals == [o.get(k) for k in kk] and st == [int(v is not None) for v in vals], b
    t.close()


def test_prove_extension_divergence(khst, oracle):
    from khipu_amd.device import Ctx, ResidentTrie
    ks, vs, queries = proof_cases.ext_case()
    o = _oracle(oracle, ks, vs)
    t = ResidentTrie(Ctx(0), ks, vs, emit=False)
    proofs = _check(t, o, queries + ks[:5])
    assert [len(p) for p in proofs[:3]] == [1, 1, 1]  # the extension is listed, nothing below it
    t.close()


def _forest(khst, oracle):
    """60 tries over 4 blocks with hashed 32-byte slots (the shape of test_gpu_export.py's), twin
    tries holding the same slot and value, and one trie emptied by deletes."""
    from khipu_amd.device import Ctx, ResidentForest
    r = random.Random(78)
    f = ResidentForest(Ctx(0), hash_keys=True, emit=False)
    tries, live = {}, {}
    ids = [r.randrange(1 << 32) for _ in range(60)]
    twins = [r.randrange(1 << 32) for _ in range(2)]
    emptied = ids[0]
    for blk in range(4):
        ups, dels = [], []
        for t in r.sample(ids[1:], 25):
            have = live.get(t, [])
            for _ in range(r.choice([1, 3, 10, 40])):
                slot = bytes(r.getrandbits(8) for _ in range(32)) if not have or r.random() < 0.6 else r.choice(have)
                ups.append((t, slot, C.storage_value(r)))
            if have and r.random() < 0.5:
                for slot in r.sample(have, min(len(have), r.choice([1, 5]))):
                    dels.append((t, slot))
        if blk == 0:
            ups += [(emptied, bytes([i]) * 32, C.storage_value(r)) for i in range(5)]
        if blk == 1:
            dels += [(emptied, bytes([i]) * 32) for i in range(5)]
        if blk == 2:
            ups += [(twins[0], b"\x11" * 32, b"\x01" * 40), (twins[1], b"\x11" * 32, b"\x01" * 40)]
        got = f.commit(ups, dels)
        for t, slot, v in ups:
            tries.setdefault(t, oracle.Trie()).put(oracle.kec256(slot), v)
            live[t] = list(dict.fromkeys(live.get(t, []) + [slot]))
        for t, slot in dels:
            tries[t].remove(oracle.kec256(slot))
            live[t] = [s for s in live[t] if s != slot]
        for t in got:
            assert got[t] == tries[t].root_hash(), (blk, t)
    return f, tries, live, twins, emptied


def test_prove_forest(khst, oracle):
    from khipu_amd.device import verify_proofs
    f, tries, live, twins, emptied = _forest(khst, oracle)
    r = random.Random(5)
    assert tries[emptied].root_hash() == EMPTY
    q = []
    for t in tries:
        for slot in r.sample(live[t], min(len(live[t]), 3)):
            q.append((t, slot))
        q.append((t, bytes(r.getrandbits(8) for _ in range(32))))
    q += [(twins[0], b"\x11" * 32), (twins[1], b"\x11" * 32), (0x7FFFFFFF, b"\x11" * 32), (emptied, b"\x00" * 32)]
    want, roots = [], []
    for t, slot in q:
        o = tries.get(t)
        root = o.root_hash() if o else EMPTY
        roots.append(root)
        want.append(P.expected_proof(_nodes(o) if o else {}, root, oracle.kec256(slot))[0])
    found, proofs = f.prove(q)
    assert proofs == want
    assert found == [t in tries and tries[t].get(oracle.kec256(s)) is not None for t, s in q]
    assert proofs[-1] == [] and proofs[-2] == [] and not found[-1] and not found[-2]
    found2, proofs2, table = f.prove(q, shared=True)
    assert proofs2 == want and found2 == found
    twin_root = tries[twins[0]].root_hash()
    assert sum(1 for h in table.hashes if h == twin_root) == 2  # one node, two tries: once per trie
    # verified with one root per key, plain and shared
    vals = f.get(q)
    for pt in (proofs, table):
        st, got = verify_proofs(roots, [s for _, s in q], pt, hash_keys=True)
        assert got == vals and st == [int(v is not None) for v in vals]
    f.close()


def test_prove_hash_keys(khst, oracle):
    from khipu_amd.device import Ctx, ResidentTrie, verify_proofs
    r = random.Random(20)
    ks = [bytes(r.getrandbits(8) for _ in range(20)) for _ in range(300)]
    vs = [C.account_value(r) for _ in ks]
    o = _oracle(oracle, [oracle.kec256(k) for k in ks], vs)
    t = ResidentTrie(Ctx(0), ks, vs, hash_keys=True, emit=False)
    q = ks[:30] + [bytes(r.getrandbits(8) for _ in range(20)) for _ in range(10)]
    found, proofs = t.prove(q)
    assert proofs == [P.expected_proof(o.reachable(), o.root_hash(), oracle.kec256(k))[0] for k in q]
    assert found == [True] * 30 + [False] * 10
    st, vals = verify_proofs(o.root_hash(), q, proofs, hash_keys=True)
    assert st == [1] * 30 + [0] * 10 and vals == vs[:30] + [None] * 10
    t.close()


def test_prove_empty_trie_and_no_keys(khst):
    from khipu_amd.device import Ctx, ResidentForest, ResidentTrie, verify_proofs
    t = ResidentTrie(Ctx(0), [], [], emit=False)
    assert t.prove([b"\x01" * 32]) == ([False], [[]])
    found, proofs, table = t.prove([b"\x01" * 32, b"\x02" * 32], shared=True)
    assert found == [False, False] and proofs == [[], []] and table.nodes == []
    assert t.prove([]) == ([], [])
    assert verify_proofs(EMPTY, [b"\x01" * 32], [[]]) == ([P.ABSENT], [None])
    assert verify_proofs(b"\x05" * 32, [b"\x01" * 32], [[]]) == ([P.SHORT], [None])
    assert verify_proofs(EMPTY, [], []) == ([], [])
    f = ResidentForest(Ctx(0))
    assert f.prove([(7, b"\x01" * 32)]) == ([False], [[]])
    t.close()
    f.close()


@pytest.mark.parametrize("shared", [False, True], ids=["plain", "shared"])
def test_prove_size_negotiation(khst, oracle, shared):
    from khipu_amd import _lib
    from khipu_amd.device import Ctx, ResidentTrie, trie_prove_raw
    r = random.Random(31)
    ks = [C._rk(r) for _ in range(300)]
    vs = [C.account_value(r) for _ in ks]
    t = ResidentTrie(Ctx(0), ks, vs, emit=False)
    q = ks[:40]
    rc, sizes, _ = trie_prove_raw(t.h, q, shared=shared, caps=(0, 0, 0))
    assert rc == _lib.KH_ENOSPC and all(s > 0 for s in sizes)
    nn, nb, npth = sizes
    assert (nn < npth) if shared else (nn == npth)
    rc, got, arrays = trie_prove_raw(t.h, q, shared=shared, caps=sizes)
    assert rc == _lib.KH_OK and got == sizes
    found, hs, rl, of, pi, po = arrays
    assert int(of[nn]) == nb and int(po[len(q)]) == npth and all(found[:len(q)])
    if not shared:
        assert list(pi[:npth]) == list(range(npth))
    for short in ((nn - 1, nb, npth), (nn, nb - 1, npth), (nn, nb, npth - 1)):
        rc, again, _ = trie_prove_raw(t.h, q, shared=shared, caps=short)
        assert rc == _lib.KH_ENOSPC and again == sizes, short
    t.close()


def test_prove_versions(khst, oracle):
    """savepoint, commit, prove: verifies under the new root; rollback, prove: under the old root
    and not under the new."""
    from khipu_amd.device import Ctx, ResidentTrie, verify_proofs
    r = random.Random(41)
    ks = [C._rk(r) for _ in range(300)]
    vs = [C.account_value(r) for _ in ks]
    o = _oracle(oracle, ks, vs)
    t = ResidentTrie(Ctx(0), ks, vs, emit=False)
    root0 = t.root
    t.savepoint()
    v1 = C.account_value(r)
    root1 = t.commit([(ks[3], v1)], [])
    o.put(ks[3], v1)
    assert root1 == o.root_hash() != root0
    _, proofs = t.prove([ks[3]])
    assert proofs == [P.expected_proof(o.reachable(), root1, ks[3])[0]]
    assert verify_proofs(root1, [ks[3]], proofs) == ([P.VALUE], [v1])
    t.rollback()
    _, proofs = t.prove([ks[3]])
    assert verify_proofs(root0, [ks[3]], proofs) == ([P.VALUE], [vs[3]])
    assert verify_proofs(root1, [ks[3]], proofs) == ([P.BAD_HASH], [None])
    t.close()


@pytest.fixture(scope="module")
def proved(khst, oracle):
    """A 300-key trie, proofs of 60 present and 20 absent keys (computed once, left unchanged)."""
    from khipu_amd.device import Ctx, ResidentTrie
    r = random.Random(51)
    ks = [C._rk(r) for _ in range(300)]
    vs = [C.storage_value(r) if i % 2 else C.account_value(r) for i in range(len(ks))]
    o = _oracle(oracle, ks, vs)
    t = ResidentTrie(Ctx(0), ks, vs, emit=False)
    q = ks[:60] + [C._rk(r) for _ in range(12)] + proof_cases.near_misses(r, ks[:60])
    found, proofs = t.prove(q)
    _, _, table = t.prove(q, shared=True)
    vals = t.get(q)
    t.close()
    return o.root_hash(), q, proofs, table, vals


def test_verify_round_trip(khst, proved):
    from khipu_amd.device import verify_proofs
    root, q, proofs, table, vals = proved
    for pt in (proofs, table):
        st, got = verify_proofs(root, q, pt)
        assert got == vals and st == [int(v is not None) for v in vals]
        st, got = verify_proofs([root] * len(q), q, pt)
        assert got == vals and st == [int(v is not None) for v in vals]


def test_verify_tampering(khst, proved):
    from khipu_amd import _lib
    from khipu_amd.device import verify_proofs
    root, q, proofs, _, vals = proved
    k, p = q[0], proofs[0]
    assert len(p) >= 3 and len(p[-1]) >= 32
    mid = p[1][:7] + bytes([p[1][7] ^ 0x40]) + p[1][8:]
    tampered = [[p[0], mid] + p[2:], p, p[:-1], p + [p[0]], p]
    roots = [root, b"\x13" * 32, root, root, root]
    st, got = verify_proofs(roots, [k] * 5, tampered)
    assert st == [_lib.KH_PROOF_BAD_HASH, _lib.KH_PROOF_BAD_HASH, _lib.KH_PROOF_SHORT, _lib.KH_PROOF_EXTRA,
                  _lib.KH_PROOF_VALUE]
    assert got == [None] * 4 + [vals[0]]
    bad = proof_cases.malformed_nodes()
    st, got = verify_proofs([P.kec(e) for _, e in bad], [b"\x11" * 32] * len(bad), [[e] for _, e in bad])
    assert st == [_lib.KH_PROOF_BAD_NODE] * len(bad), list(zip([n for n, _ in bad], st))
    # a path index equal to n_nodes
    from khipu_amd.device import ProofTable
    assert verify_proofs(root, [k], ProofTable([], p, [len(p)], [0, 1]))[0] == [_lib.KH_PROOF_BAD_NODE]
    # offsets that decrease are refused before anything is staged
    with pytest.raises(_lib.MPTException):
        verify_proofs(root, [k], ProofTable([], p, list(range(len(p))), [1, 0]))
    with pytest.raises(_lib.MPTException):
        verify_proofs([root] * 3, [k] * 5, [p] * 5)


def test_verify_mutations_match_the_checker(khst, proved):
    """300 seeded mutations of valid proofs -- a byte flip, a node dropped, two nodes swapped, a key
    bit flipped -- in one call: every status equals check_proof's."""
    from khipu_amd.device import verify_proofs
    root, q, proofs, _, _ = proved
    r = random.Random(61)
    keys, muts = [], []
    for m in range(300):
        i = r.randrange(len(q))
        key, p = q[i], list(proofs[i])
        op = m % 4
        if op == 0:
            j = r.randrange(len(p))
            b = bytearray(p[j])
            b[r.randrange(len(b))] ^= 1 << r.randrange(8)
            p[j] = bytes(b)
        elif op == 1:
            del p[r.randrange(len(p))]
        elif op == 2 and len(p) > 1:
            a, b = r.sample(range(len(p)), 2)
            p[a], p[b] = p[b], p[a]
        else:
            kb = bytearray(key)
            kb[r.randrange(32)] ^= 1 << r.randrange(8)
            key = bytes(kb)
        keys.append(key)
        muts.append(p)
    st, vals = verify_proofs(root, keys, muts)
    want = [P.check_proof(root, k, p) for k, p in zip(keys, muts)]
    assert list(zip(st, vals)) == want
    # (the mix is not one-sided: a flipped key bit leaves the path, a flipped byte breaks a hash, a
    # dropped last node leaves a reference open)
    assert {P.ABSENT, P.BAD_HASH, P.SHORT}.issubset(set(st)), set(st)


def test_prove_through_the_jni_shim(khst, oracle, tmp_path):
    """prove and verifyProofs through the in-process JNIEnv of tests/jni_stub: 400 keys, 40 proved
    (one of them absent), arrays that start too small so the grow path runs."""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    stub = os.path.join(ROOT, "tests", "jni_stub")
    exe = tmp_path / "jni_prove_driver"
    rc = subprocess.run([cc, "-std=gnu99", "-O1", "-Wall", "-Werror", "-I", stub, "-I", os.path.join(ROOT, "include"),
                         "-o", str(exe), os.path.join(stub, "jni_prove_driver.c"), os.path.join(stub, "fake_env.c"),
                         os.path.join(ROOT, "jni", "khst_jni.c"), "-L", os.path.join(ROOT, "khipu_amd"), "-lkhst",
                         "-Wl,-rpath," + os.path.join(ROOT, "khipu_amd"), "-Wl,-rpath-link,/opt/rocm/lib"],
                        capture_output=True, text=True)
    assert rc.returncode == 0, rc.stderr
    rnd = random.Random(808)
    keys = [C._rk(rnd) for _ in range(400)]
    vals = [C.account_value(rnd) for _ in keys]
    voff = np.zeros(len(vals) + 1, np.uint64)
    voff[1:] = np.cumsum([len(v) for v in vals])
    absent = C._rk(rnd)
    q = keys[:39] + [absent]
    p = tmp_path / "in.bin"
    with open(p, "wb") as f:
        f.write(np.uint32(32).tobytes() + np.uint64(len(keys)).tobytes())
        f.write(b"".join(keys) + voff.tobytes() + b"".join(vals))
        f.write(np.uint64(len(q)).tobytes() + b"".join(q))
    rc = subprocess.run([str(exe), str(p)], capture_output=True, text=True, timeout=120)
    assert rc.returncode == 0, rc.stderr
    lines = [ln.split() for ln in rc.stdout.split("\n")[:-1]]
    assert lines[-1] == ["E", "0"], lines[-1]
    o = _oracle(oracle, keys, vals)
    root, nodes = o.root_hash(), o.reachable()
    for shared in ("0", "1"):
        got = [x for x in lines if x[0] == "P" and x[1] == shared]
        assert len(got) == 40
        for k, x in zip(q, got):
            want, val = P.expected_proof(nodes, root, k)
            assert [bytes.fromhex(e) for e in x[5:]] == want and int(x[4]) == len(want)
            assert x[2] == ("1" if val is not None else "0")
            assert int(x[3]) == (P.VALUE if val is not None else P.ABSENT)
        grows = [int(x[2]) for x in lines if x[0] == "G" and x[1] == shared][0]
        assert grows >= 1
    vv = [None if x[2] == "-" else bytes.fromhex(x[2]) for x in lines if x[0] == "V"]
    assert vv == [o.get(k) for k in q]
