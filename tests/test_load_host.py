"""CPU: the forest load of khipu_amd/csrc/load.h replayed on the host under AddressSanitizer and
UBSan.  tests/load_host/load_check.cc (a stand-alone program) takes a node store and a list of
(trie id, root), replays the rounds -- count, scan, fill -- into arrays of exactly the scanned
sizes, builds an anchor map over the records and re-encodes every record through export.h.  Each
trie's node set must equal the oracle's reachable() bit for bit; missing nodes must be listed
exactly; malformed nodes must give their error code and leave nothing behind."""
import random
import subprocess

import pytest

from tests import cases as C
from tests import export_cases, hostprog, proof_cases
from tests.hostprog import rlp_list as _lst
from tests.hostprog import rlp_str as _s
from tests.hostprog import trie as _trie
from tests.hostprog import vb_trie as _vb_trie

EMPTY = bytes.fromhex("56e81f171bcc55a6ff8345e692c0f86e5b48e01b996cadc001622fb5e363b421")
OK, MISSING, BAD, VALUE = 0, 1, 2, 3  # forest.h OPEN_*


prog = hostprog.prog_fixture("load")


def _run(prog, tmp_path, store, tries):
    """store: [encoding]; tries: [(id, root)] -> (status dict, [(idx, hash)], {id: {hash: enc}}, deterministic)"""
    lines = [f"N {e.hex()}" for e in store] + [f"T {t} {r.hex()}" for t, r in tries]
    p = tmp_path / "in.txt"
    p.write_text("\n".join(lines) + "\n")
    r = subprocess.run([prog, str(p)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]  # (a sanitizer report ends the program with a non-zero status)
    out = [ln.split() for ln in r.stdout.split("\n")[:-1]]
    s = dict(zip(("code", "rounds", "records", "keys", "heap", "n_missing"), map(int, out[0][1:])))
    miss = [(int(x[1]), bytes.fromhex(x[2])) for x in out if x[0] == "M"]
    nodes = {}
    for x in out:
        if x[0] == "E":
            per = nodes.setdefault(int(x[1]), {})
            h = bytes.fromhex(x[2])
            assert h not in per, "a node emitted twice for one trie"
            per[h] = bytes.fromhex(x[3])
    det = [x for x in out if x[0] == "D"]
    return s, miss, nodes, det[0][1] == "1"


def _cases(oracle):
    r = random.Random(5)
    ks = [C._rk(r) for _ in range(300)]
    rnd = (ks, [C.storage_value(r) if i % 3 else C.account_value(r) for i, _ in enumerate(ks)])
    ek, ev, _ = proof_cases.ext_case()
    return {"one_key": ([C._rk(r)], [b"\x07" * 40]), "random300": rnd, "embedded": export_cases.embedded_case(),
            "extension": (ek, ev)}


@pytest.mark.parametrize("name", ["one_key", "random300", "embedded", "extension"])
def test_host_load_gives_the_oracles_nodes(prog, tmp_path, oracle, name):
    keys, vals = _cases(oracle)[name]
    o = _trie(oracle, keys, vals)
    want = o.reachable()
    s, miss, nodes, det = _run(prog, tmp_path, list(want.values()), [(7, o.root_hash())])
    assert s["code"] == OK and not miss and det
    assert s["keys"] == len(set(keys))
    assert nodes == {7: want}
    if name == "embedded":
        assert export_cases.holds_embedded_child(want)


def test_host_value_only_branch(prog, tmp_path, oracle):
    o, nkeys = _vb_trie(oracle)
    want = o.reachable()
    # (the construction does make one: a 17-item node whose 16 children are empty)
    assert any(len(export_cases._items(e)) == 17 and all(m == 0 for _, _, m in export_cases._items(e)[:16])
               for e in want.values())
    s, _, nodes, det = _run(prog, tmp_path, list(want.values()), [(3, o.root_hash())])
    assert s["code"] == OK and det and s["keys"] == nkeys
    assert nodes == {3: want}


def test_host_two_ids_one_root_duplicates_and_strangers(prog, tmp_path, oracle):
    r = random.Random(9)
    ka = [C._rk(r) for _ in range(120)]
    a = _trie(oracle, ka, [C.storage_value(r) for _ in ka])
    kb = [C._rk(r) for _ in range(40)]
    b = _trie(oracle, kb, [bytes([r.randrange(1, 0x80)]) for _ in kb])
    stranger = _trie(oracle, [C._rk(r) for _ in range(30)], [C.account_value(r) for _ in range(30)])
    store = list(a.reachable().values()) + list(b.reachable().values())
    store = store + store[::3] + list(stranger.reachable().values())  # duplicates and unrelated nodes
    r.shuffle(store)
    tries = [(5, a.root_hash()), (1 << 31 | 9, b.root_hash()), (6, a.root_hash()), (8, EMPTY)]
    s, miss, nodes, det = _run(prog, tmp_path, store, tries)
    assert s["code"] == OK and not miss and det
    assert s["keys"] == 2 * len(ka) + len(kb)
    assert nodes == {5: a.reachable(), 6: a.reachable(), (1 << 31 | 9): b.reachable()}  # (the empty root: nothing)


def test_host_missing_nodes_are_listed_exactly(prog, tmp_path, oracle):
    r = random.Random(13)
    tr = []
    for n in (200, 150, 90):
        ks = [C._rk(r) for _ in range(n)]
        tr.append(_trie(oracle, ks, [C.account_value(r) for _ in ks]))
    full = {}
    for o in tr:
        full.update(o.reachable())
    tries = [(10 + j, o.root_hash()) for j, o in enumerate(tr)]
    # two roots absent: round 0 reports exactly those (list index, hash)
    store = [e for h, e in full.items() if h not in (tr[0].root_hash(), tr[2].root_hash())]
    s, miss, nodes, _ = _run(prog, tmp_path, store, tries)
    assert s["code"] == MISSING and s["records"] == 0 and s["keys"] == 0 and s["heap"] == 0 and not nodes
    assert sorted(miss) == sorted([(0, tr[0].root_hash()), (2, tr[2].root_hash())])
    # one depth-2 node absent: a hash child of a hash child of trie 1's root
    enc = tr[1].reachable()
    root_items = export_cases._items(enc[tr[1].root_hash()])
    child = next(enc[tr[1].root_hash()][q:q + m] for l, q, m in root_items[:16] if not l and m == 32)
    it2 = export_cases._items(enc[child])
    grand = next(enc[child][q:q + m] for l, q, m in it2[:16] if not l and m == 32)
    assert sum(1 for e in full.values() if grand in e) == 1  # (referenced once)
    s, miss, nodes, _ = _run(prog, tmp_path, [e for h, e in full.items() if h != grand], tries)
    assert s["code"] == MISSING and s["rounds"] == 2 and s["records"] == 0 and not nodes
    assert miss == [(1, grand)]


def malformed_roots():
    """(name, root node encoding, the OPEN_* code it must give): each >= 32 B, loaded as a trie's root."""
    e = b"\x80"
    h = _s(b"\x77" * 32)
    return [("branch_value_at_depth_0", _lst([h, h] + [e] * 14 + [_s(b"v" * 40)]), VALUE),
            ("child_string_of_33_bytes", _lst([_s(b"\x33" * 33)] + [e] * 15 + [e]), BAD),
            ("leaf_path_too_long", _lst([_s(b"\x31" + b"\x11" * 32), _s(b"value" * 8)]), BAD),
            ("leaf_path_too_short", _lst([_s(b"\x20" + b"\x11" * 31), _s(b"value" * 8)]), BAD),
            ("embedded_child_of_32_bytes", _lst([_lst([_s(b"\x20" + b"\x11" * 20), _s(b"\x22" * 8)])] + [e] * 16), BAD),
            ("hp_flag_4", _lst([_s(b"\x40" + b"\x11" * 32), _s(b"value" * 8)]), BAD),
            ("three_items", _lst([_s(b"\x20" + b"\x11" * 32), _s(b"ab" * 9), _s(b"cd" * 9)]), BAD),
            ("byte_string", _s(b"\x05" * 40), BAD)]


@pytest.mark.parametrize("name,enc,code", malformed_roots(), ids=[n for n, _, _ in malformed_roots()])
def test_host_malformed_nodes_leave_nothing(prog, tmp_path, oracle, name, enc, code):
    assert len(enc) >= 32
    r = random.Random(3)
    ks = [C._rk(r) for _ in range(60)]
    good = _trie(oracle, ks, [C.account_value(r) for _ in ks])
    store = list(good.reachable().values()) + [enc]
    s, miss, nodes, det = _run(prog, tmp_path, store, [(1, good.root_hash()), (2, oracle.kec256(enc))])
    assert s["code"] == code, name
    assert s["records"] == 0 and s["keys"] == 0 and s["heap"] == 0 and not nodes and not miss and det


def test_host_malformed_node_below_the_root(prog, tmp_path, oracle):
    """A bad node two rounds down: the rounds before it had written records, all of them cleared."""
    r = random.Random(4)
    ks = [C._rk(r) for _ in range(300)]
    o = _trie(oracle, ks, [C.account_value(r) for _ in ks])
    enc = dict(o.reachable())
    root = enc[o.root_hash()]
    _, q, m = next(it for it in export_cases._items(root)[:16] if not it[0] and it[2] == 32)
    bad = _lst([_s(b"\x31" + b"\x11" * 32), _s(b"value" * 8)])  # a leaf whose path runs past nibble 64
    root2 = root[:q] + oracle.kec256(bad) + root[q + m:]
    store = [e for h, e in enc.items() if h != o.root_hash()] + [root2, bad]
    s, _, nodes, _ = _run(prog, tmp_path, store, [(0, oracle.kec256(root2))])
    assert s["code"] == BAD and s["rounds"] == 1 and s["records"] == 0 and not nodes
