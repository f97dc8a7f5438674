"""CPU: the subtree eviction of khipu_amd/csrc/load.h replayed on the host under AddressSanitizer
and UBSan.  tests/evict_host/evict_check.cc (a stand-alone program) loads the tries with the load
replay, then runs the probe, the flag pass with its predecessor search, the delete and the stub
rewrite through the KH_HD bodies the kernels call, and re-encodes what is left through export.h.
Every expectation is the reference's (tests/evict_ref.py over the oracle's node sets)."""
import random
import subprocess

import pytest

from khipu_amd import codec
from tests import cases as C
from tests import evict_ref as E
from tests import export_cases, hostprog, partial_cases, path_ref

prog = hostprog.prog_fixture("evict")


def _run(prog, tmp_path, store, tries, prefixes):
    """-> None when the list is refused, else (statuses [(status, hash or None)], counters, stubs
    [(trie, anchor depth, node depth, rref, rbref, key)], {trie: {hash: encoding}})"""
    lines = [f"N {e.hex()}" for e in store] + [f"T {t} {r.hex()}" for t, r in tries]
    lines += [f"P {t} {len(p)} {codec.nibbles_to_path32(p).hex()}" for t, p in prefixes]
    tmp_path.mkdir(exist_ok=True)
    p = tmp_path / "in.txt"
    p.write_text("\n".join(lines) + "\n")
    r = subprocess.run([prog, str(p)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])  # (a sanitizer report: a non-zero status)
    out = [ln.split() for ln in r.stdout.split("\n")[:-1]]
    if out[0] == ["X", "1"]:
        assert len(out) == 1
        return None
    status = [(int(x[2]), bytes.fromhex(x[3]) if int(x[2]) in (E.DONE, E.STUB) else None) for x in out if x[0] == "V"]
    assert all(x[3] == "00" * 32 for x in out if x[0] == "V" and int(x[2]) in (E.NONE, E.EMBEDDED))
    c = next(x for x in out if x[0] == "C")
    cnt = dict(zip(("evicted", "keys", "records", "stubs", "size"), map(int, c[1:])))
    stubs = [(int(x[1]), int(x[2]), int(x[3])) + tuple(bytes.fromhex(h) for h in x[4:7]) for x in out if x[0] == "B"]
    nodes = {}
    for x in out:
        if x[0] == "E":
            per = nodes.setdefault(int(x[1]), {})
            assert bytes.fromhex(x[2]) not in per, "a node emitted twice for one trie"
            per[bytes.fromhex(x[2])] = bytes.fromhex(x[3])
    return status, cnt, stubs, nodes


def _check(prog, tmp_path, states, prefixes, nkeys):
    """states {trie: (nodes held, root)}; prefixes [(trie, nibbles)]: everything the program prints
    against the reference run per trie."""
    store = {}
    for nodes, _ in states.values():
        store.update(nodes)
    got = _run(prog, tmp_path, list(store.values()), [(t, root) for t, (_, root) in states.items()], prefixes)
    assert got is not None
    status, cnt, stubs, left = got
    want_status = [None] * len(prefixes)
    total = dict(evicted=0, keys=0, records=0, stubs=0)
    evs = {}
    for t in sorted({t for t, _ in prefixes} | set(states)):
        nodes, root = states.get(t, ({}, None))
        idx = [i for i, (tt, _) in enumerate(prefixes) if tt == t]
        ev = evs[t] = E.evict(nodes, root, [prefixes[i][1] for i in idx])
        assert not (ev["held"] & ev["removed"])
        for i, s in zip(idx, ev["status"]):
            want_status[i] = s
        total["evicted"] += ev["evicted"]
        total["keys"] += len(ev["keys"])
        total["records"] += ev["records"]
        total["stubs"] += len(ev["stubs"])
        assert left.get(t, {}) == {h: nodes[h] for h in ev["held"]}, t
        assert sorted(rb for tt, _, _, _, rb, _ in stubs if tt == t) == ev["stubs"], t
    assert status == want_status
    assert cnt == dict(total, size=nkeys - total["keys"])
    # a stub made by the eviction: plain, at the prefix, its key zero past it
    made = {(t, p): h for (t, p), (s, h) in zip(prefixes, status) if s == E.DONE}
    by_anchor = {(t, tuple(codec.path32_to_nibbles(k, a))): (a, d, rr, rb, k) for t, a, d, rr, rb, k in stubs}
    for (t, p), h in made.items():
        assert by_anchor[(t, tuple(p))] == (len(p), len(p), h, h, codec.nibbles_to_path32(p))
    return status, evs


@pytest.fixture(scope="module")
def forest(oracle):
    """Three random tries (ids 10..12) and a fourth id with the first one's content."""
    r = random.Random(13)
    st, n = {}, 0
    for t, k in ((10, 200), (11, 150), (12, 90)):
        ks = [C._rk(r) for _ in range(k)]
        o = hostprog.trie(oracle, ks, [C.account_value(r) for _ in ks])
        st[t] = (o.reachable(), o.root_hash())
        n += k
    st[13] = st[10]
    return st, n + 200


def _hung(state, depth):
    return sorted(p for p in E.queries(*state)["hung"] if len(p) == depth)


def test_host_siblings_list_ends_and_a_shared_prefix(prog, tmp_path, forest):
    st, nkeys = forest
    top10, top12 = _hung(st[10], 1), _hung(st[12], 1)
    d2 = _hung(st[11], 2)
    sib = next((a, b) for a in d2 for b in d2 if a[0] == b[0] and a[1] + 1 == b[1])
    # trie 10's records under nibbles below top10[3] sort before every listed prefix, trie 12's
    # above top12[-2] and all of trie 13's after; (10, top10[3]) is the list's first entry, (12,
    # top12[-2]) its last; trie 13 shares every prefix with trie 10 and is not listed
    prefixes = [(12, top12[-2]), (11, sib[1]), (10, top10[3]), (11, sib[0])]
    assert top10[3][0] >= 3 and top12[-2][0] < 15
    status, evs = _check(prog, tmp_path, st, prefixes, nkeys)
    assert [s for s, _ in status] == [E.DONE] * 4
    assert evs[13]["evicted"] == 0 and evs[10]["evicted"] == 1


def test_host_a_trie_not_held_and_every_none_cause(prog, tmp_path, forest):
    st, nkeys = forest
    q = E.queries(*st[11], seed=3)
    leaf_p = next(p for p in q["below_leaf"] if len(p) >= 2)
    prefixes = [(11, q["empty_slot"][0]), (11, leaf_p), (99, (1,)), (12, _hung(st[12], 1)[0] + (0,) * 63)]
    status, _ = _check(prog, tmp_path, st, prefixes, nkeys)
    assert [s for s, _ in status] == [E.NONE] * 4


def test_host_stubs_at_below_and_inside(prog, tmp_path, forest):
    """A partial store: a prefix at a stub, one below a stub, and a subtree that holds stubs."""
    st, _ = forest
    nodes, root = st[10]
    sp = path_ref.stored_paths(nodes, root)
    d2 = [(p, h) for p, h in sp if len(p) == 2]
    gone = {h for p, h in d2 if p[0] in (2, 5)}  # every depth-2 node under the top nibbles 2 and 5
    held, _ = partial_cases.held({h: e for h, e in nodes.items() if h not in gone}, root)
    part = {h: nodes[h] for h in held}
    at = [p for p, h in d2 if p[0] == 5]
    nkeys = sum(1 for h in part if path_ref.decode(part[h])[0] == "leaf")
    prefixes = [(10, (2,)), (10, at[0]), (10, at[1] + (7,))]
    status, evs = _check(prog, tmp_path, {10: (part, root)}, prefixes, nkeys)
    assert [s for s, _ in status] == [E.DONE, E.STUB, E.NONE] and evs[10]["stubs_died"] >= 2


@pytest.mark.parametrize("case", ["embedded", "deep", "vb"])
def test_host_shapes(prog, tmp_path, oracle, case):
    if case == "embedded":
        ks, vs = export_cases.embedded_case()
        o, nkeys = hostprog.trie(oracle, ks, vs), len(set(ks))
    elif case == "deep":
        name, ks, _, _ = C.commit_scenarios()[2]
        o, nkeys = hostprog.trie(oracle, ks, [bytes([i + 1]) * 40 for i in range(len(ks))]), len(ks)
    else:
        o, nkeys = hostprog.vb_trie(oracle)
    state = (o.reachable(), o.root_hash())
    q = E.queries(*state, seed=5)
    r = random.Random(5)
    for rnd in range(3):
        pool = [p for k in sorted(q) for p in q[k]]
        r.shuffle(pool)
        first = {"embedded": q["embedded"][:2], "vb": [p for p in q["hung"] if len(p) == 64][:1],
                 "deep": [p for p in q["hung"] if path_ref.decode(state[0][dict(path_ref.stored_paths(*state))[p]])[0] == "ext"][:1]}
        assert first[case]
        chosen = E.antichain(first[case] + pool)[:25]
        status, _ = _check(prog, tmp_path / str(rnd), {0: state}, [(0, p) for p in chosen], nkeys)
        assert status[0][0] == (E.EMBEDDED if case == "embedded" else E.DONE)


def test_host_nested_and_equal_prefixes_are_refused(prog, tmp_path, forest):
    st, _ = forest
    store = list(st[10][0].values()) + list(st[11][0].values())
    tries = [(10, st[10][1]), (11, st[11][1])]
    a = _hung(st[10], 1)[0]
    for bad in ([(10, a), (10, a)], [(10, a), (11, (3,)), (10, a + (4,))], [(10, a + (0, 0)), (10, (9,)), (10, a + (0,))]):
        assert _run(prog, tmp_path, store, tries, bad) is None
    assert _run(prog, tmp_path, store, tries, [(10, a), (11, a)]) is not None  # (one prefix in two tries)
