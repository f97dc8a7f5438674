"""CPU: the range scan of khipu_amd/csrc/range.h replayed on the host under AddressSanitizer and
UBSan.  tests/range_host/range_check.cc (a stand-alone program) builds a trie's records bottom-up
and runs the rounds as range_kernels.hip does -- count, scan, a 16-lane fill into a frontier cut at
max_entries + 2 items, lengths, fit, write into outputs of exactly the scanned sizes.  Every answer
must equal tests/range_ref.expected_range over the oracle's nodes; and the same inputs with the
cut at max_entries + 1 must disagree somewhere, so the inputs can see the cut."""
import random
import subprocess

import pytest

from tests import cases as C
from tests import export_cases, hostprog, proof_cases
from tests import range_cases as RC
from tests import range_ref as RR
from tests.hostprog import hexs as _hex
from tests.hostprog import unhexs as _unhex

NAMES = ["one_key", "random300", "embedded", "extension", "value_only_branch", "dense"]


prog = hostprog.prog_fixture("range")


def _run(prog, tmp_path, puts, ranges, slack=2):
    """puts: [(key, value, makes a value-only branch)]; ranges: [(origin, limit, max_entries, val_cap)]
    -> (root, [answer in the form of range_ref.expected_range], [rounds])"""
    lines = [f"{'B' if vb else 'P'} {k.hex()} {_hex(v)}" for k, v, vb in puts]
    lines += [f"R {(o or RC.ZERO).hex()} {(l or RC.FF).hex()} {mx} {cap} {slack}" for o, l, mx, cap in ranges]
    p = tmp_path / f"in{slack}.txt"
    p.write_text("\n".join(lines) + "\n")
    r = subprocess.run([prog, str(p)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]  # (a sanitizer report ends the program with a non-zero status)
    out = [ln.split() for ln in r.stdout.split("\n")[:-1]]
    assert out[0][0] == "T"
    ans, rounds = [], []
    for x in out[1:]:
        assert x[0] == "A"
        if x[1] == "page":
            k = int(x[2])
            ans.append(("page", [bytes.fromhex(e) for e in x[6:6 + 2 * k:2]], [_unhex(e) for e in x[7:7 + 2 * k:2]],
                        x[3] == "1", _unhex(x[4]) if x[3] == "1" else None))
            rounds.append(int(x[5]))
        elif x[1] == "nospc":
            ans.append(("nospc", int(x[2])))
        else:
            ans.append(("missing", bytes.fromhex(x[2])))
    assert len(ans) == len(ranges)
    return bytes.fromhex(out[0][1]), ans, rounds


def _case(name, oracle):
    """(puts for the program, oracle trie, ranges (origin, limit))"""
    r = random.Random(5)
    o = oracle.Trie()
    vbs = {}
    if name == "one_key":
        ks, vs = [C._rk(r)], [b"\x07" * 40]
    elif name == "random300":
        ks = [C._rk(r) for _ in range(300)]
        vs = [C.storage_value(r) if i % 3 else C.account_value(r) for i, _ in enumerate(ks)]
    elif name == "embedded":
        ks, vs = export_cases.embedded_case()
    elif name == "extension":
        ks, vs, _ = proof_cases.ext_case()
    elif name == "value_only_branch":
        ks, vs, blocks, _ = proof_cases.vb_case(False)
        vbs = dict(blocks[0][0])
    else:
        ks, vs, _, dense = RC.dense_case()
    for k, v in zip(ks, vs):
        o.put(k, v)
    for k, v in vbs.items():
        o.put(k, v)
    live = sorted(set(ks))
    made_vb = {k for k in vbs if any(x != k and x[:31] == k[:31] and x[31] >> 4 == k[31] >> 4 for x in live)}
    puts = [(k, v, False) for k, v in zip(ks, vs)] + [(k, v, k in made_vb) for k, v in vbs.items()]
    if name == "dense":
        ranges = [(a, b) for a, b, _ in dense]
    else:
        ranges = [(a, b) for a, b, _ in RC.random_ranges(r, live, 30)] + [(k, k) for k in live[:3]]
        if name == "extension":
            ranges += [(q, None) for q in proof_cases.ext_case()[2]] + [(None, q) for q in proof_cases.ext_case()[2]]
        if name == "value_only_branch":
            ranges += [(k, None) for k in made_vb] + [(None, k) for k in made_vb] + [(k, k) for k in made_vb]
            assert len(made_vb) == 2
    return puts, o, ranges


@pytest.mark.parametrize("name", NAMES)
def test_host_ranges_match_the_reference(prog, tmp_path, oracle, name):
    puts, o, ranges = _case(name, oracle)
    nodes, root = o.reachable(), o.root_hash()
    q = [(a, b, mx, 1 << 30) for a, b in ranges for mx in RC.HOST_MAXES]
    got_root, got, rounds = _run(prog, tmp_path, puts, q)
    assert got_root == root
    for (a, b, mx, cap), g in zip(q, got):
        assert g == RR.expected_range(nodes, root, a, b, mx, cap), (name, a and a.hex(), b and b.hex(), mx)
    assert max(rounds) <= 66
    assert any(g[1] for g in got) and (name == "one_key" or any(g[3] for g in got))


def test_host_val_cap(prog, tmp_path, oracle):
    """val_cap at exactly a page's bytes, one less, one less than the first value, and 0."""
    puts, o, _ = _case("random300", oracle)
    nodes, root = o.reachable(), o.root_hash()
    full = RR.expected_range(nodes, root, None, None, 64)
    total, first = sum(len(v) for v in full[2]), len(full[2][0])
    q = [(None, None, 64, cap) for cap in (total, total - 1, first, first - 1, 0)]
    _, got, _ = _run(prog, tmp_path, puts, q)
    assert got == [RR.expected_range(nodes, root, *x) for x in q]
    assert len(got[0][1]) == 64 and len(got[1][1]) == 63 and got[1][3] and len(got[2][1]) == 1
    assert got[3] == got[4] == ("nospc", first)


def test_host_empty_trie_and_empty_range(prog, tmp_path, oracle):
    _, got, _ = _run(prog, tmp_path, [], [(None, None, 5, 100)])
    assert got == [("page", [], [], False, None)]
    puts, o, _ = _case("one_key", oracle)
    k = puts[0][0]
    _, got, _ = _run(prog, tmp_path, puts, [(RC.FF, RC.ZERO, 5, 100), (RC._step(k, 1), None, 5, 100),
                                             (None, RC._step(k, -1), 5, 100)])
    assert got == [("page", [], [], False, None)] * 3


def test_a_cut_at_max_entries_plus_one_is_seen(prog, tmp_path, oracle):
    """The same inputs through a frontier cut at max_entries + 1 items: at least one answer is
    wrong (an item on origin's path that turns out empty takes the place of one that holds the
    entry `more` and `next` come from)."""
    wrong = 0
    for name in ("dense", "random300"):
        puts, o, ranges = _case(name, oracle)
        nodes, root = o.reachable(), o.root_hash()
        q = [(a, b, mx, 1 << 30) for a, b in ranges for mx in RC.HOST_MAXES]
        _, got, _ = _run(prog, tmp_path, puts, q, slack=1)
        wrong += sum(1 for x, g in zip(q, got) if g != RR.expected_range(nodes, root, *x))
    assert wrong >= 1
