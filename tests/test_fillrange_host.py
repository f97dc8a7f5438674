"""CPU: the span test of khipu_amd/csrc/fillrange.h and the order check a range fill shares with
range verification, replayed on the host under AddressSanitizer and UBSan
(tests/fillrange_host/fillrange_check.cc, a stand-alone program run as a child process) and
compared with the model (tests/fillrange_ref.py) over the shapes of tests/fillrange_cases.py."""
import random
import subprocess

import pytest

from tests import fillrange_cases as FC
from tests import fillrange_ref as F
from tests import hostprog
from tests import proof_ref as P
from tests.hostprog import hexs as _hex

prog = hostprog.prog_fixture("fillrange")


def _pad(nib, fill=0):
    n = list(nib) + [fill] * (64 - len(nib))
    return bytes((n[2 * i] << 4) | n[2 * i + 1] for i in range(32))


def _run(prog, tmp_path, lines):
    p = tmp_path / "in.txt"
    p.write_text("\n".join(lines) + "\n")
    r = subprocess.run([prog, str(p)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])  # (a sanitizer report ends it with a non-zero status)
    out = [ln.split() for ln in r.stdout.split("\n")[:-1]]
    assert len(out) == len(lines)
    return out


@pytest.fixture(scope="module")
def state(oracle):
    items = FC.crafted()
    o = oracle.Trie()
    for k, v in items:
        o.put(k, v)
    return items, o.reachable(), o.root_hash()


def test_span_test_matches_the_model(prog, tmp_path, state):
    items, nodes, root = state
    r = random.Random(9)
    cases = []  # (prefix nibbles, origin, hi)
    # every stub of a sync in pages of 7, before each page, against that page's span and the open one
    held = {root}
    for origin in FC.walk_origins(items, 7, FC.EXT_ORIGIN)[:6] + FC.walk_origins(items, 7)[:12]:
        keys, vals, proof, _ = FC.page(items, nodes, root, origin, 7)
        held = F.fill_nodes(nodes, root, held, proof)
        for p, _ in F.stubs(nodes, root, held):
            cases += [(p, origin, keys[-1]), (p, origin, FC.FF)]
        held = F.fill_range(nodes, root, held, origin, keys, vals).held
    # every prefix length, at, just inside and just outside both ends of a span
    for md in range(65):
        p = [r.randrange(16) for _ in range(md)]
        lo, hi = _pad(p, 0), _pad(p, 15)
        cases += [(p, lo, hi), (p, FC.ZERO, FC.FF), (p, lo, FC.FF), (p, FC.ZERO, hi)]
        if lo != FC.FF:
            cases.append((p, FC.step(lo), FC.FF))
        if hi != FC.ZERO:
            cases.append((p, FC.ZERO, FC.step(hi, -1)))
    lines = [f"S {_pad(p).hex()} {len(p)} {lo.hex()} {hi.hex()}" for p, lo, hi in cases]
    got = _run(prog, tmp_path, lines)
    seen = set()
    for (p, lo, hi), x in zip(cases, got):
        want = F.inside(list(p), P.nibbles(lo), P.nibbles(hi))
        assert x[0] == "I" and x[1] == str(int(want)), (p, lo.hex(), hi.hex())
        assert x[2] == _pad(p, 15).hex()
        seen.add(want)
    assert seen == {True, False} and len(cases) > 300


def test_order_check_matches_the_model(prog, tmp_path, state):
    items, nodes, root = state
    r = random.Random(10)
    ranges = []
    for origin in FC.walk_origins(items, 7)[:10]:
        keys, vals, _, _ = FC.page(items, nodes, root, origin, 7)
        ranges.append((origin, keys, vals))
        ranges += [(origin, mk, mv) for _, mk, mv, _ in FC.mutations(r, items, origin, keys, vals, r.randrange(1, 6))]
    ranges += [(FC.ZERO, [], []), (FC.FF, [FC.FF], [b"\x01"]), (FC.FF, [FC.step(FC.FF, -1)], [b"\x01"])]
    lines = [f"R {o.hex()} {len(ks)}" + "".join(f" {k.hex()} {_hex(v)}" for k, v in zip(ks, vs)) for o, ks, vs in ranges]
    got = _run(prog, tmp_path, lines)
    bad = 0
    for (o, ks, vs), x in zip(ranges, got):
        want = F.whole(b"", ks, vs) == F.BAD_ORDER or bool(ks and ks[0] < o)
        assert x == ["O", str(int(want))], (o.hex(), len(ks))
        bad += want
    assert 10 <= bad < len(ranges)
