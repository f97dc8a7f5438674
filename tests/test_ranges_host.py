"""CPU: the batched range scan of khipu_amd/csrc/range.h replayed on the host under
AddressSanitizer and UBSan.  tests/ranges_host/ranges_check.cc (a stand-alone program) builds the
records of several tries bottom-up into one store and runs the rounds as range_kernels.hip's
k_ranges_* do -- one map_find a request, then count, scan and a 16-lane fill into a segmented
frontier cut at exactly max_entries + 2 * nq items, lengths, fit, write into outputs of exactly
the scanned sizes.  Every answer must equal tests/ranges_ref.expected_ranges over the oracle's
nodes; and with the cut one item smaller an input built to need the full cut must come out wrong.

Tries: 1-key tries, ten-key tries, one 300-key trie, embedded nodes, an extension at the root, a
value-only branch, and range_cases.dense_case keys with origins one nibble above and limits one
nibble below present keys at the split depths (both boundary items of a request empty at once)."""
import random
import subprocess

import pytest

from tests import cases as C
from tests import fuzz_cases as F
from tests import hostprog
from tests import range_cases as RC
from tests import ranges_ref as BR
from tests.hostprog import hexs as _hex
from tests.hostprog import unhexs as _unhex
from tests.test_range_host import _case

NQS = [1, 2, 3, 16, 17]
MAXES = [1, 2, 15, 16, 17, 255, 256, 257]  # either side of the fill's 16 items a block and the count's 256
BIG = 1 << 30
UNHELD = 999

prog = hostprog.prog_fixture("ranges")


def _run(prog, tmp_path, forest, batches, less=0):
    """forest: {id: puts [(key, value, makes a value-only branch)]}; batches: [(requests [(id, origin,
    limit)], max_entries, val_cap)] -> ({id: root}, [answer in the form of expected_ranges], [rounds])"""
    lines = []
    for t, puts in forest.items():
        lines.append(f"T {t}")
        lines += [f"{'B' if vb else 'P'} {k.hex()} {_hex(v)}" for k, v, vb in puts]
    for reqs, mx, cap in batches:
        lines.append(f"Q {mx} {cap} {less}")
        lines += [f"R {t} {(o or RC.ZERO).hex()} {(l or RC.FF).hex()}" for t, o, l in reqs]
    p = tmp_path / f"in{less}.txt"
    p.write_text("\n".join(lines) + "\n")
    r = subprocess.run([prog, str(p)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])  # (a sanitizer report ends the program non-zero)
    out = [ln.split() for ln in r.stdout.split("\n")[:-1]]
    roots = {int(x[1]): bytes.fromhex(x[2]) for x in out if x[0] == "T"}
    ans, rounds = [], []
    for (reqs, _, _), x in zip(batches, [x for x in out if x[0] == "A"]):
        nq = len(reqs)
        if x[1] == "pages":
            k, n_done = int(x[2]), int(x[3])
            eo = [int(e) for e in x[6:7 + nq]]
            ents = x[7 + nq:]
            assert len(ents) == 2 * k and eo[0] == 0 and eo[nq] == k and eo == sorted(eo)
            keys, vals = [bytes.fromhex(e) for e in ents[0::2]], [_unhex(e) for e in ents[1::2]]
            ans.append(("pages", [(keys[eo[q]:eo[q + 1]], vals[eo[q]:eo[q + 1]]) for q in range(nq)], n_done,
                        _unhex(x[4]) if n_done < nq else None))
            rounds.append(int(x[5]))
        elif x[1] == "nospc":
            ans.append(("nospc", int(x[2])))
        else:
            ans.append(("missing", bytes.fromhex(x[2]), int(x[3])))
    assert len(ans) == len(batches)
    return roots, ans, rounds


def _ten(r):
    ks = [C._rk(r) for _ in range(10)]
    return [(k, C.storage_value(r), False) for k in ks]


@pytest.fixture(scope="module")
def forest(oracle):
    """({id: puts}, {id: (nodes, root)}, {id: sorted keys}, the dense trie's id and Keys)"""
    r = random.Random(17)
    puts = {}
    for t, name in ((1, "one_key"), (2, "random300"), (3, "embedded"), (4, "extension"), (5, "value_only_branch"),
                    (70000, "dense")):
        puts[t] = _case(name, oracle)[0]
    puts[6] = [(C._rk(r), b"\x33" * 33, False)]
    for t in (7, 8, 9, 1 << 31):
        puts[t] = _ten(r)
    puts[10] = []  # an empty trie
    tries, keys = {}, {}
    for t, ps in puts.items():
        o = oracle.Trie()
        for k, v, _ in ps:
            o.put(k, v)
        root = o.root_hash()
        tries[t] = (o.reachable() if ps else {}, root)
        keys[t] = sorted({k for k, _, _ in ps})
    return puts, tries, keys


def _dense_requests(r, keys, n):
    """n requests of the dense trie: origin one nibble above a present key and limit one nibble
    below a present key, each at a split depth."""
    _, _, K, _ = RC.dense_case()
    out = []
    while len(out) < n:
        k1, k2 = sorted(r.sample(keys, 2))
        n1, n2 = F.nibbles(k1), F.nibbles(k2)
        p1, p2 = r.choice(K.P), r.choice(K.P)
        if n1[p1] == 15 or n2[p2] == 0:
            continue
        n1[p1] += 1
        n2[p2] -= 1
        out.append((70000, F.from_nibbles(n1), F.from_nibbles(n2)))  # (origin > limit now and then: empty)
    return out


def _batches(forest, seed):
    _, _, keys = forest
    r = random.Random(seed)
    ids = list(keys)
    out = []
    for nq in NQS:
        for mx in MAXES:
            for rep in range(3):
                reqs = []
                for _ in range(nq):
                    x = r.random()
                    t = UNHELD if x < 0.06 else reqs[-1][0] if (reqs and x < 0.2) else 2 if x < 0.35 else r.choice(ids)
                    a, b, _ = RC.random_ranges(r, keys.get(t, []), 1)[0]
                    if r.random() < 0.35:
                        a = b = None
                    reqs.append((t, a, b))
                if rep == 2:
                    reqs = _dense_requests(r, keys[70000], nq)
                out.append((reqs, mx, BIG))
    return out


def test_host_batches_match_the_reference(prog, tmp_path, forest):
    puts, tries, _ = forest
    batches = _batches(forest, 1)
    roots, got, rounds = _run(prog, tmp_path, puts, batches)
    assert roots == {t: root for t, (_, root) in tries.items()}
    for (reqs, mx, cap), g in zip(batches, got):
        assert g == BR.expected_ranges(tries, reqs, mx, cap), (len(reqs), mx)
    assert max(rounds) <= 66
    cut = [g for g in got if g[2] < len(g[1])]
    assert len(cut) >= 20 and len(got) - len(cut) >= 20
    assert any(not g[1][g[2]][0] for g in cut) and any(g[1][g[2]][0] for g in cut)


def test_host_val_cap(prog, tmp_path, forest):
    """val_cap at exactly the bytes of the first k entries of a batch, one less, the first value, one
    less than it, and 0."""
    puts, tries, _ = forest
    reqs = [(7, None, None), (10, None, None), (2, None, None), (8, None, None)]
    full = BR.expected_ranges(tries, reqs, 40)
    vals = [v for _, vs in full[1] for v in vs]
    assert len(vals) == 40 and full[2] == 2
    total, first = sum(len(v) for v in vals), len(vals[0])
    ten = sum(len(v) for v in vals[:10])
    batches = [(reqs, 40, cap) for cap in (total, total - 1, ten, ten - 1, first, first - 1, 0)]
    _, got, _ = _run(prog, tmp_path, puts, batches)
    assert got == [BR.expected_ranges(tries, *b) for b in batches]
    n = [sum(len(ks) for ks, _ in g[1]) if g[0] == "pages" else None for g in got]
    assert n == [40, 39, 10, 9, 1, None, None]
    assert got[2][2] == 2 and not got[2][1][2][0]  # (cut at the first entry of the request after the empty one)
    assert got[5] == got[6] == ("nospc", first)


def test_host_empty_batches(prog, tmp_path, forest):
    puts, tries, keys = forest
    k = keys[1][0]
    batches = [([(10, None, None)], 5, 100), ([(UNHELD, None, None), (10, None, None)], 5, 100),
               ([(1, RC.FF, RC.ZERO), (1, RC._step(k, 1), None), (1, None, RC._step(k, -1))], 5, 100)]
    _, got, _ = _run(prog, tmp_path, puts, batches)
    assert got == [("pages", [([], [])] * len(b[0]), len(b[0]), None) for b in batches]
    _, got, _ = _run(prog, tmp_path, {10: []}, batches[:2])  # a store without a record
    assert got == [("pages", [([], [])] * len(b[0]), len(b[0]), None) for b in batches[:2]]


def _needs_the_full_cut(nq):
    """A trie whose root branch holds 16 leaves, asked nq times for (leaf 0, leaf 15) exclusive: after
    the first round every request has 14 items holding an entry between two boundary items that
    turn out empty.  With max_entries one less than the 14 * nq entries, the entry `next` comes
    from lies under item max_entries + 2 * nq."""
    ks = [bytes([(c << 4) | 8]) + b"\x88" * 31 for c in range(16)]
    puts = [(k, bytes([c + 1]) * 5, False) for c, k in enumerate(ks)]
    reqs = [(3, RC._step(ks[0], 1), RC._step(ks[15], -1))] * nq
    return puts, ks, (reqs, 14 * nq - 1, BIG)


@pytest.mark.parametrize("nq", [1, 2, 3, 17])
def test_a_cut_one_item_smaller_is_seen(prog, tmp_path, forest, oracle, nq):
    """The library's cut answers the constructed input and the dense batches; a frontier cut at
    max_entries + 2 * nq - 1 items loses the item that holds thing max_entries + 1 of the
    constructed input (the answer then claims to be complete)."""
    puts, ks, b = _needs_the_full_cut(nq)
    o = oracle.Trie()
    for k, v, _ in puts:
        o.put(k, v)
    tries = {3: (o.reachable(), o.root_hash())}
    want = BR.expected_ranges(tries, *b)
    assert want[2] == nq - 1 and want[3] == ks[14]
    _, got, _ = _run(prog, tmp_path, {3: puts}, [b])
    assert got == [want]
    _, got, _ = _run(prog, tmp_path, {3: puts}, [b], less=1)
    assert got != [want] and got[0][2] == nq
    if nq == 17:  # the dense batches through the smaller cut as well: no fault, and they count what they see
        fp, ft, _ = forest
        batches = [x for x in _batches(forest, 1) if x[0][0][0] == 70000 and x[0][0][1] is not None]
        _, got, _ = _run(prog, tmp_path, fp, batches, less=1)
        wrong = sum(1 for x, g in zip(batches, got) if g != BR.expected_ranges(ft, *x))
        print("dense batches wrong under the smaller cut:", wrong, "of", len(batches))
