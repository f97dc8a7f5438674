"""Inputs of the trie-diff tests, drawn by construction (tests/test_diff_ref.py pins their conditions
with the oracle alone; tests/test_diff_host.py and tests/test_gpu_diff.py run them).  No GPU, no
library."""
import bisect
import random

from tests import cases as C
from tests import export_cases, proof_cases
from tests import fuzz_cases as F
from tests import range_cases as RC
from tests.proof_ref import EMPTY_ROOT

ZERO, FF = RC.ZERO, RC.FF
HOST_MAXES = [1, 2, 3, 15, 16, 17, 63, 64, 65, 257]
SPAN = 3  # ordered pairs of states (i, j) with |i - j| <= SPAN


def vb_equal_value_scenario():
    """A re-put of k1 with the value it already has, under a depth-63 branch: khipu's value-only
    branch against a leaf of equal value, and nothing else changes."""
    ks, vs, _, (k1, _, _) = proof_cases.vb_case(False)
    return ("vb_equal_value", ks, vs, [([(k1, vs[ks.index(k1)])], [])])


def scenarios():
    """cases.commit_scenarios(), then khipu's value-only branch made, changed and left behind
    (proof_cases.vb_case) and made with an unchanged value."""
    ks, vs, blocks, _ = proof_cases.vb_case(False)
    return list(C.commit_scenarios()) + [("value_only_branch", ks, vs, blocks), vb_equal_value_scenario()]


def fold(o, ups, dels):
    for k, v in ups:
        o.put(k, v)
    for k in dels:
        o.remove(k)


def oracle_at(oracle, scen, upto):
    """The oracle's trie of scenario `scen` after its first `upto` batches."""
    _, ks, vs, batches = scen
    o = oracle.Trie()
    for k, v in zip(ks, vs):
        o.put(k, v)
    for b in batches[:upto]:
        fold(o, *b)
    return o


def states(oracle, scen):
    """[(nodes, root)] of every state of a scenario: one oracle trie folded batch by batch."""
    _, ks, vs, batches = scen
    o = oracle.Trie()
    for k, v in zip(ks, vs):
        o.put(k, v)
    out = [snap(o)]
    for b in batches:
        fold(o, *b)
        out.append(snap(o))
    return out


def snap(o):
    root = o.root_hash()
    return (o.reachable() if root != EMPTY_ROOT else {}, root)


def pairs(n):
    return [(i, j) for i in range(n) for j in range(n) if abs(i - j) <= SPAN]


def _nudge(k, p, d):
    n = F.nibbles(k)
    if not 0 <= n[p] + d <= 15:
        return None
    n[p] += d
    return F.from_nibbles(n)


def queries(r, diffs, per_kind=2):
    """(origin, limit, max_entries, val_cap) for a pair whose full difference list is `diffs`
    [(key, kind, value of b)]: origins and limits one nibble either side of a changed key of each
    kind, budgets that cut right before and right after the first difference of each kind, and
    val_cap at a page's bytes, one less, the first non-empty value, one less than it, and 0."""
    big = 1 << 30
    out = [(None, None, 1000, big)]
    keys = [k for k, _, _ in diffs]
    for kind in (1, 2, 3):
        mine = [i for i, d in enumerate(diffs) if d[1] == kind]
        for i in r.sample(mine, min(per_kind, len(mine))):
            k = keys[i]
            for p in (0, r.randrange(1, 63), 63):
                for d in (-1, 1):
                    b = _nudge(k, p, d)
                    if b is None:
                        continue
                    out += [(b, None, r.choice([1, 3, 1000]), big), (None, b, 1000, big),
                            (min(b, k), max(b, k), 1000, big)]
            out += [(k, k, 1, big), (RC._step(k, 1), None, 2, big), (None, RC._step(k, -1), 1000, big)]
        if mine:
            first = mine[0]
            out += [(None, None, mx, big) for mx in (first, first + 1) if mx >= 1]
    page = diffs[:8]
    total = sum(len(v) for _, _, v in page)
    lens = [len(v) for _, _, v in page if v]
    if lens:
        out += [(None, None, 8, cap) for cap in (total, total - 1, lens[0], lens[0] - 1, 0)]
    return out


def expected_from_content(diffs, origin, limit, max_entries, val_cap):
    """expected_diff of two FULL stores from their merged content: the same rules over a sorted list."""
    keys = [k for k, _, _ in diffs]
    lo = bisect.bisect_left(keys, ZERO if origin is None else origin)
    hi = bisect.bisect_right(keys, FF if limit is None else limit)
    things = diffs[lo:max(lo, min(hi, lo + max_entries + 1))]
    k = total = 0
    while k < min(len(things), max_entries) and total + len(things[k][2]) <= val_cap:
        total += len(things[k][2])
        k += 1
    if things and k == 0:
        return ("nospc", len(things[0][2]))
    more = k < len(things)
    return ("page", things[:k], more, things[k][0] if more else None)


# ---- the shapes of the host replay: (name, puts of a, puts of b), a put = (key, value, it leaves a
# value-only branch)
def _acct(r):
    return C.account_value(r)


def shapes(seed=17):
    r = random.Random(seed)
    out = []
    k = C._rk(r)
    out.append(("one_key_against_none", [(k, _acct(r), False)], []))
    out.append(("none_against_one_key", [], [(k, _acct(r), False)]))
    out.append(("same_key_two_values", [(k, _acct(r), False)], [(k, _acct(r), False)]))
    K = F.Keys(r)
    assert len(K.P) == 17
    base = K.key(r)
    for p in K.P:  # two leaves whose keys part at each of the 17 split depths
        n = F.nibbles(base)
        n[p] = (n[p] + 1 + r.randrange(15)) % 16
        out.append((f"two_leaves_split_{p}", [(base, _acct(r), False)], [(F.from_nibbles(n), _acct(r), False)]))
    # a leaf against a branch at depth 9: the leaf's key under the branch (one of its keys, and a
    # third child), and off its extension (parting at nibble 4)
    def at(key, p, v):
        n = F.nibbles(key)
        n[p] = v
        return F.from_nibbles(n)
    k0 = at(base, 9, 3)
    k1 = at(base, 9, 7)
    two = [(k0, _acct(r), False), (k1, _acct(r), False)]
    out.append(("leaf_under_branch_same_key", [two[0]], two))
    out.append(("leaf_under_branch_other_value", [(k0, _acct(r), False)], two))
    out.append(("leaf_under_branch_third_child", [(at(base, 9, 5), _acct(r), False)], two))
    out.append(("leaf_off_the_extension", [(at(base, 4, (F.nibbles(base)[4] + 1) % 16), _acct(r), False)], two))
    out.append(("branch_against_leaf", two, [(at(base, 9, 5), _acct(r), False)]))
    # an extension on one side that the other side branches inside: the same two keys under an
    # extension of 9 nibbles, and with a third key parting at nibble 4 (the branch at 9 is the same
    # node under a shorter extension: carried down, then skipped by its own reference)
    k3 = at(base, 4, (F.nibbles(base)[4] + 5) % 16)
    out.append(("branch_inside_extension", two, two + [(k3, _acct(r), False)]))
    out.append(("extension_inside_branch", two + [(k3, _acct(r), False)], two))
    out.append(("branch_inside_extension_changed", two, [two[0], (k1, _acct(r), False), (k3, _acct(r), False)]))
    # embedded nodes: one value changed, one key gone, one new
    ks, vs = export_cases.embedded_case()
    a = [(x, v, False) for x, v in zip(ks, vs)]
    b = [(x, (b"\x7f" if i == 5 else v), False) for i, (x, v) in enumerate(zip(ks, vs)) if i != 11]
    b.append((ks[20][:31] + bytes([ks[20][31] ^ 0x0F]), b"\x01", False))
    out.append(("embedded", a, b))
    # a value-only branch against a leaf of equal value
    k1, k2 = ks[0], ks[0][:31] + bytes([ks[0][31] ^ 0x01])
    v1, v2 = _acct(r), _acct(r)
    out.append(("vb_against_leaf", [(k1, v1, False), (k2, v2, False)], [(k1, v1, True), (k2, v2, False)]))
    out.append(("leaf_against_vb", [(k1, v1, True), (k2, v2, False)], [(k1, v1, False), (k2, v2, False)]))
    # dense keys: branches only at the 17 split depths
    dk, dv, _, _ = RC.dense_case()
    a = [(x, v, False) for x, v in zip(dk, dv)]
    b = [(x, (F.value(r) if i % 9 == 0 else v), False) for i, (x, v) in enumerate(zip(dk, dv)) if i % 7]
    b += [(K.key(r), F.value(r), False) for _ in range(10)]
    out.append(("dense", a, b))
    # 300 keys with 1, 7 and 150 of them changed
    ks = [C._rk(r) for _ in range(300)]
    vs = [_acct(r) if i % 3 else C.storage_value(r) for i in range(300)]
    a = [(x, v, False) for x, v in zip(ks, vs)]
    for nch in (1, 7, 150):
        ch = set(r.sample(range(300), nch))
        b = []
        for i, (x, v) in enumerate(zip(ks, vs)):
            if i not in ch:
                b.append((x, v, False))
            elif i % 3 == 0:
                b.append((C._rk(r), v, False))  # gone, and another key in its place
            else:
                b.append((x, _acct(r), False))
        out.append((f"random300_changed_{nch}", a, b))
    return out


def sixteen_children_one_differs(seed):
    """A branch pair of 16 children of which only the last differs: (puts of a, puts of b)."""
    r = random.Random(seed)
    base = F.nibbles(C._rk(r))
    a = []
    for c in range(16):
        n = list(base)
        n[0] = c
        a.append((F.from_nibbles(n), _acct(r), False))
    b = list(a)
    b[15] = (a[15][0], _acct(r), False)
    return a, b
