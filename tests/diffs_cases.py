"""Request batches for the batched trie-diff tests (tests/test_diffs_ref.py pins their conditions with
the oracle alone; tests/test_gpu_diffs.py runs them).  No GPU, no library.

A STATE PAIR is two forests {id: (nodes, root)}, side a and side b (for "ids" they are ONE forest):
    ids        every state of every scenario of tests/diff_cases.scenarios() under an id of its own;
               the requests name the ordered state pairs (i, j), |i - j| <= 3, that
               tests/test_diff_ref.py uses
    v01 v12 v20   version v of the forest holds scenario s, under id s + 1, after its first v batches
               (its last state when it has fewer): two versions of one forest, the same id on both sides
    forest60   60 small tries of hashed slots with ids past 2^16 and two twin tries, against the same
               forest after a block that changes a few slots of half of them, drops one trie and
               makes a new one
batches() draws request batches over a state pair: nq in NQS, repeated pairs, an identical pair at
the front, in the middle and at the end, an id held by one side only and by neither, origin > limit,
whole-trie requests mixed with bounded ones, and budgets aimed so that the answer ends complete, cut
inside a request, cut exactly at a request's first difference, cut by val_cap, and cut directly after
an empty request."""
import bisect
import random

from tests import cases as C
from tests import diff_cases as DC
from tests import diff_ref as DR
from tests import proof_ref as P
from tests import range_cases as RC

NQS = [1, 2, 3, 17, 64]
BIG = 1 << 26
UNHELD = [0x7FFFFFF1, 0x7FFFFFF4]  # ids no side of any state pair holds
SCEN = DC.scenarios()
# state pair -> (seed, batches): what the device test runs and the CPU pin holds its conditions for
RUNS = {"ids": (201, 40), "v01": (202, 24), "v12": (203, 24), "v20": (204, 24), "forest60": (205, 40)}
VERSIONS = {"v01": (0, 1), "v12": (1, 2), "v20": (2, 0)}
ONLY_A_ID, ONLY_B_ID, TWIN_ID = 9001, 9002, 1 << 20  # what the version pairs hold beside the scenarios


def sid(s, j):
    """The id of state j of scenario s in the "ids" forest."""
    return 100 * s + j + 1


def scenario_states(oracle):
    """[[(nodes, root)] per state] per scenario."""
    return [DC.states(oracle, s) for s in SCEN]


def ids_forest(states):
    return {sid(s, j): st for s, sts in enumerate(states) for j, st in enumerate(sts)}


def version(states, v):
    """{s + 1: scenario s after its first v batches (its last state when it has fewer)}"""
    return {s + 1: sts[min(v, len(sts) - 1)] for s, sts in enumerate(states)}


def forest60_ops(oracle):
    """(puts of side a [(id, raw key, value)], the block (upserts [(id, raw key, value)], deletes [(id,
    raw key)]) that makes side b, the twin ids).  The trie keys are the kec256 values of the raw keys."""
    r = random.Random(78)
    ids = [r.randrange(1 << 16, 1 << 32) for _ in range(56)] + [0, 7, 65535, 65536]
    twins = [r.randrange(1 << 32) for _ in range(2)]
    puts = []
    for t in ids:
        for _ in range(r.choice([1, 3, 10, 40])):
            puts.append((t, RC._rk(r), C.storage_value(r)))
    for tw in twins:
        puts += [(tw, bytes([j]) * 32, b"\x01" * 40) for j in range(6)]
    ups, dels = [], []
    for t in ids[::2]:
        mine = [k for u, k, _ in puts if u == t]
        for k in r.sample(mine, min(len(mine), r.choice([1, 2, 3]))):
            if r.random() < 0.3 and len(mine) > 3:
                dels.append((t, k))
            else:
                ups.append((t, k, C.storage_value(r)))
        if r.random() < 0.5:
            ups.append((t, RC._rk(r), C.storage_value(r)))
    gone = ids[1]  # held by side a only afterwards
    dels += [(gone, k) for u, k, _ in puts if u == gone]
    new = 0x80000005  # held by side b only
    ups += [(new, RC._rk(r), C.storage_value(r)) for _ in range(5)]
    return puts, (ups, dels), twins


def forest60_pair(oracle):
    puts, (ups, dels), _ = forest60_ops(oracle)
    tries = {}
    for t, k, v in puts:
        tries.setdefault(t, oracle.Trie()).put(oracle.kec256(k), v)
    a = {t: DC.snap(o) for t, o in tries.items()}
    for t, k, v in ups:
        tries.setdefault(t, oracle.Trie()).put(oracle.kec256(k), v)
    for t, k in dels:
        tries[t].remove(oracle.kec256(k))
    b = {t: DC.snap(o) for t, o in tries.items() if o.root_hash() != P.EMPTY_ROOT}
    return a, b


def state_pair(oracle, name, states=None):
    """(side a, side b, both are one handle, the candidate pairs [(id of a, id of b)])"""
    if name == "forest60":
        a, b = forest60_pair(oracle)
        return a, b, False, [(t, t) for t in sorted(set(a) | set(b))]
    states = states or scenario_states(oracle)
    if name == "ids":
        f = ids_forest(states)
        pairs = [(sid(s, i), sid(s, j)) for s, sts in enumerate(states) for i, j in DC.pairs(len(sts))]
        pairs += [(sid(0, 0), UNHELD[0]), (UNHELD[0], sid(0, 1))]  # an id one side of the request lacks
        return f, f, True, pairs
    va, vb = VERSIONS[name]
    a, b = version(states, va), version(states, vb)
    n = len(a)
    a[ONLY_A_ID] = states[1][0]  # held by side a only
    b[ONLY_B_ID] = states[1][1]  # held by side b only
    a[TWIN_ID] = b[TWIN_ID] = states[0][0]  # the same trie on both sides
    # the same id on both sides, and a few crossed pairs (two different scenarios: all of both differ)
    pairs = [(t, t) for t in sorted(set(a) | set(b))] + [(1, 2), (2, 1), (3, n)]
    return a, b, False, pairs


def full_diffs(a, b, same, pairs):
    """{(id of a, id of b): [(key, kind, value of b)]}, the whole difference list of each pair."""
    out = {}
    for ta, tb in pairs:
        if same and ta == tb:
            out[(ta, tb)] = []
            continue
        na, ra = a.get(ta, ({}, P.EMPTY_ROOT))
        nb, rb = b.get(tb, ({}, P.EMPTY_ROOT))
        out[(ta, tb)] = [(t[1], t[2], t[3]) for t in DR.walk_diff(na, ra, nb, rb)]
    return out


def _span(keys, o, l):
    """The indices [lo, hi) of sorted keys within [o, l]."""
    o, l = RC.ZERO if o is None else o, RC.FF if l is None else l
    if o > l:
        return 0, 0
    lo = bisect.bisect_left(keys, o)
    return lo, max(lo, bisect.bisect_right(keys, l))


def _request(r, diffs, differing, identical, prev, same):
    x = r.random()
    if x < 0.06:
        return (UNHELD[0], UNHELD[1] if r.random() < 0.5 else None, None, None)  # held by neither side
    if x < 0.14 and identical:
        ta, tb = r.choice(identical)
        return (ta, tb, None, RC._point(r, []) if r.random() < 0.3 else None)
    ta, tb = prev if (prev in diffs and diffs[prev] and x < 0.3) else r.choice(differing)
    keys = [k for k, _, _ in diffs[(ta, tb)]]
    tb_arg = None if (ta == tb and not same and r.random() < 0.5) else tb
    y = r.random()
    if y < 0.4:
        return (ta, tb_arg, None, None)
    if y < 0.55:
        return (ta, tb_arg, RC._point(r, keys), None)
    if y < 0.68:
        return (ta, tb_arg, None, RC._point(r, keys))
    o, l = sorted([RC._point(r, keys), RC._point(r, keys)])
    if y < 0.93 or o == l:
        return (ta, tb_arg, o, l)
    return (ta, tb_arg, l, o)  # origin > limit


def batches(r, diffs, same, n):
    """n batches (requests, max_entries, val_cap) over diffs {(id of a, id of b): difference list}."""
    differing = [p for p in diffs if diffs[p]]
    identical = [p for p in diffs if not diffs[p]]
    assert differing and identical
    out = []
    for i in range(n):
        nq = NQS[i % len(NQS)] if i < 2 * len(NQS) else r.choice(NQS)
        reqs, prev = [], None
        for _ in range(nq):
            reqs.append(_request(r, diffs, differing, identical, prev, same))
            prev = (reqs[-1][0], reqs[-1][0] if reqs[-1][1] is None else reqs[-1][1])
        where = i % 7  # an identical pair at the front, in the middle, at the end
        if where == 1:
            reqs[0] = identical[0] + (None, None)
        elif where == 2:
            reqs[nq // 2] = identical[-1] + (None, None)
        elif where == 3:
            reqs[-1] = identical[0] + (None, None)
        # the whole answer, from the difference lists alone: (request, value length) per difference
        ents, start, cnt = [], [], []
        for q, (ta, tb, o, l) in enumerate(reqs):
            d = diffs.get((ta, ta if tb is None else tb), [])
            lo, hi = _span([k for k, _, _ in d], o, l)
            start.append(len(ents))
            cnt.append(hi - lo)
            ents += [(q, len(v)) for _, _, v in d[lo:hi]]
        total = len(ents)
        mx, cap = r.choice(RC.MAXES), BIG
        aim = i % 6
        if aim == 0:  # complete
            mx = max(1, total + r.choice([0, 0, 1, 5]))
        elif aim == 1:  # cut inside a request
            qs = [q for q in range(nq) if cnt[q] >= 2]
            if qs:
                q = r.choice(qs)
                mx = start[q] + r.randrange(1, cnt[q])
        elif aim == 2:  # cut exactly at a request's first difference
            qs = [q for q in range(nq) if cnt[q] and start[q]]
            if qs:
                mx = start[r.choice(qs)]
        elif aim == 3:  # cut by val_cap (at a difference that carries a value)
            ms = [m for m in range(1, total) if ents[m][1]]
            if ms:
                m = r.choice(ms)
                mx = total + 3
                cap = sum(ln for _, ln in ents[:m]) + r.randrange(0, ents[m][1])
        elif aim == 4:  # an empty request directly before the cut one
            qs = [q for q in range(1, nq) if cnt[q] and start[q] and not cnt[q - 1]]
            if qs:
                q = r.choice(qs)
                mx = start[q] + r.randrange(0, cnt[q])
        out.append((reqs, mx, cap))
    return out


def batches_for(name, diffs, same):
    seed, n = RUNS[name]
    return batches(random.Random(seed), diffs, same, n)
