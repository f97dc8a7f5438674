"""Request batches for the batched range-scan tests (tests/test_ranges_ref.py pins their conditions
with the oracle alone; tests/test_gpu_ranges.py runs them).  No GPU, no library.

A STATE is a set of tries {id: oracle trie} (an id whose trie is empty is in it too); batches()
draws request batches over a state's content: nq in NQS, repeated tries, an unheld id, empty tries
at the front, in the middle and at the end, origin > limit, whole-trie requests mixed with bounded
ones, and budgets aimed so that the answer ends complete, cut inside a request, cut exactly at a
request's first entry, cut by val_cap, and cut directly after an empty request."""
import bisect
import random

from tests import cases as C
from tests import proof_ref as P
from tests import range_cases as RC

NQS = [1, 2, 3, 17, 64]
BIG = 1 << 26
UNHELD = 0x7FFFFFF1  # an id no state holds
EMPTY_IDS = [0x7FFFFFF2, 0x7FFFFFF3]  # ids every state holds as empty tries
# state -> (seed, batches): what the device test runs and the CPU pin holds its conditions for
RUNS = {"scenarios": (101, 60), "forest60": (102, 60), "big": (103, 40)}


def scenario_tries(oracle):
    """Every state of tests/cases.commit_scenarios() -- the opened trie and the trie after each
    batch -- as one trie of a forest: {id: (nodes, root)}."""
    out = {}
    for name, ks, vs, batches in C.commit_scenarios():
        o = oracle.Trie()
        for k, v in zip(ks, vs):
            o.put(k, v)
        for b in range(len(batches) + 1):
            if b:
                for k, v in batches[b - 1][0]:
                    o.put(k, v)
                for k in batches[b - 1][1]:
                    o.remove(k)
            out[len(out) + 1] = _store(oracle, o)
    return out


def _store(oracle, o):
    root = o.root_hash()
    return (o.reachable() if root != P.EMPTY_ROOT else {}, root)


def forest60_tries(oracle):
    """60 small tries of hashed 32-byte slots, ids up to 2^32, and two twin tries of the same
    content (the forest of tests/test_gpu_range.py, built from its data alone)."""
    r = random.Random(78)
    ids = [r.randrange(1 << 16, 1 << 32) for _ in range(56)] + [0, 7, 65535, 65536]
    twins = [r.randrange(1 << 32) for _ in range(2)]
    tries = {t: oracle.Trie() for t in ids + twins}
    for t in ids:
        for _ in range(r.choice([1, 3, 10, 40])):
            tries[t].put(oracle.kec256(RC._rk(r)), C.storage_value(r))
    for tw in twins:
        for j in range(6):
            tries[tw].put(oracle.kec256(bytes([j]) * 32), b"\x01" * 40)
    return {t: _store(oracle, o) for t, o in tries.items()}


def big_tries(oracle):
    """One trie of 2,000 entries (a frontier of several blocks) and three small ones."""
    r = random.Random(79)
    out = {}
    for t, n in ((5, 2000), (6, 10), (1 << 20, 1), (9, 33)):
        o = oracle.Trie()
        for i in range(n):
            o.put(RC._rk(r), C.account_value(r) if i % 3 else C.storage_value(r))
        out[t] = _store(oracle, o)
    return out


STATES = {"scenarios": scenario_tries, "forest60": forest60_tries, "big": big_tries}


def state(oracle, name):
    """{id: (nodes, root)} of state `name`, the always-empty ids included."""
    out = STATES[name](oracle)
    for e in EMPTY_IDS:
        out[e] = ({}, P.EMPTY_ROOT)
    return out


def _span(keys, o, l):
    """The indices [lo, hi) of sorted keys within [o, l]."""
    o, l = RC.ZERO if o is None else o, RC.FF if l is None else l
    if o > l:
        return 0, 0
    lo = bisect.bisect_left(keys, o)
    return lo, max(lo, bisect.bisect_right(keys, l))


def _request(r, content, held, prev):
    x = r.random()
    if x < 0.08:
        return (UNHELD, None, None)
    if x < 0.16:
        return (r.choice(EMPTY_IDS), None, _pick(r, []) if r.random() < 0.3 else None)
    t = prev if (prev in content and content[prev] and x < 0.3) else r.choice(held)
    keys = [k for k, _ in content[t]]
    y = r.random()
    if y < 0.4:
        return (t, None, None)
    if y < 0.55:
        return (t, _pick(r, keys), None)
    if y < 0.68:
        return (t, None, _pick(r, keys))
    a, b = sorted([_pick(r, keys), _pick(r, keys)])
    if y < 0.93 or a == b:
        return (t, a, b)
    return (t, b, a)  # origin > limit


def _pick(r, keys):
    return RC._point(r, keys)


def batches(r, content, n):
    """n batches (requests, max_entries, val_cap) over content {id: [(key, value)] in key order}."""
    held = [t for t in content if content[t]]
    out = []
    for i in range(n):
        nq = NQS[i % len(NQS)] if i < 2 * len(NQS) else r.choice(NQS)
        reqs, prev = [], None
        for _ in range(nq):
            reqs.append(_request(r, content, held, prev))
            prev = reqs[-1][0]
        where = i % 7  # empty tries at the front, in the middle, at the end
        if where == 1:
            reqs[0] = (EMPTY_IDS[0], None, None)
        elif where == 2:
            reqs[nq // 2] = (EMPTY_IDS[1], None, None)
        elif where == 3:
            reqs[-1] = (EMPTY_IDS[0], None, None)
        # the whole answer, from the content alone: (request, value length) per entry
        ents, start, cnt = [], [], []
        for q, (t, o, l) in enumerate(reqs):
            lo, hi = _span([k for k, _ in content.get(t, [])], o, l)
            start.append(len(ents))
            cnt.append(hi - lo)
            ents += [(q, len(v)) for _, v in content[t][lo:hi]] if hi > lo else []
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
        elif aim == 2:  # cut exactly at a request's first entry
            qs = [q for q in range(nq) if cnt[q] and start[q]]
            if qs:
                mx = start[r.choice(qs)]
        elif aim == 3:  # cut by val_cap
            if total >= 2:
                m = r.randrange(1, total)
                mx = total + 3
                cap = sum(ln for _, ln in ents[:m]) + r.randrange(0, max(ents[m][1], 1))
        elif aim == 4:  # an empty request directly before the cut one
            qs = [q for q in range(1, nq) if cnt[q] and start[q] and not cnt[q - 1]]
            if qs:
                q = r.choice(qs)
                mx = start[q] + r.randrange(0, cnt[q])
        out.append((reqs, mx, cap))
    return out


def batches_for(name, content):
    seed, n = RUNS[name]
    return batches(random.Random(seed), content, n)
