"""The independent reference of the batched range scan (kh_trie_ranges_host), built on
tests/range_ref.walk: the walks of the requests chained in request order, the first
max_entries + 1 things of the chain, then the missing / nospc / fit rules.  Nothing of the library
is imported.

expected_ranges(tries, requests, max_entries, val_cap)
    tries     {trie id: (nodes {hash: encoding}, root)}; an id it lacks is an empty trie
    requests  [(trie id, origin or None, limit or None)]
 -> ("pages", pages, n_done, next)   pages[q] = (keys, vals); n_done leading requests are answered
                                     completely; next: the first key of request n_done not returned
                                     (None when n_done == len(requests))
    ("nospc", size of the first value of the whole answer)
    ("missing", hash, request index)
"""
from tests import range_ref as RR


def things_of(tries, requests, most):
    """The first `most` things of the chained walks: [(request index, thing of range_ref.walk)]."""
    out = []
    for q, (t, origin, limit) in enumerate(requests):
        if t not in tries:
            continue
        nodes, root = tries[t]
        for th in RR.walk(nodes, root, origin, limit):
            out.append((q, th))
            if len(out) == most:
                return out
    return out


def expected_ranges(tries, requests, max_entries=1024, val_cap=1 << 20):
    nq = len(requests)
    things = things_of(tries, requests, max_entries + 1)
    for q, th in things:
        if th[0] == "missing":
            return ("missing", th[1], q)
    ents = things[:max_entries]
    k = total = 0
    while k < len(ents) and total + len(ents[k][1][2]) <= val_cap:
        total += len(ents[k][1][2])
        k += 1
    if ents and k == 0:
        return ("nospc", len(ents[0][1][2]))
    pages = [([], []) for _ in range(nq)]
    for q, th in ents[:k]:
        pages[q][0].append(th[1])
        pages[q][1].append(th[2])
    if k < len(things):
        return ("pages", pages, things[k][0], things[k][1][1])
    return ("pages", pages, nq, None)
