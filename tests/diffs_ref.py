"""The independent reference of the batched trie diff (kh_trie_diffs_host), built on
tests/diff_ref.walk_diff: the walks of the requests chained in request order, the first
max_entries + 1 things of the chain, then the missing / nospc / fit rules.  Nothing of the library
is imported.

expected_diffs(side_a, side_b, requests, max_entries, val_cap)
    side_a, side_b  {trie id: (nodes {hash: encoding}, root)}; an id a side lacks is an empty trie.
                    same=True: both sides are ONE handle, so a request naming one id twice is empty
    requests        [(trie id of a, trie id of b or None (the same id), origin or None, limit or None)]
 -> ("pages", pages, n_done, next)   pages[q] = [(key, kind, value of b)]; n_done leading requests
                                     are answered completely; next: the first differing key of
                                     request n_done not returned (None when n_done == len(requests))
    ("nospc", size of the first value of the whole answer)
    ("missing", hash, request index)
"""
from tests import diff_ref as DR
from tests import proof_ref as P

EMPTY = ({}, P.EMPTY_ROOT)


def things_of(side_a, side_b, requests, most, same=False):
    """The first `most` things of the chained walks: [(request index, thing of diff_ref.walk_diff)]."""
    out = []
    for q, (ta, tb, origin, limit) in enumerate(requests):
        tb = ta if tb is None else tb
        if same and ta == tb:
            continue
        na, ra = side_a.get(ta, EMPTY)
        nb, rb = side_b.get(tb, EMPTY)
        for th in DR.walk_diff(na, ra, nb, rb, origin, limit):
            out.append((q, th))
            if len(out) == most:
                return out
    return out


def expected_diffs(side_a, side_b, requests, max_entries=1024, val_cap=1 << 20, same=False):
    nq = len(requests)
    things = things_of(side_a, side_b, requests, max_entries + 1, same)
    for q, th in things:
        if th[0] == "missing":
            return ("missing", th[1], q)
    ents = things[:max_entries]
    k = total = 0
    while k < len(ents) and total + len(ents[k][1][3]) <= val_cap:
        total += len(ents[k][1][3])
        k += 1
    if ents and k == 0:
        return ("nospc", len(ents[0][1][3]))
    pages = [[] for _ in range(nq)]
    for q, th in ents[:k]:
        pages[q].append((th[1], th[2], th[3]))
    if k < len(things):
        return ("pages", pages, things[k][0], things[k][1][1])
    return ("pages", pages, nq, None)
