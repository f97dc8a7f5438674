"""The independent model of kh_trie_changes_since_host, written from its contract over two Python
dicts (nothing of the library is imported): the content at the savepoint and the content now,

    {(trie id, key): (value bytes, is a value-only branch)}      (a single trie: trie id 0)

differences(before, after, reverse)
    every difference in (trie id, key) order: [(trie, key, kind, value)] with kind 1 (in `before`
    only, value b""), 2 (in `after` only) or 3 (in both; the values or the value-only-branch status
    differ) and `after`'s value; reverse swaps the two dicts.

expected(before, after, reverse, start, max_entries, val_cap)
    one call: the differences at or after start = (trie, key) (None: all), their count n_total, at
    most max_entries of them cut to the longest prefix whose values fit val_cap:
        ("page", [(trie, key, kind, value)], more, next (trie, key) or None, n_total)
        ("nospc", size of the first value, n_total)

ops(entries)
    the (upserts [(trie, key, value)], deletes [(trie, key)]) that the entries stand for.
"""
ONLY_A, ONLY_B, CHANGED = 1, 2, 3


def differences(before, after, reverse=False):
    a, b = (after, before) if reverse else (before, after)
    out = []
    for tk in sorted(set(a) | set(b)):
        if tk not in b:
            out.append((tk[0], tk[1], ONLY_A, b""))
        elif tk not in a:
            out.append((tk[0], tk[1], ONLY_B, b[tk][0]))
        elif a[tk] != b[tk]:
            out.append((tk[0], tk[1], CHANGED, b[tk][0]))
    return out


def expected(before, after, reverse=False, start=None, max_entries=1024, val_cap=1 << 20):
    diffs = [d for d in differences(before, after, reverse) if start is None or (d[0], d[1]) >= tuple(start)]
    n_total = len(diffs)
    ents = diffs[:max_entries]
    k = total = 0
    while k < len(ents) and total + len(ents[k][3]) <= val_cap:
        total += len(ents[k][3])
        k += 1
    if ents and k == 0:
        return ("nospc", len(ents[0][3]), n_total)
    more = k < n_total
    return ("page", ents[:k], more, (diffs[k][0], diffs[k][1]) if more else None, n_total)


def ops(entries):
    ups = [(t, k, v) for t, k, kind, v in entries if kind != ONLY_A]
    dels = [(t, k) for t, k, kind, _ in entries if kind == ONLY_A]
    return ups, dels


def single(d):
    """{key: value or (value, vb)} of one trie as a model dict under trie id 0."""
    return {(0, k): (v if isinstance(v, tuple) else (v, False)) for k, v in d.items()}
