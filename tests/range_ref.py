"""The independent reference of the range-scan tests: an in-order walk over a node store
{hash: encoding} from a root, written from the RLP, HexPrefix and Merkle-Patricia-trie rules alone
(tests/proof_ref.list_items decodes; nothing of the library is imported).

walk(nodes, root, origin, limit) yields, in key order,
    ("entry", key, value)      an entry with origin <= key <= limit
    ("missing", hash, prefix)  a subtree whose node the store lacks and whose prefix (nibbles) meets
                               the range: one thing, at its lowest key
and never enters a subtree whose prefix lies outside the prefixes of [origin, limit].

expected_range(nodes, root, origin, limit, max_entries, val_cap) is what kh_trie_range_host documents:
    ("page", keys, vals, more, next) | ("nospc", size of the first value) | ("missing", hash)

Not a key -> value dict: khipu's value-only branch (a 17-item node at depth 64 holding only a
value) makes a trie's content depend on its history, and the walk reads it like any node.
"""
from tests import proof_ref as P

ZERO, FF = b"\x00" * 32, b"\xff" * 32


def _key(nib):
    return bytes((nib[2 * i] << 4) | nib[2 * i + 1] for i in range(32))


def _meets(prefix, on, ln):
    d = len(prefix)
    return on[:d] <= prefix <= ln[:d]


def walk(nodes, root, origin=None, limit=None):
    origin = ZERO if origin is None else origin
    limit = FF if limit is None else limit
    if root == P.EMPTY_ROOT or origin > limit:
        return
    on, ln = P.nibbles(origin), P.nibbles(limit)

    def by_hash(h, prefix):
        if not _meets(prefix, on, ln):
            return
        if h not in nodes:
            yield ("missing", h, list(prefix))
            return
        yield from node(nodes[h], 0, prefix)

    def child(d, item, prefix):
        is_list, start, s, e = item
        if is_list:  # a node embedded in its parent
            if _meets(prefix, on, ln):
                yield from node(d, start, prefix)
        elif e - s == 32:
            yield from by_hash(bytes(d[s:e]), prefix)
        else:
            assert e == s, "a child is empty, a hash or an embedded node"

    def node(d, pos, prefix):
        _, it = P.list_items(d, pos, len(d))
        if len(it) == 17:
            if len(prefix) == 64:  # a value-only branch
                _, _, s, e = it[16]
                k = _key(prefix)
                if e > s and origin <= k <= limit:
                    yield ("entry", k, bytes(d[s:e]))
                return
            for c in range(16):
                yield from child(d, it[c], prefix + [c])
            return
        assert len(it) == 2
        _, _, s, e = it[0]
        hp = P.nibbles(d[s:e])
        path = hp[1:] if hp[0] & 1 else hp[2:]
        if hp[0] & 2:
            k = _key(prefix + path)
            if origin <= k <= limit:
                yield ("entry", k, bytes(d[it[1][2]:it[1][3]]))
        else:
            yield from child(d, it[1], prefix + path)

    yield from by_hash(root, [])


def expected_range(nodes, root, origin=None, limit=None, max_entries=1024, val_cap=1 << 20):
    things = []
    for t in walk(nodes, root, origin, limit):
        things.append(t)
        if len(things) == max_entries + 1:
            break
    for t in things:
        if t[0] == "missing":
            return ("missing", t[1])
    ents = things[:max_entries]
    k = total = 0
    while k < len(ents) and total + len(ents[k][2]) <= val_cap:
        total += len(ents[k][2])
        k += 1
    if ents and k == 0:
        return ("nospc", len(ents[0][2]))
    more = k < len(things)
    return ("page", [t[1] for t in ents[:k]], [t[2] for t in ents[:k]], more, things[k][1] if more else None)


class Snapshot:
    """One walk of a full store, kept: expected_range answered from the walked list, for tests that
    ask many ranges of one state (tests/test_range_ref.py holds it equal to expected_range)."""

    def __init__(self, nodes, root):
        self.items = content(nodes, root)
        self.keys = [k for k, _ in self.items]

    def expected_range(self, origin=None, limit=None, max_entries=1024, val_cap=1 << 20):
        import bisect
        lo = bisect.bisect_left(self.keys, ZERO if origin is None else origin)
        hi = bisect.bisect_right(self.keys, FF if limit is None else limit)
        things = self.items[lo:max(lo, min(hi, lo + max_entries + 1))]
        k = total = 0
        while k < min(len(things), max_entries) and total + len(things[k][1]) <= val_cap:
            total += len(things[k][1])
            k += 1
        if things and k == 0:
            return ("nospc", len(things[0][1]))
        more = k < len(things)
        return ("page", [x for x, _ in things[:k]], [v for _, v in things[:k]], more, things[k][0] if more else None)


def content(nodes, root):
    """Every (key, value) of the trie in key order (a full store)."""
    out = []
    for t in walk(nodes, root):
        assert t[0] == "entry", t
        out.append((t[1], t[2]))
    return out
