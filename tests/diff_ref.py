"""The independent reference of the trie-diff tests, written from kh_trie_diff_host's contract over
node stores {hash: encoding} (tests/proof_ref.list_items decodes; nothing of the library is imported).

content_diff(nodes_a, root_a, nodes_b, root_b)
    merges the two tries' full (key, value, is a value-only branch) lists: [(key, kind, value of b)].
    Full stores only.

walk_diff(nodes_a, root_a, nodes_b, root_b, origin, limit, stats)
    descends both stores in lockstep by nibble path.  A side at a path is nothing, a node that STARTS
    there (known by its reference: a 32-byte hash, or the bytes of a node embedded in its parent), or
    a place inside the path of a leaf or an extension that started higher up.  Two nodes that start
    at the same path with the same reference are skipped unread; a hash the store lacks that is not
    skipped is a missing thing.  Yields, in key order,
        ("diff", key, kind, value of b)   kind 1: in a only (value b""), 2: in b only, 3: in both and
                                          the values or the value-only-branch status differ
        ("missing", hash)                 (side a's when both sides miss a node at one path)
    stats (a dict, optional) counts: "decoded" nodes, "skipped" pairs, "splits" (both sides present,
    no child nibble in common), "vb" (a kind-3 difference of equal values).

expected_diff(...) applies the max_entries + 1, missing, nospc and fit rules:
    ("page", [(key, kind, value)], more, next) | ("nospc", size) | ("missing", hash)
"""
from tests import proof_ref as P

ZERO, FF = b"\x00" * 32, b"\xff" * 32
ONLY_A, ONLY_B, CHANGED = 1, 2, 3


def _key(nib):
    return bytes((nib[2 * i] << 4) | nib[2 * i + 1] for i in range(32))


def _decode(d, depth):
    """An encoding that starts at `depth` -> ("branch", [ref or None] * 16) | ("vb", value) |
    ("leaf", path, value) | ("ext", path, ref); a ref is a hash or an embedded node's bytes."""
    _, it = P.list_items(d, 0, len(d))

    def ref(item):
        is_list, start, s, e = item
        if is_list:
            return bytes(d[start:e])
        assert e - s in (0, 32), "a child is empty, a hash or an embedded node"
        return bytes(d[s:e]) if e > s else None

    if len(it) == 17:
        if depth == 64:
            return ("vb", bytes(d[it[16][2]:it[16][3]]))
        return ("branch", [ref(x) for x in it[:16]])
    assert len(it) == 2
    hp = P.nibbles(d[it[0][2]:it[0][3]])
    path = hp[1:] if hp[0] & 1 else hp[2:]
    if hp[0] & 2:
        return ("leaf", path, bytes(d[it[1][2]:it[1][3]]))
    return ("ext", path, ref(it[1]))


class _Missing(Exception):
    def __init__(self, h):
        self.h = h


def _resolve(nodes, side, depth, stats):
    """A side -> its form at this depth.  side: None | ("start", ref) | a form already inside a path."""
    if side is None or side[0] != "start":
        return side
    r = side[1]
    if len(r) == 32:
        if r not in nodes:
            raise _Missing(r)
        r = nodes[r]
    if stats is not None:
        stats["decoded"] = stats.get("decoded", 0) + 1
    return _decode(r, depth)


def _children(form):
    """{nibble: the side one nibble down} of a form that is not an entry yet."""
    if form is None:
        return {}
    if form[0] == "branch":
        return {c: ("start", r) for c, r in enumerate(form[1]) if r is not None}
    kind, path, x = form
    c, rest = path[0], path[1:]
    if kind == "ext" and not rest:
        return {c: ("start", x)}
    return {c: (kind, rest, x)}


def _entry(form):
    """(value, is a value-only branch) of a form that is an entry at depth 64, else None."""
    if form is None:
        return None
    if form[0] == "vb":
        return form[1], True
    if form[0] == "leaf" and not form[1]:
        return form[1 + 1], False
    return None


def walk_diff(nodes_a, root_a, nodes_b, root_b, origin=None, limit=None, stats=None):
    origin = ZERO if origin is None else origin
    limit = FF if limit is None else limit
    if origin > limit:
        return
    on, ln = P.nibbles(origin), P.nibbles(limit)

    def bump(what):
        if stats is not None:
            stats[what] = stats.get(what, 0) + 1

    def step(prefix, sa, sb):
        d = len(prefix)
        if (sa is None and sb is None) or not on[:d] <= prefix <= ln[:d]:
            return
        if sa is not None and sb is not None and sa[0] == "start" and sb[0] == "start" and sa[1] == sb[1]:
            bump("skipped")
            return
        try:
            fa = _resolve(nodes_a, sa, d, stats)
        except _Missing as m:
            yield ("missing", m.h)
            return
        try:
            fb = _resolve(nodes_b, sb, d, stats)
        except _Missing as m:
            yield ("missing", m.h)
            return
        if d == 64:
            ea, eb = _entry(fa), _entry(fb)
            assert (ea is not None or fa is None) and (eb is not None or fb is None)
            k = _key(prefix)
            if eb is None:
                yield ("diff", k, ONLY_A, b"")
            elif ea is None:
                yield ("diff", k, ONLY_B, eb[0])
            elif ea != eb:
                if ea[0] == eb[0]:
                    bump("vb")
                yield ("diff", k, CHANGED, eb[0])
            return
        ca, cb = _children(fa), _children(fb)
        if ca and cb and not set(ca) & set(cb):
            bump("splits")
        for c in sorted(set(ca) | set(cb)):
            yield from step(prefix + [c], ca.get(c), cb.get(c))

    yield from step([], None if root_a == P.EMPTY_ROOT else ("start", root_a),
                    None if root_b == P.EMPTY_ROOT else ("start", root_b))


def content(nodes, root):
    """Every (key, value, is a value-only branch) of a full store, in key order."""
    out = []
    for t in walk_diff(nodes, root, {}, P.EMPTY_ROOT):
        assert t[0] == "diff" and t[2] == ONLY_A
        out.append(t[1])
    # the one-sided walk names the keys; their values and kinds come from a walk with the sides swapped
    vals = {t[1]: t[3] for t in walk_diff({}, P.EMPTY_ROOT, nodes, root)}
    vbs = _vb_keys(nodes, root)
    return [(k, vals[k], k in vbs) for k in out]


def _vb_keys(nodes, root):
    """The keys held by value-only branches: a plain descent of the store."""
    out = set()

    def node(ref, prefix):
        form = _decode(nodes[ref] if len(ref) == 32 else ref, len(prefix))
        if form[0] == "vb":
            out.add(_key(prefix))
        elif form[0] == "branch":
            for c, r in enumerate(form[1]):
                if r is not None:
                    node(r, prefix + [c])
        elif form[0] == "ext":
            node(form[2], prefix + form[1])

    if root != P.EMPTY_ROOT:
        node(root, [])
    return out


def content_diff(nodes_a, root_a, nodes_b, root_b):
    """The merge of the two full (key, value, value-only branch) lists: [(key, kind, value of b)]."""
    a = {k: (v, vb) for k, v, vb in content(nodes_a, root_a)}
    b = {k: (v, vb) for k, v, vb in content(nodes_b, root_b)}
    out = []
    for k in sorted(set(a) | set(b)):
        if k not in b:
            out.append((k, ONLY_A, b""))
        elif k not in a:
            out.append((k, ONLY_B, b[k][0]))
        elif a[k] != b[k]:
            out.append((k, CHANGED, b[k][0]))
    return out


def expected_diff(nodes_a, root_a, nodes_b, root_b, origin=None, limit=None, max_entries=1024, val_cap=1 << 20):
    things = []
    for t in walk_diff(nodes_a, root_a, nodes_b, root_b, origin, limit):
        things.append(t)
        if len(things) == max_entries + 1:
            break
    for t in things:
        if t[0] == "missing":
            return ("missing", t[1])
    ents = things[:max_entries]
    k = total = 0
    while k < len(ents) and total + len(ents[k][3]) <= val_cap:
        total += len(ents[k][3])
        k += 1
    if ents and k == 0:
        return ("nospc", len(ents[0][3]))
    more = k < len(things)
    return ("page", [(t[1], t[2], t[3]) for t in ents[:k]], more, things[k][1] if more else None)
