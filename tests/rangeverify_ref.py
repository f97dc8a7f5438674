"""The independent reference of the range-verification tests, written from the contract of
kh_verify_ranges (include/khst.h) and the RLP, HexPrefix and Merkle-Patricia-trie rules alone:
nothing of the library is imported (tests/proof_ref.list_items decodes).

boundary_walk(nodes, root, origin, hi) -> (status, more, missing, kept): the walk along origin's
path and hi's path over {hash: encoding}; kept is a list of (prefix nibbles, reference bytes, side),
side 0 for a subtree kept on the left, 1 on the right; the reference is a 32-byte hash or an
embedded list shorter than 32 bytes.

verify(nodes, root, origin, keys, vals, proved) -> (status, more, missing): the whole contract.  The
rebuild is a recursive canonical builder over the entries and the kept subtrees (group by nibble,
the longest common prefix becomes an extension, a 17-item branch; a kept subtree that would have
to move: BAD_ROOT) -- not the device's sort-and-topology build.
"""
from tests import proof_ref as P

OK, BAD_ORDER, MISSING, BAD_NODE, BAD_ROOT, INCOMPLETE = range(6)
ZERO = b"\x00" * 32


class _Problem(Exception):
    def __init__(self, status, missing=None):
        self.status, self.missing = status, missing


def _child_ref(d, item):
    """A child item of a node: None (empty), or its reference -- the 32-byte hash, or the embedded
    list's bytes (shorter than 32)."""
    is_list, start, s, e = item
    if not is_list:
        if e == s:
            return None
        if e - s != 32:
            raise _Problem(BAD_NODE)
        return bytes(d[s:e])
    if e - start >= 32:
        raise _Problem(BAD_NODE)
    return bytes(d[start:e])


def _walk_path(nodes, root, on, hn, side, kept):
    """One boundary path (side 0: origin's, 1: hi's).  Where both paths coincide the origin's walk
    alone keeps, so nothing is kept twice.  Returns `more`; raises _Problem at the first problem."""
    path = hn if side else on
    more = False
    ref, d = root, 0
    while True:
        if len(ref) == 32:
            if ref not in nodes:
                raise _Problem(MISSING, ref)
            enc = nodes[ref]
        else:
            enc = ref
        try:
            end, it = P.list_items(enc, 0, len(enc))
        except P.Bad:
            raise _Problem(BAD_NODE)
        if end != len(enc):
            raise _Problem(BAD_NODE)
        prefix = path[:d]
        emits = side == 0 or prefix != on[:d]
        if len(it) == 17:
            if d == 64:  # a value-only branch: a leaf with the key `prefix`, which lies within
                if it[16][0]:
                    raise _Problem(BAD_NODE)
                return more
            nxt = None
            for c in range(16):
                r = _child_ref(enc, it[c])
                if r is None:
                    continue
                p = prefix + [c]
                if c == path[d]:
                    nxt = r
                elif not emits:
                    continue
                elif p < on[:d + 1]:
                    kept.append((p, r, 0))
                elif p > hn[:d + 1]:
                    kept.append((p, r, 1))
                    more = True
            if nxt is None:
                return more
            ref, d = nxt, d + 1
            continue
        if len(it) != 2:
            raise _Problem(BAD_NODE)
        is_list, _, s, e = it[0]
        if is_list or e == s:
            raise _Problem(BAD_NODE)
        hp = P.nibbles(enc[s:e])
        flag = hp[0]
        if flag > 3 or (not flag & 1 and hp[1]):
            raise _Problem(BAD_NODE)
        q = prefix + (hp[1:] if flag & 1 else hp[2:])
        if len(q) > 64:
            raise _Problem(BAD_NODE)
        if flag & 2:
            if it[1][0] or len(q) != 64:
                raise _Problem(BAD_NODE)
            child = None
        else:
            child = _child_ref(enc, it[1])
            if child is None:
                raise _Problem(BAD_NODE)
            if q == path[:len(q)]:
                ref, d = child, len(q)
                continue
        if emits:
            if q < on[:len(q)]:
                kept.append((prefix, ref, 0))
            elif q > hn[:len(q)]:
                kept.append((prefix, ref, 1))
                more = True
        return more


def boundary_walk(nodes, root, origin, hi):
    on, hn = P.nibbles(origin), P.nibbles(hi)
    kept, probs, more = [], [], False
    if root != P.EMPTY_ROOT:
        for side in (0, 1):
            try:
                more = _walk_path(nodes, root, on, hn, side, kept) or more
            except _Problem as p:
                probs.append(p)
    if any(p.status == BAD_NODE for p in probs):
        return BAD_NODE, more, None, kept
    if probs:
        return MISSING, more, probs[0].missing, kept
    return OK, more, None, kept


# ---- the canonical builder
def _rlp_len(n, base):
    if n < 56:
        return bytes([base + n])
    b = n.to_bytes((n.bit_length() + 7) // 8, "big")
    return bytes([base + 55 + len(b)]) + b


def _rlp_str(b):
    return bytes(b) if len(b) == 1 and b[0] < 0x80 else _rlp_len(len(b), 0x80) + bytes(b)


def _rlp_list(items):
    body = b"".join(items)
    return _rlp_len(len(body), 0xC0) + body


def _hp(nib, leaf):
    flag = 2 if leaf else 0
    nib = [flag + 1] + nib if len(nib) & 1 else [flag, 0] + nib
    return bytes((nib[i] << 4) | nib[i + 1] for i in range(0, len(nib), 2))


class _Moved(Exception):
    pass


def _capped(enc):
    """What a parent holds of a node: its encoding when shorter than 32 bytes, else its hash."""
    return enc if len(enc) < 32 else _rlp_str(P.kec(enc))


def _slot(items, depth):
    """The parent's item for the subtree of `items`, which share their first `depth` nibbles: each
    (nibbles, value) for an entry or (prefix, None, reference) for a kept subtree."""
    if len(items) == 1 and len(items[0]) == 3:
        prefix, _, ref = items[0]
        if len(prefix) != depth:  # it would need an extension above it: its place would move
            raise _Moved
        return ref if len(ref) < 32 else _rlp_str(ref)
    return _capped(_node(items, depth))


def _node(items, depth):
    if len(items) == 1:
        nib, val = items[0]
        return _rlp_list([_rlp_str(_hp(nib[depth:], True)), _rlp_str(val)])
    cp = depth
    while all(len(it[0]) > cp for it in items) and len({it[0][cp] for it in items}) == 1:
        cp += 1
    if any(len(it[0]) <= cp for it in items):  # something runs under a kept subtree's prefix
        raise _Moved
    groups = [[] for _ in range(16)]
    for it in items:
        groups[it[0][cp]].append(it)
    branch = _rlp_list([_slot(g, cp + 1) if g else b"\x80" for g in groups] + [b"\x80"])
    if cp == depth:
        return branch
    return _rlp_list([_rlp_str(_hp(items[0][0][depth:cp], False)), _capped(branch)])


def rebuilt_root(keys, vals, kept):
    """The root of the canonical trie over the entries and the kept subtrees; None when a kept
    subtree's place would have to move."""
    items = [(P.nibbles(k), v) for k, v in zip(keys, vals)] + [(list(p), None, r) for p, r, _ in kept]
    if not items:
        return P.EMPTY_ROOT
    try:
        if len(items) == 1 and len(items[0]) == 3:  # the root node itself was kept
            if items[0][0]:
                raise _Moved
            return items[0][2]
        return P.kec(_node(items, 0))
    except _Moved:
        return None


def verify(nodes, root, origin, keys, vals, proved=1):
    """(status, more, missing) of one range by the contract of kh_verify_ranges."""
    origin = ZERO if origin is None else origin
    keys, vals = list(keys), list(vals)
    if any(len(v) == 0 for v in vals) or (keys and keys[0] < origin) or \
            any(a >= b for a, b in zip(keys, keys[1:])):
        return BAD_ORDER, False, None
    if not proved:
        return (OK if rebuilt_root(keys, vals, []) == root else BAD_ROOT), False, None
    st, more, missing, kept = boundary_walk(nodes, root, origin, keys[-1] if keys else origin)
    if st != OK:
        return st, False, missing
    if not keys and more:
        return INCOMPLETE, True, None
    return (OK if rebuilt_root(keys, vals, kept) == root else BAD_ROOT), more, None
