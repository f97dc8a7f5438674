"""The independent model of the range-fill tests, written from the contract of
kh_trie_fill_ranges_host (include/khst.h) and the trie rules alone: nothing of the library is
imported (tests/proof_ref decodes, tests/rangeverify_ref builds).

A partial handle is modelled as the set `held` of node hashes it holds, over the oracle's full node
set `nodes` ({hash: encoding} of every stored node, oracle.Trie.reachable()).  A stub is a hash
child of a held node that is not held; it is named by the nibble prefix at which the missing node
starts.  The inside test works on nibble prefixes.  A stub an entry reaches is rebuilt from the
entries under its prefix with the recursive canonical builder of tests/rangeverify_ref; the
rebuild is accepted when it hashes to the stub's hash, and the handle then holds the oracle's nodes
under that hash.

fill_nodes(nodes, root, held, encs) -> held afterwards (kh_trie_fill_nodes: stubs resolved from the
given encodings, round after round).
fill_range(nodes, root, held, origin, keys, vals) -> Result(status, held, n_keys, n_stubs, missing).
whole(root, keys, vals) -> status of a trie given whole (not resident before).
"""
import collections

from tests import partial_cases as PC
from tests import proof_ref as P
from tests import rangeverify_ref as RV

OK, BAD_ORDER, MISSING, BAD_NODE, BAD_ROOT, INCOMPLETE = range(6)
ZERO, FF = b"\x00" * 32, b"\xff" * 32

Result = collections.namedtuple("Result", "status held n_keys n_stubs missing")


def _decode(enc):
    """("branch", [ref or None] * 16) | ("ext", path, ref) | ("leaf", path, value); a ref is a
    32-byte hash or the bytes of an embedded node."""
    end, it = P.list_items(enc, 0, len(enc))
    assert end == len(enc)
    if len(it) == 17:
        return "branch", [RV._child_ref(enc, it[c]) for c in range(16)]
    _, _, s, e = it[0]
    hp = P.nibbles(enc[s:e])
    path = hp[1:] if hp[0] & 1 else hp[2:]
    if hp[0] & 2:
        _, _, vs, ve = it[1]
        return "leaf", path, bytes(enc[vs:ve])
    return "ext", path, RV._child_ref(enc, it[1])


def _enc(nodes, ref):
    return nodes[ref] if len(ref) == 32 else ref


def stubs(nodes, root, held):
    """[(prefix nibbles, hash)] of the handle's stubs: the prefix is where the missing node starts
    (past the extension, for a held extension whose branch is missing)."""
    out = []

    def rec(ref, prefix):
        if len(ref) == 32 and ref not in held:
            out.append((prefix, ref))
            return
        node = _decode(_enc(nodes, ref))
        if node[0] == "branch":
            for c, r in enumerate(node[1]):
                if r is not None:
                    rec(r, prefix + [c])
        elif node[0] == "ext":
            rec(node[2], prefix + node[1])

    if root != P.EMPTY_ROOT:
        rec(root, [])
    return out


def keys_held(nodes, root, held):
    """The number of keys whose leaf the handle holds."""
    n = 0
    todo = [root] if root != P.EMPTY_ROOT else []
    while todo:
        ref = todo.pop()
        if len(ref) == 32 and ref not in held:
            continue
        node = _decode(_enc(nodes, ref))
        if node[0] == "branch":
            todo += [r for r in node[1] if r is not None]
        elif node[0] == "ext":
            todo.append(node[2])
        else:
            n += 1
    return n


def fill_nodes(nodes, root, held, encs):
    supply = {P.kec(e) for e in encs}
    held = set(held)
    while True:
        got = {h for _, h in stubs(nodes, root, held) if h in supply}
        if not got:
            return held
        held |= got


def inside(prefix, on, hn):
    return on <= prefix + [0] * (64 - len(prefix)) and prefix + [15] * (64 - len(prefix)) <= hn


def _walk_key(nodes, root, held, kn):
    """Where key kn's walk over the held nodes ends: ("stub", prefix, hash), ("leaf", value) on its
    own leaf, or ("absent",)."""
    ref, d = root, 0
    while True:
        if len(ref) == 32 and ref not in held:
            return "stub", kn[:d], ref
        node = _decode(_enc(nodes, ref))
        if node[0] == "branch":
            if d == 64:
                return ("absent",)  # a value-only branch: no entry can express it
            ref = node[1][kn[d]]
            if ref is None:
                return ("absent",)
            d += 1
        elif node[0] == "ext":
            if kn[d:d + len(node[1])] != node[1]:
                return ("absent",)
            ref, d = node[2], d + len(node[1])
        else:
            return ("leaf", node[2]) if kn[d:] == node[1] else ("absent",)


def whole(root, keys, vals):
    keys, vals = list(keys), list(vals)
    if any(len(v) == 0 for v in vals) or any(a >= b for a, b in zip(keys, keys[1:])):
        return BAD_ORDER
    return OK if RV.rebuilt_root(keys, vals, []) == root else BAD_ROOT


def fill_range(nodes, root, held, origin, keys, vals):
    origin = ZERO if origin is None else origin
    keys, vals = list(keys), list(vals)
    same = Result(None, set(held), 0, 0, set())
    if any(len(v) == 0 for v in vals) or (keys and keys[0] < origin) or any(a >= b for a, b in zip(keys, keys[1:])):
        return same._replace(status=BAD_ORDER)
    on, hn = P.nibbles(origin), P.nibbles(keys[-1] if keys else FF)
    ins = {tuple(p): h for p, h in stubs(nodes, root, held) if inside(p, on, hn)}
    if not keys:
        return same._replace(status=INCOMPLETE if ins else OK)
    missing, bad = set(), False
    under = collections.defaultdict(list)  # reached inside stub -> its entries
    for k, v in zip(keys, vals):
        kn = P.nibbles(k)
        end = _walk_key(nodes, root, held, kn)
        if end[0] == "stub":
            if tuple(end[1]) in ins:
                under[tuple(end[1])].append((kn, v))
            else:
                missing.add(end[2])
        elif end[0] == "leaf":
            bad = bad or end[1] != v  # a resident leaf re-delivered must carry its value
        else:
            bad = True  # a key the trie does not hold
    if missing:
        return same._replace(status=MISSING, missing=missing)
    if bad or set(under) != set(ins):  # (an inside stub no entry reached stands for omitted keys)
        return same._replace(status=BAD_ROOT)
    gained = set()
    for p, items in under.items():
        try:
            enc = RV._node(items, len(p))
        except RV._Moved:
            return same._replace(status=BAD_ROOT)
        if len(enc) < 32 or P.kec(enc) != ins[p]:
            return same._replace(status=BAD_ROOT)
        gained |= PC.subtree(nodes, ins[p])
    return Result(OK, set(held) | gained, sum(len(v) for v in under.values()), len(under), set())
