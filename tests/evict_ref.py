"""Reference for subtree eviction (kh_trie_evict_subtrees), written from the contract of
include/khst.h over a {hash: encoding} node set and a root, with the decoders the tests already have
(tests/path_ref.decode over tests/export_cases._items, tests/partial_cases); nothing of the library
is imported.

A prefix names the subtree that HANGS at it: the item the slot of a branch, that many nibbles down,
holds.  Descending from the root a branch consumes one nibble and an extension its nibbles; only a
prefix that ends right after a branch's slot can name a subtree."""
import random

from tests import partial_cases, path_ref

NONE, DONE, STUB, EMBEDDED = 0, 1, 2, 3
# why a prefix reports NONE
CAUSES = ("no_trie", "empty_slot", "in_leaf", "off_leaf", "in_ext", "off_ext", "ext_target", "below_stub")


def locate(nodes, root, nibbles):
    """(status, hash or None, cause or None, item) of one prefix over the set: item is the ("hash",
    h) reference of a DONE prefix."""
    nib = list(nibbles)
    if root is None or root == path_ref.EMPTY_ROOT:
        return NONE, None, "no_trie", None
    cur, pos, after_slot = ("hash", root), 0, False
    while True:
        if pos == len(nib):  # the prefix ends here
            if not after_slot:
                return NONE, None, "ext_target", None  # (the extension's path is where the subtree hangs)
            if cur is None:
                return NONE, None, "empty_slot", None
            if cur[0] == "emb":
                return EMBEDDED, None, None, None
            if cur[1] not in nodes:
                return STUB, cur[1], None, None
            node = path_ref.decode(nodes[cur[1]])
            if node[0] == "ext" and node[2][0] == "hash" and node[2][1] not in nodes:
                return STUB, node[2][1], None, None  # the held extension of a missing branch: one stub with it
            return DONE, cur[1], None, cur
        if cur is None:
            return NONE, None, "empty_slot", None
        if cur[0] == "hash" and cur[1] not in nodes:
            return NONE, None, "below_stub", None
        node = path_ref.decode(nodes[cur[1]] if cur[0] == "hash" else cur[1])
        rest = nib[pos:]
        if node[0] == "branch":
            cur, pos, after_slot = node[1][nib[pos]], pos + 1, True
            continue
        own = list(node[1])
        fits = rest[:len(own)] == own[:len(rest)]
        if node[0] == "leaf":  # (a 32-byte key's leaf ends at nibble 64: no prefix ends below it)
            return NONE, None, "in_leaf" if fits else "off_leaf", None
        if len(rest) < len(own) or not fits:
            return NONE, None, "in_ext" if fits else "off_ext", None
        cur, pos, after_slot = node[2], pos + len(own), False


def _key(nibbles):
    assert len(nibbles) == 64
    return bytes((nibbles[2 * i] << 4) | nibbles[2 * i + 1] for i in range(32))


def subtree_stats(nodes, ref, path):
    """What hangs at ref (a ("hash", h) or ("emb", enc) item at the nibble path `path`) within the
    set: (hashes held, keys, hashes of the stubs inside, records).  A record is a leaf, a branch
    (with the extension above it) or a stub."""
    hashes, keys, stubs, recs = set(), [], [], 0
    todo = [(tuple(path), ref)]
    while todo:
        p, r = todo.pop()
        if r[0] == "hash":
            if r[1] not in nodes:
                stubs.append(r[1])
                recs += 1
                continue
            hashes.add(r[1])
            node = path_ref.decode(nodes[r[1]])
        else:
            node = path_ref.decode(r[1])
        if node[0] == "leaf":
            keys.append(_key(list(p) + list(node[1])))
            recs += 1
        elif node[0] == "ext":
            todo.append((p + tuple(node[1]), node[2]))
        else:
            recs += 1
            if len(p) == 64:  # khipu's value-only branch holds the key that ends there
                keys.append(_key(list(p)))
            for c in range(16):
                if node[1][c] is not None:
                    todo.append((p + (c,), node[1][c]))
    return hashes, keys, stubs, recs


def evict(nodes, root, prefixes):
    """The eviction of `prefixes` (nibble sequences, none equal to or extending another) from the
    handle that holds the set `nodes` under `root`.  Returns a dict:
      status    [(status, hash or None)] per prefix
      cause     [cause or None] per prefix (why NONE)
      removed   the hashes of the evicted subtrees
      held      the hashes still held, stubs the hashes the stubs ask for (sorted): what a handle
                opened from the set without `removed` holds (partial_cases.held)
      keys      the keys evicted (a set), records the records that died (the anchors' own records,
                rewritten as stubs, not among them), evicted the DONE prefixes, stubs_died the
                stubs inside the evicted subtrees"""
    status, cause, removed, keys = [], [], set(), set()
    records = stubs_died = evicted = 0
    for p in prefixes:
        st, h, why, item = locate(nodes, root, p)
        status.append((st, h))
        cause.append(why)
        if st != DONE:
            continue
        hs, ks, stubs, recs = subtree_stats(nodes, item, p)
        removed |= hs
        keys |= set(ks)
        records += recs - 1
        stubs_died += len(stubs)
        evicted += 1
    if root is None or root == path_ref.EMPTY_ROOT:
        held, stubs = set(), []
    else:
        held, stubs = partial_cases.held({h: e for h, e in nodes.items() if h not in removed}, root)
    return {"status": status, "cause": cause, "removed": removed, "held": held, "stubs": sorted(stubs),
            "keys": keys, "records": records, "evicted": evicted, "stubs_died": stubs_died}


def queries(nodes, root, seed=0):
    """{kind: [prefix]} drawn from one state by construction (as tests/path_cases.py):
      hung        every stored path of depth >= 1 whose parent is a branch
      empty_slot  an empty slot of each branch
      inside_ext  a cut inside each extension of 2 or more nibbles
      ext_target  each extension's target path
      below_leaf  one nibble into each leaf's own path
      embedded    every embedded node's path whose parent is a branch"""
    r = random.Random(seed)
    q = {k: [] for k in ("hung", "empty_slot", "inside_ext", "ext_target", "below_leaf", "embedded")}
    for path, ref, node in path_ref.walk(nodes, root):
        if node[0] == "branch":
            empty = [c for c in range(16) if node[1][c] is None]
            if empty and len(path) < 64:
                q["empty_slot"].append(path + (r.choice(empty),))
            for c in range(16):
                kid = node[1][c]
                if kid is None or len(path) >= 64:
                    continue
                if kid[0] == "emb":
                    q["embedded"].append(path + (c,))
                elif kid[1] in nodes:
                    q["hung"].append(path + (c,))
        elif node[0] == "ext":
            ext = tuple(node[1])
            if len(ext) >= 2:
                q["inside_ext"].append(path + ext[:r.randrange(1, len(ext))])
            q["ext_target"].append(path + ext)
        elif len(path) < 64:
            q["below_leaf"].append(path + (node[1][0],))
    return q


def antichain(prefixes):
    """The prefixes none of which equals or extends an earlier kept one (list order decides)."""
    kept = []
    for p in prefixes:
        p = tuple(p)
        if not any(p[:len(k)] == k or k[:len(p)] == p for k in kept):
            kept.append(p)
    return kept
