"""Reference for nodes by path (snap's GetTrieNodes), written from the contract of DESIGN.md §4
"Nodes by path" over a {hash: encoding} node set and tests/export_cases._items; nothing of the
library is imported.

A path names the node that STARTS after its nibbles: the root at the empty path, a branch's child c
at path + [c], an extension's target at path + the extension's nibbles.  A node is served when a
node store holds it (it is referred to by hash, or it is the root); a node embedded in its parent,
a path that ends inside an extension, below a leaf or in an empty slot give 0."""
from tests import export_cases

EMPTY_ROOT = bytes.fromhex("56e81f171bcc55a6ff8345e692c0f86e5b48e01b996cadc001622fb5e363b421")


def _hp(b):
    """(nibbles, is_leaf) of a HexPrefix string."""
    flag = b[0] >> 4
    nib = [b[0] & 0xF] if flag & 1 else []
    for x in b[1:]:
        nib += [x >> 4, x & 0xF]
    return nib, bool(flag & 2)


def _child(enc, item):
    """A child item of a node: None (empty), ("hash", h) or ("emb", encoding)."""
    is_list, q, m = item
    if is_list:
        return ("emb", enc[q - 1:q + m])  # (an embedded node is < 32 B: a one-byte list header)
    if m == 0:
        return None
    assert m == 32, "a child is empty, a hash or an embedded list"
    return ("hash", enc[q:q + m])


def decode(enc):
    """("branch", [16 children]) | ("ext", nibbles, child) | ("leaf", nibbles)."""
    it = export_cases._items(enc)
    if len(it) == 17:
        return ("branch", [_child(enc, x) for x in it[:16]])
    assert len(it) == 2
    nib, leaf = _hp(enc[it[0][1]:it[0][1] + it[0][2]])
    return ("leaf", nib) if leaf else ("ext", nib, _child(enc, it[1]))


def node_at(nodes, root, nibbles):
    """(1, encoding) the stored node at the path; (0, None) no stored node starts there; (2, None)
    a hash on the way is absent from the set."""
    nib = list(nibbles)
    if root == EMPTY_ROOT:
        return 0, None
    cur, pos = ("hash", root), 0
    while True:
        if cur is None:
            return 0, None  # an empty slot
        if cur[0] == "hash":
            if cur[1] not in nodes:
                return 2, None
            enc = nodes[cur[1]]
            if pos == len(nib):
                return 1, enc
        else:
            enc = cur[1]
            if pos == len(nib):
                return 0, None  # embedded in its parent
        node = decode(enc)
        if node[0] == "leaf":
            return 0, None  # below a leaf
        if node[0] == "branch":
            cur = node[1][nib[pos]]
            pos += 1
            continue
        ext = node[1]
        if len(nib) < pos + len(ext) or nib[pos:pos + len(ext)] != ext:
            return 0, None  # inside the extension, or off it
        pos += len(ext)
        cur = node[2]


def walk(nodes, root):
    """Every node of the set reachable from root, parents first: (path, ref, decoded), ref being
    ("hash", h) or ("emb", encoding).  A hash absent from the set is not entered."""
    if root == EMPTY_ROOT:
        return
    todo = [((), ("hash", root))]
    while todo:
        path, ref = todo.pop()
        if ref[0] == "hash" and ref[1] not in nodes:
            continue
        node = decode(nodes[ref[1]] if ref[0] == "hash" else ref[1])
        yield path, ref, node
        if node[0] == "branch":
            for c in range(15, -1, -1):
                if node[1][c] is not None:
                    todo.append((path + (c,), node[1][c]))
        elif node[0] == "ext":
            todo.append((path + tuple(node[1]), node[2]))


def stored_paths(nodes, root):
    """[(path, hash)] of every stored node of the set reachable from root."""
    return [(path, ref[1]) for path, ref, _ in walk(nodes, root) if ref[0] == "hash"]
