"""The independent proof checker of the proof tests, written from the RLP, HexPrefix and
Merkle-Patricia-trie rules alone (nothing of the library is imported).

expected_proof(nodes, root, key): the nodes MerklePatriciaTrie.get visits from the root in a node
store {hash: encoding} (oracle.Trie.reachable()), listed root first; a node embedded in its parent
is walked in place and not listed.  Returns (proof, value), value None for an absent key.

check_proof(root, key, proof): (status, value) by the walk kh_verify_proofs documents; the first
condition met, in walk order, decides the status.
"""
from oracle import oracle  # (kec256 only: the CPU oracle's Keccak)

ABSENT, VALUE, BAD_HASH, BAD_NODE, SHORT, EXTRA = range(6)
EMPTY_ROOT = bytes.fromhex("56e81f171bcc55a6ff8345e692c0f86e5b48e01b996cadc001622fb5e363b421")


def kec(b):
    return oracle.kec256(bytes(b))


def nibbles(key):
    return [x for b in key for x in (b >> 4, b & 15)]


class Bad(Exception):
    pass


def rlp_item(d, pos, end):
    """The item at d[pos] inside d[:end]: (is_list, payload start, payload end)."""
    if pos >= end:
        raise Bad
    p = d[pos]
    if p < 0x80:
        is_list, off, ln = False, pos, 1
    elif p <= 0xB7:
        is_list, off, ln = False, pos + 1, p - 0x80
    elif p < 0xC0 or p > 0xF7:
        ll = p - 0xB7 if p < 0xC0 else p - 0xF7
        if ll > 4 or pos + 1 + ll > end:
            raise Bad
        is_list, off, ln = p >= 0xC0, pos + 1 + ll, int.from_bytes(d[pos + 1:pos + 1 + ll], "big")
    else:
        is_list, off, ln = True, pos + 1, p - 0xC0
    if off + ln > end:
        raise Bad
    return is_list, off, off + ln


def list_items(d, pos, end):
    """The node at d[pos]: a list; returns (its end, [(is_list, start of item, payload start, payload end)])."""
    is_list, a, b = rlp_item(d, pos, end)
    if not is_list:
        raise Bad
    out, p = [], a
    while p < b:
        l, s, e = rlp_item(d, p, end)
        if e > b:
            raise Bad
        out.append((l, p, s, e))
        p = e
    return b, out


def _walk(root, key, next_node):
    """The shared walk.  next_node(expected hash) -> encoding, or raises _Stop(status).  Returns
    (status ABSENT / VALUE / BAD_NODE, value)."""
    kn = nibbles(key)
    nib = 0
    expect = root
    while True:
        d = next_node(expect)
        pos, top = 0, True
        while True:  # the listed node, then the nodes embedded in it
            try:
                end, it = list_items(d, pos, len(d))
            except Bad:
                return BAD_NODE, None
            if top and end != len(d):
                return BAD_NODE, None
            top = False
            if len(it) == 17:
                if nib == 64:
                    l, _, s, e = it[16]
                    if l:
                        return BAD_NODE, None
                    return (VALUE, bytes(d[s:e])) if e > s else (ABSENT, None)
                c = kn[nib]
                nib += 1
            elif len(it) == 2:
                l, _, s, e = it[0]
                if l or e == s:
                    return BAD_NODE, None
                hp = nibbles(d[s:e])
                flag = hp[0]
                if flag > 3 or (not flag & 1 and hp[1]):
                    return BAD_NODE, None
                path = hp[1:] if flag & 1 else hp[2:]
                if nib + len(path) > 64:
                    return BAD_NODE, None
                leaf = bool(flag & 2)
                if leaf and it[1][0]:
                    return BAD_NODE, None
                if kn[nib:nib + len(path)] != path or (leaf and nib + len(path) != 64):
                    return ABSENT, None
                if leaf:
                    return VALUE, bytes(d[it[1][2]:it[1][3]])
                nib += len(path)
                c = 1
            else:
                return BAD_NODE, None
            l, start, s, e = it[c]
            if not l:
                if e == s:
                    return ABSENT, None
                if e - s != 32:
                    return BAD_NODE, None
                expect = bytes(d[s:e])
                break
            if e - start >= 32:
                return BAD_NODE, None
            pos = start


class _Stop(Exception):
    def __init__(self, status):
        self.status = status


def expected_proof(nodes, root, key):
    """(the list of encodings on key's path from root through the store `nodes`, the value or None)."""
    proof = []
    if root == EMPTY_ROOT:
        return proof, None

    def nxt(h):
        proof.append(nodes[h])
        return nodes[h]
    st, val = _walk(root, key, nxt)
    assert st in (ABSENT, VALUE), st
    return proof, val


def check_proof(root, key, proof):
    proof = list(proof)
    if not proof:
        return (ABSENT if root == EMPTY_ROOT else SHORT), None
    k = [0]

    def nxt(h):
        if k[0] == len(proof):
            raise _Stop(SHORT)
        d = proof[k[0]]
        k[0] += 1
        if kec(d) != h:
            raise _Stop(BAD_HASH)
        return d
    try:
        st, val = _walk(root, key, nxt)
    except _Stop as s:
        return s.status, None
    if st == BAD_NODE:
        return st, None
    if k[0] != len(proof):
        return EXTRA, None
    return st, val
