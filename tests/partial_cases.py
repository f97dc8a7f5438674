"""Helpers shared by the partial-handle tests (tests/test_partial_host.py on the CPU,
tests/test_gpu_partial.py on the device): what a handle opened from a witness holds, read off the
node encodings alone (tests/export_cases._items); nothing of the library is imported."""
from tests import export_cases, proof_ref


def hash_children(enc):
    """The 32-byte child items of a node (a branch's 16 slots, an extension's target), those of the
    nodes embedded in it included."""
    it = export_cases._items(enc)
    if len(it) == 17:
        slots = it[:16]
    elif len(it) == 2 and not (enc[it[0][1]] >> 4) & 2:  # an extension (HexPrefix flag bit 1 clear)
        slots = it[1:2]
    else:
        slots = []
    out = []
    for is_list, q, m in slots:
        if is_list:  # an embedded node (< 32 B): the list item with its one-byte header
            out += hash_children(enc[q - 1:q + m])
        elif m == 32:
            out.append(enc[q:q + m])
    return out


def subtree(nodes, h):
    """The hashes of the stored nodes under h (h included) in the full store `nodes`."""
    out = {h}
    for c in hash_children(nodes[h]):
        out |= subtree(nodes, c)
    return out


def held(witness, root):
    """(held, stubs) of a handle opened from root over the store `witness`: the hashes of the nodes
    it holds (those reachable from the root through the witness) and the hashes its stubs ask for
    (an extension whose branch is absent is held; its one stub asks for the branch)."""
    have, stubs = set(), []
    todo = [root]
    while todo:
        h = todo.pop()
        enc = witness[h]
        kids = hash_children(enc)
        have.add(h)
        for c in kids:
            if c in witness:
                todo.append(c)
            else:
                stubs.append(c)
    return have, stubs


def path_hashes(nodes, root, key):
    """The hashes of expected_proof(nodes, root, key), root first, and the value."""
    proof, val = proof_ref.expected_proof(nodes, root, key)
    return [proof_ref.kec(e) for e in proof], val


def fetchable(nodes, root, keys):
    """Every hash a commit of `keys` on a partial handle may ask for: the nodes of each key's
    expected_proof in the pre-commit store and their 32-byte child items (the path the reference
    walks, and the one child its fix loads)."""
    if root == proof_ref.EMPTY_ROOT:
        return set()
    out = set()
    for k in keys:
        proof, _ = proof_ref.expected_proof(nodes, root, k)
        for e in proof:
            out.add(proof_ref.kec(e))
            out.update(hash_children(e))
    return out
