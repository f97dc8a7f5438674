"""The independent reference of the commit-witness tests (kh_trie_commit_witness_host), written from
the node encodings and the key sets alone: nothing of the library is imported.

expected(nodes, root, live_keys, up_keys, del_keys) -> (set of node hashes, n_collapse): the witness
of the batch (upserts up_keys, then deletes del_keys; a key in both is a delete) on the trie
`root` of the store `nodes` {hash: encoding} that holds exactly live_keys (32-byte trie keys).

  (1) the union of proof_ref.expected_proof over the op keys;
  (2) for every branch on those paths (a branch embedded in a listed node included): when exactly
      one of its 16 slots has a key of the POST-BATCH key set under it, and that slot was not empty
      before, the 32-byte item of that slot.  An embedded item adds nothing.

n_collapse counts the hashes of (2) that are not in (1).  Whether a slot survives is decided by
prefix on the sorted post-batch keys, not by walking the trie bottom-up as the device does.
"""
import bisect

from tests import proof_ref


def _branches(nodes, root, key):
    """[(nibble prefix of the branch as a hex string, its 17 items, its bytes)] for the branch
    nodes MerklePatriciaTrie.get passes on key's path, those embedded in a stored node included."""
    out = []
    if root == proof_ref.EMPTY_ROOT:
        return out
    kn = proof_ref.nibbles(key)
    hexkey = key.hex()
    nib, expect = 0, root
    while True:
        d = nodes[expect]
        pos = 0
        while True:
            _, it = proof_ref.list_items(d, pos, len(d))
            if len(it) == 17:
                out.append((hexkey[:nib], it, d))
                if nib == 64:
                    return out
                c = kn[nib]
                nib += 1
            else:
                _, _, s, e = it[0]
                hp = proof_ref.nibbles(d[s:e])
                path = hp[1:] if hp[0] & 1 else hp[2:]
                if hp[0] & 2 or kn[nib:nib + len(path)] != path:
                    return out  # a leaf, or the key leaves the extension
                nib += len(path)
                c = 1
            is_list, start, s, e = it[c]
            if not is_list:
                if e == s:
                    return out
                expect = bytes(d[s:e])
                break
            pos = start


def expected(nodes, root, live_keys, up_keys, del_keys):
    dels = set(del_keys)
    post = sorted(k.hex() for k in (set(live_keys) | set(up_keys)) - dels)

    def occupied(prefix):
        i = bisect.bisect_left(post, prefix)
        return i < len(post) and post[i].startswith(prefix)

    paths, extra = set(), set()
    seen = set()
    for k in list(up_keys) + list(del_keys):
        for e in proof_ref.expected_proof(nodes, root, k)[0]:
            paths.add(proof_ref.kec(e))
        for prefix, it, d in _branches(nodes, root, k):
            if prefix in seen:
                continue
            seen.add(prefix)
            left = [c for c in range(16) if occupied(prefix + "0123456789abcdef"[c])]
            if len(left) != 1:
                continue
            is_list, _, s, e = it[left[0]]
            if not is_list and e - s == 32:  # (an old slot referred to by hash; empty: e == s)
                extra.add(bytes(d[s:e]))
    return paths | extra, len(extra - paths)
