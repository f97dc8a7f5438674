"""Hand-made commit-witness cases with known answers, shared by tests/test_witness_ref.py (the
reference alone), tests/test_witness_host.py (the host replay) and tests/test_gpu_witness.py.
Nothing of the library is imported.

A case is (name, keys, values, upserts [(key, value)], deletes [key], cover, n_collapse): the
witness is the union over (key, k) of `cover` of the first k nodes (None: all) of
proof_ref.expected_proof(key) in the pre-batch store, n_collapse of them being collapse children.
"""
from tests import proof_ref

# three keys under a root branch (slots 1, 5, 9); hashed leaves with 40-byte values
A, B, C = b"\x11" + b"\xaa" * 31, b"\x52" + b"\xbb" * 31, b"\x93" + b"\xcc" * 31
A2 = b"\x11" + b"\xab" + b"\xaa" * 30  # absent; its walk ends on leaf A
B2 = b"\x57" + b"\xbb" * 31            # with B: a branch in slot 5
B3 = b"\x52" + b"\xbc" + b"\xbb" * 30  # with B: an extension (2, b) in slot 5, then a branch
X, Y, Z = b"\x11" + b"\x01" * 31, b"\x12" + b"\x02" * 31, b"\x53" + b"\x03" * 31  # P{b{x, y}, z}
# two keys that share 62 nibbles: with 1-byte values the leaves and their branch are embedded
E1 = b"\x77" * 31 + b"\x10"
E2 = b"\x77" * 31 + b"\x20"
V = [b"a" * 40, b"b" * 44, b"c" * 48, b"d" * 52]


def hand_cases():
    two = ([A, B], V[:2])
    return [
        ("two_leaves_delete_a", *two, [], [A], [(A, None), (B, None)], 1),
        ("embedded_sibling", [E1, E2], [b"\x01", b"\x02"], [], [E1], [(E1, None)], 0),
        ("sibling_branch", [A, B, B2], V[:3], [], [A], [(A, None), (B, 2)], 1),
        ("sibling_extension", [A, B, B3], V[:3], [], [A], [(A, None), (B, 2)], 1),
        ("cascade", [X, Y, Z], V[:3], [], [X, Y], [(X, None), (Y, None), (Z, None)], 1),
        ("delete_and_fill_a_slot", *two, [(C, V[2])], [A], [(A, None)], 0),
        ("upsert_and_delete_absent", *two, [(C, V[2])], [C], [(C, None)], 0),
        ("upsert_and_delete_present", *two, [(A, V[3])], [A], [(A, None), (B, None)], 1),
        ("delete_everything", *two, [], [A, B], [(A, None), (B, None)], 0),
        ("delete_absent_empty_slot", *two, [], [C], [(C, None)], 0),
        ("delete_absent_under_a_leaf", *two, [], [A2], [(A, None)], 0),
        ("upsert_beside_the_survivor", *two, [(B2, V[2])], [A], [(A, None), (B, None)], 0),
    ]


def want(nodes, root, cover):
    out = set()
    for key, k in cover:
        out.update(proof_ref.kec(e) for e in proof_ref.expected_proof(nodes, root, key)[0][:k])
    return out
