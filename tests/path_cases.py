"""Queries for nodes by path, drawn from a state by construction so that every kind of answer is
asked for without a percentage to meet (tests/test_path_ref.py)."""
import random

from tests import path_ref


def queries(nodes, root, seed=0):
    """{kind: [path]} over the node set of one state:
      stored      every stored node's path (each must be found, with its bytes and hash)
      empty_slot  for each branch with an empty slot, its path + that nibble
      inside_ext  for each extension of 2 or more nibbles, its path cut inside it
      below_leaf  for each leaf that ends above depth 64, its path + 1 nibble
      embedded    every embedded node's path
      mismatch    for each extension, the path of its target with the last nibble changed
      random      50 random paths of random length"""
    r = random.Random(seed)
    q = {k: [] for k in ("stored", "empty_slot", "inside_ext", "below_leaf", "embedded", "mismatch", "random")}
    for path, ref, node in path_ref.walk(nodes, root):
        q["stored" if ref[0] == "hash" else "embedded"].append(path)
        if node[0] == "branch":
            empty = [c for c in range(16) if node[1][c] is None]
            if empty and len(path) < 64:
                q["empty_slot"].append(path + (r.choice(empty),))
        elif node[0] == "ext":
            ext = tuple(node[1])
            if len(ext) >= 2:
                q["inside_ext"].append(path + ext[:r.randrange(1, len(ext))])
            q["mismatch"].append(path + ext[:-1] + (ext[-1] ^ (1 + r.randrange(15)),))
        elif len(path) < 64:
            q["below_leaf"].append(path + (node[1][0],))
    for _ in range(50):
        q["random"].append(tuple(r.randrange(16) for _ in range(r.randrange(65))))
    return q


def flat(q):
    """[(kind, path)] in a fixed order."""
    return [(k, p) for k in sorted(q) for p in q[k]]

