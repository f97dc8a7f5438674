"""Responses for the range-verification tests (tests/test_rangeverify_ref.py pins their conditions
on the CPU; tests/test_rangeverify_host.py and tests/test_gpu_rangeverify.py run them).  No GPU,
no library: a response is cut from the content of a state (tests/range_ref.content) and carries
the nodes of tests/proof_ref.expected_proof for its two boundary keys.

A response is a dict: origin, keys, vals, nodes (a list of encodings, duplicates included), more,
max (the max_entries it was cut at).
tampers(r, resp, items, nodes, root) lists (kind, response, proved, expected): expected is the
status the contract of kh_verify_ranges assigns to that kind of tamper -- (status, more or None,
missing or None) -- worked out from the kind, not by running a verifier.
"""
import random

from tests import proof_ref as P
from tests import range_cases as RC

OK, BAD_ORDER, MISSING, BAD_NODE, BAD_ROOT, INCOMPLETE = range(6)
N_RESPONSES = 40


def _proof_nodes(nodes, root, key):
    return P.expected_proof(nodes, root, key)[0]


def response(items, nodes, root, origin, max_entries):
    """The honest response for (origin, max_entries) over the content `items` (sorted (key, value))."""
    inr = [(k, v) for k, v in items if k >= origin]
    page = inr[:max_entries]
    keys, vals = [k for k, _ in page], [v for _, v in page]
    enc = _proof_nodes(nodes, root, origin) + _proof_nodes(nodes, root, keys[-1] if keys else origin)
    return {"origin": origin, "keys": keys, "vals": vals, "nodes": enc, "more": len(inr) > len(page),
            "max": max_entries}


def seed(i, b):
    return random.Random(7000 + 100 * i + b)


def responses(r, items, nodes, root, n=N_RESPONSES):
    """n honest responses of a state: origin at, next to or between present keys (0.85) or zero,
    max_entries from range_cases.MAXES."""
    keys = [k for k, _ in items]
    out = []
    for _ in range(n):
        origin = RC._point(r, keys) if r.random() < 0.85 else RC.ZERO
        out.append(response(items, nodes, root, origin, r.choice(RC.MAXES)))
    return out


def busy(resp, items):
    """An entry, `more` and a key below origin all at once: both boundary paths keep subtrees."""
    return bool(resp["keys"]) and resp["more"] and bool(items) and items[0][0] < resp["origin"]


def _with(resp, **kw):
    out = dict(resp)
    out.update(kw)
    return out


def tampers(r, resp, items, nodes, root):
    o, ks, vs, enc = resp["origin"], resp["keys"], resp["vals"], resp["nodes"]
    m = len(ks)
    present = {k for k, _ in items}
    out = []
    if m >= 3:
        j = r.randrange(1, m - 1)
        out.append(("drop_middle", _with(resp, keys=ks[:j] + ks[j + 1:], vals=vs[:j] + vs[j + 1:]), 1,
                    (BAD_ROOT, None, None)))
    if m >= 2:
        out.append(("drop_first", _with(resp, keys=ks[1:], vals=vs[1:]), 1, (BAD_ROOT, None, None)))
        # cut at its end, with the new last key's path: still the trie's content up to that key
        out.append(("drop_last", _with(resp, keys=ks[:-1], vals=vs[:-1], nodes=enc + _proof_nodes(nodes, root, ks[-2])),
                    1, (OK, True, None)))
        j = r.randrange(m - 1)
        out.append(("swap", _with(resp, keys=ks[:j] + [ks[j + 1], ks[j]] + ks[j + 2:],
                                  vals=vs[:j] + [vs[j + 1], vs[j]] + vs[j + 2:]), 1, (BAD_ORDER, None, None)))
        j = r.randrange(m - 1)
        mid = RC._step(ks[j], 1)
        if mid < ks[j + 1] and mid not in present:
            out.append(("insert_between", _with(resp, keys=ks[:j + 1] + [mid] + ks[j + 1:],
                                                vals=vs[:j + 1] + [vs[j]] + vs[j + 1:]), 1, (BAD_ROOT, None, None)))
    if m >= 1:
        j = r.randrange(m)
        v = bytearray(vs[j])
        v[r.randrange(len(v))] ^= 1 << r.randrange(8)
        out.append(("flip_value", _with(resp, vals=vs[:j] + [bytes(v)] + vs[j + 1:]), 1, (BAD_ROOT, None, None)))
        j = r.randrange(m)
        out.append(("repeat", _with(resp, keys=ks[:j + 1] + ks[j:], vals=vs[:j + 1] + vs[j:]), 1,
                    (BAD_ORDER, None, None)))
        j = r.randrange(m)
        out.append(("empty_value", _with(resp, vals=vs[:j] + [b""] + vs[j + 1:]), 1, (BAD_ORDER, None, None)))
        if ks[0] != RC.FF:
            out.append(("raise_origin", _with(resp, origin=RC._step(ks[0], 1)), 1, (BAD_ORDER, None, None)))
        if resp["more"] or (items and items[0][0] < o):
            out.append(("claim_whole", resp, 0, (BAD_ROOT, None, None)))
    if o != RC.ZERO:
        out.append(("insert_below_origin", _with(resp, keys=[RC._step(o, -1)] + ks, vals=[b"\x01"] + vs), 1,
                    (BAD_ORDER, None, None)))
    # one node withheld from each boundary path (every copy of it): the walk that needs it stops there
    for name, key in (("withhold_origin_path", o), ("withhold_last_path", ks[-1] if ks else o)):
        path = _proof_nodes(nodes, root, key)
        if path:
            gone = r.choice(path)
            out.append((name, _with(resp, nodes=[e for e in enc if e != gone]), 1, (MISSING, None, P.kec(gone))))
    return out
