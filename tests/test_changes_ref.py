"""CPU: the model of the changes-since tests (tests/changes_ref.py, two dicts) against the trie-diff
reference (tests/diff_ref.py and tests/diffs_ref.py, over the oracle's node stores): the tries built
from the two dicts must diff to exactly what the model says, paged and cut the same way."""
import random

from tests import cases as C
from tests import changes_ref as CR
from tests import diff_cases as DC
from tests import diff_ref as DR
from tests import diffs_ref as DSR
from tests import hostprog
from tests import proof_cases


def _snap(oracle, d, t):
    """The oracle's trie of trie id t of a model dict (no value-only branches)."""
    return DC.snap(hostprog.trie(oracle, [k for (u, k) in sorted(d) if u == t], [d[(u, k)][0] for (u, k) in sorted(d) if u == t]))


def _two_versions(seed, n=120, tries=(0,)):
    r = random.Random(seed)
    before = {(t, C._rk(r)): (C.account_value(r), False) for t in tries for _ in range(n)}
    after = dict(before)
    keys = sorted(before)
    for tk in r.sample(keys, n // 4):
        del after[tk]
    for tk in r.sample(sorted(after), n // 4):
        after[tk] = (C.account_value(r), False)
    for t in tries:
        for _ in range(n // 5):
            after[(t, C._rk(r))] = (C.account_value(r), False)
    return before, after


def test_model_matches_the_diff_reference_single_trie(oracle):
    before, after = _two_versions(5)
    (na, ra), (nb, rb) = _snap(oracle, before, 0), _snap(oracle, after, 0)
    for rev, (x, y) in ((False, ((na, ra), (nb, rb))), (True, ((nb, rb), (na, ra)))):
        full = CR.differences(before, after, rev)
        assert [(k, kind, v) for _, k, kind, v in full] == DR.content_diff(*x, *y)
        starts = [None, full[3][1], DC.RC._step(full[3][1], 1), full[-1][1]]
        for start in starts:
            for mx, cap in ((1, 1 << 20), (7, 1 << 20), (1000, 1 << 20), (1000, 200), (5, 0)):
                want = DR.expected_diff(*x, *y, start, None, mx, cap)
                got = CR.expected(before, after, rev, None if start is None else (0, start), mx, cap)
                if want[0] == "nospc":
                    assert got[:2] == want
                else:
                    assert got[0] == "page" and [(k, kind, v) for _, k, kind, v in got[1]] == want[1]
                    assert got[2] == want[2] and (got[3][1] if got[3] else None) == want[3]
                n_from = sum(1 for d in full if start is None or d[1] >= start)
                assert got[-1] == n_from


def test_model_matches_the_batched_reference_forest(oracle):
    tries = (3, 4, 900)
    before, after = _two_versions(6, n=40, tries=tries)
    for tk in [tk for tk in after if tk[0] == 4]:  # trie 4 is emptied, trie 77 is new
        del after[tk]
    r = random.Random(1)
    for _ in range(10):
        after[(77, C._rk(r))] = (C.account_value(r), False)
    ids = sorted(set(t for t, _ in before) | set(t for t, _ in after))
    sa = {t: _snap(oracle, before, t) for t in ids}
    sb = {t: _snap(oracle, after, t) for t in ids}
    reqs = [(t, None, None, None) for t in ids]
    for mx, cap in ((1000, 1 << 20), (9, 1 << 20), (1000, 300)):
        want = DSR.expected_diffs(sa, sb, reqs, mx, cap)
        got = CR.expected(before, after, False, None, mx, cap)
        assert want[0] == "pages" and got[0] == "page"
        flat = [(ids[q], k, kind, v) for q, page in enumerate(want[1]) for k, kind, v in page]
        assert got[1] == flat
        # the cut request and its next key are the model's next pair
        assert got[3] == ((ids[want[2]], want[3]) if want[2] < len(ids) else None) and got[2] == (want[2] < len(ids))
    assert {t for t, _, _, _ in CR.differences(before, after)} >= {4, 77}


def test_model_value_only_branch(oracle):
    """hostprog.vb_trie: a re-put under a depth-63 branch makes a value-only branch -- against the
    plain trie of the same keys and values the key is a kind-3 difference of equal values."""
    ks, vs, blocks, _ = proof_cases.vb_case(False)
    o_vb, n = hostprog.vb_trie(oracle)
    live = {k: o_vb.get(k) for k in ks}
    plain = hostprog.trie(oracle, list(live), list(live.values()))
    before = {(0, k): (v, False) for k, v in live.items()}
    # the re-put keys of the block that have a sibling sharing 63 nibbles are the value-only branches
    vbk = sorted(k for k, _ in blocks[0][0] if k[:31] + bytes([k[31] ^ 1]) in live)
    assert len(vbk) == 2
    after = {(0, k): (v, k in vbk) for k, v in live.items()}
    assert n == len(live)
    want = DR.content_diff(*DC.snap(plain), *DC.snap(o_vb))
    assert want == [(k, 3, live[k]) for k in vbk]
    assert [(k, kind, v) for _, k, kind, v in CR.differences(before, after)] == want
    assert [(k, kind, v) for _, k, kind, v in CR.differences(before, after, True)] == DR.content_diff(
        *DC.snap(o_vb), *DC.snap(plain))


def test_model_ops_and_no_differences():
    before, after = _two_versions(8)
    assert CR.expected(before, before) == ("page", [], False, None, 0)
    ups, dels = CR.ops(CR.differences(before, after))
    d = dict(before)
    for t, k in dels:
        del d[(t, k)]
    for t, k, v in ups:
        d[(t, k)] = (v, False)
    assert d == after
