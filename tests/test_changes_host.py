"""CPU: the changes since a savepoint of khipu_amd/csrc/changes.h replayed on the host under
AddressSanitizer and UBSan.  tests/changes_host/changes_check.cc (a stand-alone program) takes
hand-made record arrays -- the handle's records now, the journal's saved copies with their indices,
the savepoint's record count and journal fill, one heap -- and runs collect, order, join and page as
range_kernels.hip does, into outputs of exactly the scanned sizes.  Every answer must equal
tests/changes_ref.expected over the two dicts the same scenario stands for."""
import subprocess

import pytest

from tests import changes_ref as CR
from tests import hostprog
from tests.hostprog import hexs as _hex
from tests.hostprog import unhexs as _unhex

BIG = 1 << 30
prog = hostprog.prog_fixture("changes")


def K(i):
    """A 32-byte key whose first 8 bytes differ for the i in use, i big-endian in its last 4 bytes."""
    return bytes([i % 251 + 1]) * 8 + bytes(20) + i.to_bytes(4, "big")


class Scenario:
    """Record arrays and the two contents they stand for.  Records before `savepoint()` are the
    savepoint's; journal copies before it belong to an enclosing savepoint."""

    def __init__(self, forest=False):
        self.forest = forest
        self.R, self.J = [], []
        self.rn0 = self.j0 = 0
        self.before, self.after = {}, {}

    def rec(self, t, k, kind, v=b""):
        self.R.append((t, k, kind, v))
        return len(self.R) - 1

    def save(self, idx, t, k, kind, v=b""):
        self.J.append(("-" if idx is None else idx, t, k, kind, v))

    def savepoint(self):
        self.rn0, self.j0 = len(self.R), len(self.J)

    def kill(self, idx):
        t, k, kind, v = self.R[idx]
        self.R[idx] = (t, k, kind.lower(), v)

    def text(self, queries):
        lines = [f"F {int(self.forest)}"]
        lines += [f"R {t} {k.hex()} {kind} {_hex(v)}" for t, k, kind, v in self.R]
        lines += [f"J {i} {t} {k.hex()} {kind} {_hex(v)}" for i, t, k, kind, v in self.J]
        lines += [f"S {self.rn0} {self.j0}"]
        lines += [f"Q {int(rev)} {st[0] if st else 0} {st[1].hex() if st else '-'} {mx} {cap}" for rev, st, mx, cap in queries]
        return "\n".join(lines) + "\n"

    # ---- what commits do to the arrays, with the model kept beside them
    def old_leaf(self, t, k, v, vb=False):
        """a leaf of the savepoint's version"""
        self.before[(t, k)] = self.after[(t, k)] = (v, vb)
        return self.rec(t, k, "V" if vb else "L", v)

    def delete(self, idx):
        t, k, kind, v = self.R[idx]
        self.save(idx, t, k, kind, v)
        self.kill(idx)
        self.after.pop((t, k), None)

    def put(self, t, k, v, old=None, vb=False):
        if old is not None:
            self.delete(old)
        self.after[(t, k)] = (v, vb)
        return self.rec(t, k, "V" if vb else "L", v)

    def reanchor(self, idx):
        """saved, then written again at its index with the same key and value span"""
        t, k, kind, v = self.R[idx]
        self.save(idx, t, k, kind, v)


def _run(prog, tmp_path, sc, queries, tag=""):
    p = tmp_path / f"in{tag}.txt"
    p.write_text(sc.text(queries))
    r = subprocess.run([prog, str(p)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])  # (a sanitizer report ends the program non-zero)
    ans, passes = [], []
    for x in (ln.split() for ln in r.stdout.split("\n")[:-1]):
        assert x[0] == "A"
        if x[1] == "nospc":
            ans.append(("nospc", int(x[2]), int(x[3])))
            passes.append(None)
            continue
        k, more = int(x[2]), x[3] == "1"
        ents = [(int(x[8 + 4 * i]), bytes.fromhex(x[9 + 4 * i]), int(x[10 + 4 * i]), _unhex(x[11 + 4 * i])) for i in range(k)]
        ans.append(("page", ents, more, (int(x[4]), bytes.fromhex(x[5])) if more else None, int(x[6])))
        passes.append(int(x[7]))
    assert len(ans) == len(queries)
    return ans, passes


def _check(prog, tmp_path, sc, queries, tag=""):
    got, passes = _run(prog, tmp_path, sc, queries, tag)
    for (rev, st, mx, cap), g in zip(queries, got):
        assert g == CR.expected(sc.before, sc.after, rev, st, mx, cap), (rev, st, mx, cap)
    return got, passes


def _block():
    """One trie: everything a journal can hold, beside the keys it must not report."""
    sc = Scenario()
    # an enclosing savepoint's journal: the copy of a record deleted BEFORE this savepoint
    sc.save(sc.rec(0, K(900), "l", b"older than the savepoint"), 0, K(900), "L", b"older than the savepoint")
    keep = sc.old_leaf(0, K(1), b"untouched")
    gone = sc.old_leaf(0, K(2), b"deleted")
    chg = sc.old_leaf(0, K(3), b"old value")
    anch = sc.old_leaf(0, K(4), b"re-anchored only")
    twice = sc.old_leaf(0, K(5), b"saved twice")
    back = sc.old_leaf(0, K(6), b"deleted and put back")
    lasts = [sc.old_leaf(0, K(10 + n), bytes([7]) * (n - 1) + b"\x01") for n in (1, 33, 56, 300)]
    tovb = sc.old_leaf(0, K(20), b"same value, other node")
    anch2 = sc.old_leaf(0, K(21), b"re-anchored, then changed")
    br = sc.rec(0, K(30), "B")
    sc.savepoint()
    sc.delete(gone)
    sc.put(0, K(3), b"new value", old=chg)
    sc.reanchor(anch)
    # saved when it was re-anchored, saved again when a later commit killed it: the second copy is of
    # the record as the first commit left it -- here made DEAD, so only the earliest copy can count
    sc.reanchor(twice)
    sc.save(twice, 0, K(5), "l", b"saved twice")
    sc.kill(twice)
    sc.after.pop((0, K(5)))
    sc.put(0, K(6), b"deleted and put back", old=back)
    for n, idx in zip((1, 33, 56, 300), lasts):
        sc.put(0, K(10 + n), bytes([7]) * (n - 1) + b"\x02", old=idx)
    sc.put(0, K(20), b"same value, other node", old=tovb, vb=True)
    sc.reanchor(anch2)
    sc.put(0, K(21), b"changed after the re-anchor", old=anch2)
    sc.save(br, 0, K(30), "B")                       # a branch rewritten in place: no entry
    sc.save(None, 0, K(40), "L", b"jidx is NONE")    # a slot of k_rec_save's second list that held no source
    new = sc.put(0, K(50), b"created")
    tmp = sc.put(0, K(51), b"created and deleted again")
    sc.delete(tmp)                                   # its copy has an index past the savepoint's records
    sc.put(0, K(52), b"created, then changed", old=sc.put(0, K(52), b"created"))
    assert new > sc.rn0
    return sc


def test_host_block_of_every_journal_case(prog, tmp_path):
    sc = _block()
    full = CR.differences(sc.before, sc.after)
    kinds = {k: kind for _, k, kind, _ in full}
    assert kinds[K(2)] == 1 and kinds[K(3)] == 3 and kinds[K(5)] == 1 and kinds[K(20)] == 3 and kinds[K(21)] == 3
    assert kinds[K(50)] == 2 and kinds[K(52)] == 2 and all(kinds[K(10 + n)] == 3 for n in (1, 33, 56, 300))
    assert not {K(1), K(4), K(6), K(30), K(40), K(51), K(900)} & set(kinds)
    q = [(rev, None, mx, BIG) for rev in (False, True) for mx in (1000, len(full), len(full) - 1, 1)]
    got, passes = _check(prog, tmp_path, sc, q)
    assert got[0][1] == full and got[0][4] == len(full)
    assert set(passes) == {1}  # (distinct first words: one pass, no tie)
    # the reverse answer carries the SAVEPOINT's values, the deleted key's among them
    rev = {k: (kind, v) for _, k, kind, v in got[4][1]}
    assert rev[K(2)] == (2, b"deleted") and rev[K(5)] == (2, b"saved twice") and rev[K(50)] == (1, b"")
    assert rev[K(20)] == (3, b"same value, other node")


def test_host_enclosing_savepoint_sees_the_older_copy(prog, tmp_path):
    """The same arrays read from journal position 0: the older copy counts, and its key -- absent
    from the records now -- is a kind-1 difference of that outer level."""
    sc = _block()
    sc.j0 = 0
    sc.before[(0, K(900))] = (b"older than the savepoint", False)
    got, _ = _check(prog, tmp_path, sc, [(False, None, 1000, BIG)])
    assert (0, K(900), 1, b"") in got[0][1]


def test_host_paging_resume_and_caps(prog, tmp_path):
    sc = _block()
    full = CR.differences(sc.before, sc.after)
    keys = [k for _, k, _, _ in full]
    between = keys[2][:31] + bytes([keys[2][31] + 1])
    assert keys[2] < between < keys[3]
    q = [(False, (0, keys[3]), 1000, BIG), (False, (0, between), 1000, BIG), (False, (0, keys[-1]), 1000, BIG),
         (False, (0, b"\xff" * 32), 1000, BIG), (True, (0, keys[3]), 2, BIG)]
    got, _ = _check(prog, tmp_path, sc, q, "resume")
    assert got[0][1] == got[1][1] == full[3:] and got[0][4] == len(full) - 3 and got[3][1] == []
    # chained pages of one entry give the one-call answer
    out, start = [], None
    for _ in range(len(full) + 1):
        (g,), _ = _check(prog, tmp_path, sc, [(False, start, 1, BIG)], "chain")
        out += g[1]
        assert g[4] == len(full) - len(out) + len(g[1])
        if not g[2]:
            break
        start = g[3]
    assert out == full
    # val_cap: cut after the first entry that carries a value; too small for it: ENOSPC with n_total
    i = next(i for i, d in enumerate(full) if d[3])
    first = len(full[i][3])
    q = [(False, (0, keys[i]), 1000, first), (False, (0, keys[i]), 1000, first - 1), (False, (0, keys[i]), 1000, 0)]
    got, _ = _check(prog, tmp_path, sc, q, "cap")
    assert len(got[0][1]) >= 1 and got[0][2] and sum(len(e[3]) for e in got[0][1]) <= first
    assert got[1] == got[2] == ("nospc", first, len(full) - i)


def test_host_forest_same_key_in_two_tries(prog, tmp_path):
    sc = Scenario(forest=True)
    a = [sc.old_leaf(t, K(7), b"v%d" % t) for t in (9, 3, 600000)]
    sc.old_leaf(3, K(8), b"quiet")
    sc.savepoint()
    sc.put(9, K(7), b"nine", old=a[0])
    sc.put(3, K(7), b"three", old=a[1])
    sc.delete(a[2])
    sc.put(4, K(7), b"a new trie")
    q = [(False, None, 1000, BIG), (True, None, 1000, BIG), (False, (3, K(8)), 1000, BIG), (False, (4, K(7)), 1, BIG),
         (False, None, 2, BIG)]
    got, passes = _check(prog, tmp_path, sc, q)
    assert [(t, kind) for t, _, kind, _ in got[0][1]] == [(3, 3), (4, 2), (9, 3), (600000, 1)]
    assert got[4][3] == (9, K(7)) and set(passes) == {2}


def test_host_keys_equal_in_their_first_eight_bytes(prog, tmp_path):
    """Dense keys: one stretch of equal first words.  The first order (one word) is flagged and the
    call sorts all four words; keys differing only in word 1, 2 or 3 come out in key order."""
    sc = Scenario()
    head = b"\x42" * 8
    ks = [head + bytes(8 * w) + b"\x01" + bytes(23 - 8 * w) for w in range(3)] + [head + bytes(23) + bytes([i]) for i in (9, 2, 5)]
    ks = [k[:32] for k in ks]
    old = [sc.old_leaf(0, k, b"o" + bytes([i])) for i, k in enumerate(ks)]
    sc.savepoint()
    for i, (k, idx) in enumerate(zip(ks, old)):
        if i % 2:
            sc.put(0, k, b"n" + bytes([i]), old=idx)
        else:
            sc.delete(idx)
    sc.put(0, head + b"\xff" * 24, b"last")
    got, passes = _check(prog, tmp_path, sc, [(False, None, 1000, BIG), (False, None, 3, BIG)])
    assert [k for _, k, _, _ in got[0][1]] == sorted(ks + [head + b"\xff" * 24])
    assert passes == [5, 5]  # one pass, the tie, four passes


def test_host_nothing_changed(prog, tmp_path):
    sc = Scenario()
    a = sc.old_leaf(0, K(1), b"x")
    sc.savepoint()
    got, _ = _check(prog, tmp_path, sc, [(False, None, 5, BIG)], "none")
    assert got == [("page", [], False, None, 0)]
    sc.reanchor(a)
    sc.put(0, K(1), b"x", old=a)  # upserted with the bytes it had
    got, _ = _check(prog, tmp_path, sc, [(False, None, 5, BIG), (True, None, 5, 0)], "same")
    assert got == [("page", [], False, None, 0)] * 2
