"""CPU: the digest forms of khipu_amd/csrc/keccak.h -- the last round that computes lanes 0..3 only
(keccak_round_digest, keccakf_digest), the hashes that end in it (kec256_msg_digest,
kec256_short_digest) and the one-block hash of a compile-time length (kec256_fixed) -- run on the
host by tests/keccak_host/keccak_check.cc (a stand-alone program) and compared with the full
permutation, with kec256_short / kec256_msg, with the oracle's Keccak and with known vectors.  The
program runs twice: built plain, and built with AddressSanitizer and UBSan (every message is placed
at all 8 byte alignments in a buffer that ends with its last aligned word, so a read outside the
message's aligned span is reported)."""
import os
import random
import subprocess

import pytest

from tests import hostprog

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "keccak_host", "keccak_check.cc")

KNOWN = {  # Keccak-256 (0x01 padding)
    b"": "c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470",
    b"abc": "4e03657aea45a94fc7d47ba826c8d667c0d1e6e33a64a036ec44f58fa12d6c45",
}
LENGTHS = (0, 1, 7, 8, 19, 20, 21, 31, 32, 33, 134, 135)  # the generic form; 136 and up: more than one block
LONG = (136, 137, 200, 271, 272, 300)
N_STATES = 10_000


def _messages():
    r = random.Random(2025)
    msgs = list(KNOWN)
    for ln in LENGTHS + LONG:
        msgs += [bytes(r.getrandbits(8) for _ in range(ln)) for _ in range(3)]
    for ln in (20, 32):  # the fixed-length forms: more inputs, the all-zero and all-ones words among them
        msgs += [bytes(ln), b"\xff" * ln] + [bytes(r.getrandbits(8) for _ in range(ln)) for _ in range(60)]
    return msgs


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "sanitized"])
def out(request, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("keccak_host")
    if request.param:
        exe = hostprog.compile_prog(SRC, tmp / "keccak_check_san")
    else:
        exe = hostprog.compile_prog(SRC, tmp / "keccak_check", ["-O2", "-std=c++17"])
    text = f"P {N_STATES} 7\n" + "".join(f"M {m.hex() or '-'}\n" for m in _messages())
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]  # (a sanitizer report ends the program with a non-zero status)
    rows = [ln.split() for ln in r.stdout.split("\n") if ln]
    per_msg, k = [], 0
    p = [x for x in rows if x[0] == "P"]
    mrows = [x for x in rows if x[0] == "M"]
    for m in _messages():
        forms = {}
        while k < len(mrows) and int(mrows[k][1]) == len(m) and mrows[k][2] not in forms:
            forms[mrows[k][2]] = mrows[k][3]
            k += 1
        per_msg.append((m, forms))
    assert k == len(mrows)
    return p, per_msg


def test_digest_permutation_equals_the_full_one_on_lanes_0_to_3(out):
    p, _ = out
    assert p == [["P", "0"]]  # mismatches among N_STATES random states, every loop shape


def test_every_form_gives_the_same_digest(out, oracle):
    _, per_msg = out
    seen = set()
    for m, forms in per_msg:
        want = {"msg", "msg_digest"} | ({"short", "short_digest"} if len(m) <= 135 else set())
        want |= {"fixed"} if len(m) in (19, 20, 32, 135) else set()
        assert set(forms) == want, (len(m), sorted(forms))
        ref = oracle.kec256(m).hex()
        for f, d in forms.items():
            assert d == ref, (len(m), f, m.hex())
        seen.add(len(m))
    assert seen >= set(LENGTHS) | set(LONG)


def test_known_vectors(out):
    _, per_msg = out
    got = {m: forms for m, forms in per_msg if m in KNOWN}
    assert set(got) == set(KNOWN)
    for m, forms in got.items():
        assert forms["short_digest"] == forms["msg_digest"] == KNOWN[m]
