"""What the host replay tests (tests/test_*_host.py) share: the build of a stand-alone program
under AddressSanitizer and UBSan, the hex form of the programs' input files, oracle tries and
hand-made RLP."""
import os
import shutil
import subprocess

import pytest

from tests import proof_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARN = ["-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas"]
SANITIZE = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def compile_prog(src, exe, flags=SANITIZE):
    """The stand-alone program `src` compiled to `exe` (run as a child process, never loaded)."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    r = subprocess.run([cxx] + flags + WARN + ["-o", str(exe), src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def prog_fixture(name):
    """A module's `prog` fixture: tests/<name>_host/<name>_check.cc, built once with the sanitizers."""
    @pytest.fixture(scope="module")
    def prog(tmp_path_factory):
        src = os.path.join(ROOT, "tests", f"{name}_host", f"{name}_check.cc")
        return compile_prog(src, tmp_path_factory.mktemp(f"{name}_host") / f"{name}_check")
    return prog


def hexs(b):
    return b.hex() or "-"


def unhexs(s):
    return b"" if s == "-" else bytes.fromhex(s)


def trie(oracle, keys, vals):
    o = oracle.Trie()
    for k, v in zip(keys, vals):
        o.put(k, v)
    return o


def vb_trie(oracle):
    """khipu's value-only branch: a re-put of a key whose leaf hangs under a depth-63 branch.
    -> (trie, the number of its keys)"""
    ks, vs, blocks, _ = proof_cases.vb_case(False)
    o = trie(oracle, ks, vs)
    for ups, dels in blocks[:1]:
        for k, v in ups:
            o.put(k, v)
        for k in dels:
            o.remove(k)
    live = {k: o.get(k) for k in ks}
    return o, sum(1 for v in live.values() if v is not None)


def rlp_str(b):
    return bytes([0x80 + len(b)]) + b if len(b) != 1 or b[0] >= 0x80 else b


def rlp_list(items):
    p = b"".join(items)
    return (bytes([0xC0 + len(p)]) if len(p) < 56 else bytes([0xF8, len(p)]) if len(p) < 256
            else bytes([0xF9, len(p) >> 8, len(p) & 255])) + p
