"""CPU: the record -> node encoder of khipu_amd/csrc/export.h replayed on the host under
AddressSanitizer and UBSan.  tests/export_host/export_check.cc (a stand-alone program) builds a
trie's records bottom-up with the encoder itself, runs the sizes and write bodies over them into
buffers of exactly the scanned size, and prints the node set; it must equal the oracle's
reachable() -- every node with an encoding >= 32 B, plus the root."""
import random
import subprocess

import pytest

from tests import export_cases, hostprog


prog = hostprog.prog_fixture("export")


def _run(prog, tmp_path, keys, vals, *args):
    p = tmp_path / "in.txt"
    p.write_text("".join(f"{k.hex()} {v.hex() or '-'}\n" for k, v in zip(keys, vals)))
    r = subprocess.run([prog, str(p), *args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = r.stdout.split("\n")[:-1]
    assert lines[-1].startswith("verify_bad ")
    pairs = [tuple(bytes.fromhex(x) for x in ln.split()) for ln in lines[:-1]]
    return pairs, int(lines[-1].split()[1])


def _oracle_nodes(oracle, keys, vals):
    t = oracle.Trie()
    for k, v in zip(keys, vals):
        t.put(k, v)
    return t.reachable()


def _cases():
    r = random.Random(5)
    one = ([bytes(r.getrandbits(8) for _ in range(32))], [b"\x07" * 40])
    ks = [bytes(r.getrandbits(8) for _ in range(32)) for _ in range(300)]
    from tests import cases
    rnd = (ks, [cases.storage_value(r) if i % 3 else cases.account_value(r) for i, _ in enumerate(ks)])
    return {"one_key": one, "random300": rnd, "embedded": export_cases.embedded_case()}


@pytest.mark.parametrize("name", ["one_key", "random300", "embedded"])
def test_host_encoder_matches_oracle(prog, tmp_path, oracle, name):
    keys, vals = _cases()[name]
    want = _oracle_nodes(oracle, keys, vals)
    if name == "embedded":
        assert export_cases.holds_embedded_child(want)
    pairs, bad = _run(prog, tmp_path, keys, vals)
    assert bad == 0
    assert len(pairs) == len(want)  # no node twice
    assert dict(pairs) == want


def test_verify_counts_a_flipped_reference(prog, tmp_path):
    keys, vals = _cases()["random300"]
    _, bad = _run(prog, tmp_path, keys, vals, "flip")
    assert bad > 0
