"""GPU: range responses verified against a root without a handle (kh_verify_ranges /
kh_dev_verify_ranges), held to tests/rangeverify_ref.py on the responses and tampers of
tests/rangeverify_cases.py, on pages a resident trie serves, on mixed proved / unproved calls, and
through the JNI shim."""
import ctypes
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

from tests import cases as C
from tests import proof_cases
from tests import proof_ref as P
from tests import range_cases as RC
from tests import range_ref as RR
from tests import rangeverify_cases as VC
from tests import rangeverify_ref as VR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCEN = C.commit_scenarios()


def _oracle(oracle, ks, vs):
    o = oracle.Trie()
    for k, v in zip(ks, vs):
        o.put(k, v)
    return o


def _nodes(o):
    return o.reachable() if o.root_hash() != P.EMPTY_ROOT else {}


def _ref(root, resp, proved=1):
    return VR.verify({P.kec(e): e for e in resp["nodes"]}, root, resp["origin"], resp["keys"], resp["vals"], proved)


def _dev(root, resps, proved=None):
    """The responses in ONE call over the union of their node lists."""
    from khipu_amd import verify_ranges
    enc = [e for x in resps for e in x["nodes"]]
    return verify_ranges([root] * len(resps), [x["origin"] for x in resps], [(x["keys"], x["vals"]) for x in resps], enc,
                         proved)


def _same(got, want, tag):
    """A device answer against the reference's: the status, `more` where it means something, the
    missing hash."""
    assert got[0] == want[0], (tag, got, want)
    if want[0] in (VR.OK, VR.INCOMPLETE):
        assert got[1] == want[1], (tag, got, want)
    assert got[2] == want[2], (tag, got, want)


@pytest.mark.parametrize("i", range(len(SCEN)), ids=[s[0] for s in SCEN])
def test_verify_after_commits(khst, oracle, i):
    from khipu_amd import verify_range, verify_ranges
    from khipu_amd.device import Ctx, ResidentTrie
    name, ks, vs, batches = SCEN[i]
    o = _oracle(oracle, ks, vs)
    trie = ResidentTrie(Ctx(0), ks, vs, emit=False)
    for b in range(len(batches) + 1):
        if b:
            for k, v in batches[b - 1][0]:
                o.put(k, v)
            for k in batches[b - 1][1]:
                o.remove(k)
            assert trie.commit(*batches[b - 1]) == o.root_hash(), (name, b)
        nodes, root = _nodes(o), o.root_hash()
        items = RR.content(nodes, root)
        r = VC.seed(i, b)
        resps = VC.responses(r, items, nodes, root)
        tam = [t for x in resps for t in VC.tampers(r, x, items, nodes, root)]
        # the state's 40 responses in one call (one shared node set); five of them again singly
        got = _dev(root, resps)
        for x, g in zip(resps, got):
            assert g == (VR.OK, x["more"], None), (name, b, x["origin"].hex(), g)
        for x, g in list(zip(resps, got))[::8]:
            assert verify_range(root, x["origin"], x["keys"], x["vals"], x["nodes"]) == g
        # the same responses served by the resident trie of this state (range_proof), verified singly
        # and in one call over the union of their proof tables
        served = [trie.range_proof(x["origin"], None, x["max"]) for x in resps]
        for x, (keys, vals, more, _, table) in zip(resps, served):
            assert (keys, vals, more) == (x["keys"], x["vals"], x["more"]), (name, b, x["origin"].hex())
            assert verify_range(root, x["origin"], keys, vals, table) == (VR.OK, more, None), (name, b, x["origin"].hex())
        assert verify_ranges([root] * len(resps), [x["origin"] for x in resps], [(s[0], s[1]) for s in served],
                             [e for s in served for e in s[4].nodes]) == [(VR.OK, s[2], None) for s in served]
        # every tamper against the reference (each with its own nodes there).  On the device the ones
        # that withhold a node go singly -- the node must not come back through a neighbour -- and
        # the others in one call: their walks read their own boundary paths only
        wants = [_ref(root, t, proved) for _, t, proved, _ in tam]
        assert [w[0] for w in wants] == [exp[0] for _, _, _, exp in tam]
        rest = [j for j, t in enumerate(tam) if not t[0].startswith("withhold")]
        got = dict(zip(rest, _dev(root, [tam[j][1] for j in rest], [tam[j][2] for j in rest]))) if rest else {}
        for j, (kind, t, proved, _) in enumerate(tam):
            g = got[j] if j in got else verify_range(root, t["origin"], t["keys"], t["vals"], t["nodes"])
            _same(g, wants[j], (name, b, kind))
        # the whole content unproved, and minus one entry
        kk, vv = [k for k, _ in items], [v for _, v in items]
        assert verify_range(root, None, kk, vv, None) == (VR.OK, False, None)
        if items:
            j = r.randrange(len(items))
            assert verify_range(root, None, kk[:j] + kk[j + 1:], vv[:j] + vv[j + 1:], None)[0] == VR.BAD_ROOT
    trie.close()


@pytest.mark.parametrize("hashed", [False, True], ids=["raw", "hashed"])
def test_verify_what_a_resident_trie_serves(khst, oracle, hashed):
    """The serve / verify pair: ResidentTrie.range_proof's page and table verify OK with the page's
    `more`; on a hash_keys handle the keys are the kec256 values and are not hashed again."""
    from khipu_amd import verify_range, verify_ranges
    from khipu_amd.device import Ctx, ResidentTrie
    r = random.Random(71)
    raw = [bytes(r.getrandbits(8) for _ in range(20 if hashed else 32)) for _ in range(300)]
    vs = [C.account_value(r) if j % 3 else C.storage_value(r) for j in range(len(raw))]
    tk = sorted(oracle.kec256(k) for k in raw) if hashed else sorted(raw)
    t = ResidentTrie(Ctx(0), raw, vs, hash_keys=hashed, emit=False)
    root = t.root_hash
    pages = []
    for _ in range(40):
        origin = RC._point(r, tk) if r.random() < 0.85 else None
        keys, vals, more, nxt, table = t.range_proof(origin, None, r.choice(RC.MAXES))
        assert verify_range(root, origin, keys, vals, table) == (VR.OK, more, None)
        pages.append((origin, keys, vals, more, table))
    got = verify_ranges([root] * 40, [p[0] for p in pages], [(p[1], p[2]) for p in pages],
                        [e for p in pages for e in p[4].nodes])
    assert got == [(VR.OK, p[3], None) for p in pages]
    assert sum(1 for p in pages if p[1] and p[3]) >= 8
    t.close()


def test_mixed_call_of_whole_tries_and_a_proved_tail(khst, oracle):
    """A storage-ranges response: 60 unproved whole tries of 1-300 slots and one proved tail in one
    call; one of the 60 has a changed value, and its status alone is BAD_ROOT."""
    from khipu_amd import verify_ranges
    r = random.Random(81)
    sizes = [1, 2, 3, 300] + [r.choice([1, 5, 17, 60, 300]) for _ in range(56)]
    roots, resp = [], []
    for n in sizes:
        ks = sorted(C._rk(r) for _ in range(n))
        vs = [C.storage_value(r) for _ in ks]
        roots.append(_oracle(oracle, ks, vs).root_hash())
        resp.append((ks, vs))
    ks = sorted(C._rk(r) for _ in range(200))
    vs = [C.storage_value(r) for _ in ks]
    o = _oracle(oracle, ks, vs)
    tail = VC.response(list(zip(ks, vs)), o.reachable(), o.root_hash(), RC.ZERO, 50)
    bad = 37
    v = bytearray(resp[bad][1][0])
    v[-1] ^= 1
    resp[bad] = (resp[bad][0], [bytes(v)] + resp[bad][1][1:])
    got = verify_ranges(roots + [o.root_hash()], None, resp + [(tail["keys"], tail["vals"])], tail["nodes"],
                        [0] * 60 + [1])
    assert len(sizes) == 60 and got[60] == (VR.OK, True, None)
    assert [g[0] for g in got[:60]] == [VR.BAD_ROOT if j == bad else VR.OK for j in range(60)]
    assert all(g[1:] == (False, None) for g in got[:60])


def test_empty_tries_and_the_value_only_branch_limit(khst, oracle):
    from khipu_amd import verify_range, verify_ranges
    E = P.EMPTY_ROOT
    assert verify_range(E, None, [], [], []) == (VR.OK, False, None)
    assert verify_range(E, None, [], [], None) == (VR.OK, False, None)
    assert verify_range(E, b"\x55" * 32, [], [], []) == (VR.OK, False, None)
    assert verify_range(E, None, [b"\x01" * 32], [b"v"], [])[0] == VR.BAD_ROOT
    assert verify_range(E, None, [b"\x01" * 32], [b"v"], None)[0] == VR.BAD_ROOT
    assert verify_range(b"\x07" * 32, None, [], [], []) == (VR.MISSING, False, b"\x07" * 32)
    assert verify_range(b"\x07" * 32, None, [], [], None)[0] == VR.BAD_ROOT
    assert verify_ranges([], None, [], []) == []
    # khipu's value-only branch inside a range: BAD_ROOT; a range that ends below it: OK
    ks, vs, blocks, (k1, k2, k3) = proof_cases.vb_case(False)
    o = _oracle(oracle, ks, vs)
    for k, v in blocks[0][0]:
        o.put(k, v)
    nodes, root = o.reachable(), o.root_hash()
    items = RR.content(nodes, root)
    at = [k for k, _ in items].index(min(k1, ks[-2]))  # (blocks[0] re-puts k1 and q1 = ks[-2])
    around = VC.response(items, nodes, root, items[at - 2][0], 5)
    below = VC.response(items, nodes, root, RC.ZERO, at - 1)
    upto = VC.response(items, nodes, root, RC.ZERO, at + 1)
    got = [verify_range(root, x["origin"], x["keys"], x["vals"], x["nodes"]) for x in (around, below, upto)]
    assert [g[0] for g in got] == [VR.BAD_ROOT, VR.OK, VR.BAD_ROOT] and got[1] == (VR.OK, True, None)
    assert [g[0] for g in got] == [_ref(root, x)[0] for x in (around, below, upto)]
    # no entries: INCOMPLETE while keys lie above origin; malformed nodes as the root: BAD_NODE
    none = dict(VC.response(items, nodes, root, items[5][0], 3), keys=[], vals=[])
    assert verify_range(root, none["origin"], [], [], none["nodes"]) == (VR.INCOMPLETE, True, None)
    key = b"\x11" * 32
    for name, enc in proof_cases.malformed_nodes():
        for keys, vals in (([], []), ([key], [b"v"])):
            g = verify_range(P.kec(enc), key, keys, vals, [enc])
            assert g == (VR.BAD_NODE, False, None), (name, g)
            assert VR.verify({P.kec(enc): enc}, P.kec(enc), key, keys, vals)[0] == VR.BAD_NODE, name


def _case(oracle, seed=91):
    r = random.Random(seed)
    ks = sorted(C._rk(r) for _ in range(300))
    vs = [C.account_value(r) if j % 3 else C.storage_value(r) for j in range(len(ks))]
    o = _oracle(oracle, ks, vs)
    items = list(zip(ks, vs))
    resps = VC.responses(r, items, o.reachable(), o.root_hash(), 12)
    return r, items, o, resps


def test_device_buffers_against_the_host_form(khst, oracle):
    """kh_dev_verify_ranges with every array in HBM, honest and tampered ranges mixed."""
    import torch
    from khipu_amd import _lib, verify_ranges
    from khipu_amd.device import Ctx, _range_arrays
    r, items, o, resps = _case(oracle)
    root = o.root_hash()
    tam = [t for x in resps[:4] for t in VC.tampers(r, x, items, o.reachable(), root) if t[2]]
    allr = resps + [t[1] for t in tam if not t[0].startswith("withhold")]
    enc = [e for x in allr for e in x["nodes"]]
    args = ([root] * len(allr), [x["origin"] for x in allr], [(x["keys"], x["vals"]) for x in allr], enc, None)
    want = verify_ranges(*args)
    assert {w[0] for w in want} >= {VR.OK, VR.BAD_ORDER, VR.BAD_ROOT}
    nr, nn, a = _range_arrays(*args)
    ctx = Ctx(0)
    dev = {k: (torch.from_numpy(v.view(np.int64) if v.dtype == np.uint64 else v).to("cuda:0")) for k, v in a.items()}
    status, more, miss = np.zeros(nr, np.uint8), np.zeros(nr, np.uint8), np.zeros(32 * nr, np.uint8)
    ctx._sync()
    for c in (ctx.h, None):
        status[:] = 9
        rc = _lib.lib().kh_dev_verify_ranges(c, *[ctypes.c_void_p(dev[k].data_ptr()) for k in ("roots", "origins", "proved")],
                                             nr, *[ctypes.c_void_p(dev[k].data_ptr()) for k in
                                                   ("keys", "vals", "voff", "ent_off", "enc", "off")],
                                             nn, status.ctypes.data, more.ctypes.data, miss.ctypes.data)
        assert rc == _lib.KH_OK, _lib.lib().kh_last_error()
        got = [(int(status[s]), bool(more[s]), miss[32 * s:32 * s + 32].tobytes() if status[s] == VR.MISSING else None)
               for s in range(nr)]
        assert got == want
    # the keys are read as 64-bit words: a pointer off by four bytes is refused, nothing written
    status[:] = 9
    ptr = {k: dev[k].data_ptr() + (4 if k == "keys" else 0) for k in dev}
    rc = _lib.lib().kh_dev_verify_ranges(ctx.h, *[ctypes.c_void_p(ptr[k]) for k in ("roots", "origins", "proved")], nr,
                                         *[ctypes.c_void_p(ptr[k]) for k in
                                           ("keys", "vals", "voff", "ent_off", "enc", "off")],
                                         nn, status.ctypes.data, more.ctypes.data, miss.ctypes.data)
    assert rc == _lib.KH_EINVAL and (status == 9).all()
    ctx.close()


def test_argument_errors_write_nothing(khst, oracle):
    from khipu_amd import _lib
    from khipu_amd.device import _range_arrays
    _, items, o, resps = _case(oracle, 92)
    x = resps[0]
    nr, nn, a = _range_arrays([o.root_hash()] * 2, [x["origin"]] * 2, [(x["keys"], x["vals"])] * 2, x["nodes"], None)
    L = _lib.lib()

    def call(**kw):
        b = dict(a)
        b.update(kw)
        status, more, miss = np.full(nr, 9, np.uint8), np.full(nr, 9, np.uint8), np.full(32 * nr, 9, np.uint8)
        p = {k: (v.ctypes.data if v is not None else None) for k, v in b.items() if k not in ("nr", "nn", "status")}
        rc = L.kh_verify_ranges(p["roots"], p["origins"], p["proved"], b.get("nr", nr), p["keys"], p["vals"], p["voff"],
                                p["ent_off"], p["enc"], p["off"], b.get("nn", nn),
                                None if b.get("status", 1) is None else status.ctypes.data, more.ctypes.data,
                                miss.ctypes.data)
        assert (status == 9).all() and (more == 9).all() and (miss == 9).all() or rc == _lib.KH_OK
        return rc
    assert call() == _lib.KH_OK
    assert call(origins=None) == _lib.KH_OK
    for k in ("roots", "proved", "keys", "voff", "ent_off", "enc", "off"):
        assert call(**{k: None}) == _lib.KH_EINVAL, k
    assert call(status=None) == _lib.KH_EINVAL
    for k in ("voff", "ent_off", "off"):
        v = a[k].copy()
        v[1], v[2] = v[2] + 1, v[1]
        assert call(**{k: v}) == _lib.KH_EINVAL, k
    assert call(nr=1 << 31) == _lib.KH_EINVAL and call(nn=1 << 31) == _lib.KH_EINVAL
    big = a["ent_off"].copy()
    big[2] = 1 << 31
    assert call(ent_off=big) == _lib.KH_EINVAL


def test_verify_through_the_jni_shim(khst, oracle, tmp_path):
    """verifyRanges through the in-process JNIEnv of tests/jni_stub: honest, tampered and unproved
    ranges in one call, the statuses, `more` and missing hashes printed back."""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    from khipu_amd.device import _range_arrays
    stub = os.path.join(ROOT, "tests", "jni_stub")
    exe = tmp_path / "jni_rangeverify_driver"
    rc = subprocess.run([cc, "-std=gnu99", "-O1", "-Wall", "-Werror", "-I", stub, "-I", os.path.join(ROOT, "include"),
                         "-o", str(exe), os.path.join(stub, "jni_rangeverify_driver.c"), os.path.join(stub, "fake_env.c"),
                         os.path.join(ROOT, "jni", "khst_jni.c"), "-L", os.path.join(ROOT, "khipu_amd"), "-lkhst",
                         "-Wl,-rpath," + os.path.join(ROOT, "khipu_amd"), "-Wl,-rpath-link,/opt/rocm/lib"],
                        capture_output=True, text=True)
    assert rc.returncode == 0, rc.stderr
    r, items, o, resps = _case(oracle, 93)
    root = o.root_hash()
    tam = [t for x in resps[:3] for t in VC.tampers(r, x, items, o.reachable(), root)]
    allr = [(x, 1) for x in resps] + [(t[1], t[2]) for t in tam if not t[0].startswith("withhold")]
    gone = [t for t in tam if t[0].startswith("withhold")][0]
    want = [_ref(root, x, p) for x, p in allr]
    nr, nn, a = _range_arrays([root] * len(allr), [x["origin"] for x, _ in allr], [(x["keys"], x["vals"]) for x, _ in allr],
                              [e for x, _ in allr for e in x["nodes"]], [p for _, p in allr])
    p = tmp_path / "in.bin"

    def dump(path, nr, nn, a):
        with open(path, "wb") as f:
            ne, vb, nb = int(a["ent_off"][nr]), int(a["voff"][-1]), int(a["off"][nn])
            f.write(np.asarray([nr, ne, vb, nn, nb], np.uint64).tobytes())
            f.write(a["roots"][:32 * nr].tobytes() + a["origins"][:32 * nr].tobytes() + a["proved"][:nr].tobytes())
            f.write(a["keys"][:32 * ne].tobytes() + a["vals"][:vb].tobytes() + a["voff"].tobytes())
            f.write(a["ent_off"].tobytes() + a["enc"][:nb].tobytes() + a["off"].tobytes())
    dump(p, nr, nn, a)
    x = gone[1]
    p2 = tmp_path / "in2.bin"
    dump(p2, *_range_arrays([root], [x["origin"]], [(x["keys"], x["vals"])], x["nodes"], None))
    for path, exp in ((p, want), (p2, [_ref(root, x)])):
        rc = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=120)
        assert rc.returncode == 0, rc.stderr
        lines = [ln.split() for ln in rc.stdout.split("\n")[:-1]]
        assert [ln for ln in lines if ln[0] == "E"] == [["E", "0"]], lines
        # null or empty offset arrays: an exception before anything is read; one-offset arrays: none
        iae = "java/lang/IllegalArgumentException"
        assert lines[-5:] == [["X", str(c), "1", iae] for c in range(4)] + [["X", "4", "0"]], lines[-5:]
        got = [(int(ln[2]), ln[3] == "1", bytes.fromhex(ln[4]) if int(ln[2]) == VR.MISSING else None)
               for ln in lines if ln[0] == "R"]
        assert len(got) == len(exp)
        for g, w in zip(got, exp):
            _same(g, w, path.name)
    assert exp[0][0] == VR.MISSING and {w[0] for w in want} >= {VR.OK, VR.BAD_ORDER, VR.BAD_ROOT}
