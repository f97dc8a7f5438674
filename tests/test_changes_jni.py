"""CPU: the JNI wrapper of kh_trie_changes_since_host (jni/khst_jni.c changesSince) through the
in-process JNIEnv of tests/jni_stub: it compiles and links with the rest of the shim, its own
argument checks raise IllegalArgumentException before any library call, and the library's KH_EINVAL
becomes MPTException.  A resident handle needs a device, so the answers themselves are
tests/test_gpu_changes.py's."""
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "khipu_amd", "libkhst.so")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not os.path.exists(LIB):
        pytest.skip("libkhst.so not built (__graft_entry__.build())")
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    stub = os.path.join(ROOT, "tests", "jni_stub")
    exe = tmp_path_factory.mktemp("jni_changes") / "jni_changes_driver"
    rc = subprocess.run([cc, "-std=gnu99", "-O1", "-Wall", "-Werror", "-I", stub, "-I", os.path.join(ROOT, "include"),
                         "-o", str(exe), os.path.join(stub, "jni_changes_driver.c"), os.path.join(stub, "fake_env.c"),
                         os.path.join(ROOT, "jni", "khst_jni.c"), "-L", os.path.join(ROOT, "khipu_amd"), "-lkhst",
                         "-Wl,-rpath," + os.path.join(ROOT, "khipu_amd"), "-Wl,-rpath-link,/opt/rocm/lib"],
                        capture_output=True, text=True)
    assert rc.returncode == 0, rc.stderr
    return str(exe)


def test_wrapper_refusals_through_a_jnienv(driver):
    r = subprocess.run([driver], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    got = {d["check"]: d for d in map(json.loads, r.stdout.split("\n")[:-1])}
    for c in ("next_short", "sizes_short", "from_short", "no_room", "tries_bound"):
        assert got[c]["pending"] == 1 and got[c]["exc"] == "java/lang/IllegalArgumentException" and got[c]["ret"] == 0, got[c]
    assert got["null_handle"]["pending"] == 1 and got["null_handle"]["ret"] == 0
    assert got["null_handle"]["exc"] == "khipu/trie/MerklePatriciaTrie$MPTException", got["null_handle"]


def test_wrapper_is_modelled_on_diff():
    """Region copies through Bufs, the -1 return for KH_ENOSPC, five size words."""
    with open(os.path.join(ROOT, "jni", "khst_jni.c")) as f:
        shim = f.read()
    body = shim[shim.index("Java_khipu_trie_gpu_Khst_changesSince("):]
    body = body[:body.index("\n}\n")]
    assert "kh_trie_changes_since_host(" in body and "KH_CHANGES_REVERSE" in body
    assert "bufs_free(&b)" in body and "if (rc == KH_ENOSPC) return -1;" in body
    assert re.search(r"put_l\(env, sizes, sz, 5\)", body)
