"""CPU: every kernel of the built library stands in exactly one of its code objects.

libkhst.so is seven compilation units (__graft_entry__.UNITS): khst.hip and leaf_kernel.hip hold
the hot kernels, whose code placement is measured (tests/test_code_layout.py), and five cold units
hold a service each, kernels and host driver.  The drivers reach the scans and the radix sort of
prims.h through plain wrappers of khst.hip (csrc/host.h): a driver that instantiated a kernel
template itself would emit the kernel a second time into its own code object, the runtime keeps
whichever copy registered first, and the hot build could then run a copy placed differently."""
import collections
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "khipu_amd", "libkhst.so")
sys.path.insert(0, os.path.join(ROOT, "scripts"))

# a kernel here is k_* in the global namespace (_Z<len>k_...; k_... where it has C linkage) or, the
# kernels of prims.h, in namespace khst (_ZN4khst<len>k_...)
KERNEL = re.compile(r"^(?:_Z(?:N4khst)?\d+)?k_")


def _code_objects():
    """[{function symbol, ...}, ...]: one set per code object of the library"""
    if not os.path.exists(LIB):
        pytest.skip("libkhst.so not built")
    import code_align as C
    try:
        txt = C.disassemble(LIB)
    except (OSError, Exception) as e:  # (objcopy / the ROCm LLVM tools absent)
        pytest.skip(f"disassembly unavailable: {e}")
    parts = re.split(r"(?m)^.*file format elf64-amdgpu.*$", txt)[1:]
    return [set(re.findall(r"(?m)^[0-9a-f]{16} <([\w.$]+)>:", p)) for p in parts]


def test_every_kernel_in_exactly_one_code_object():
    objs = _code_objects()
    assert len(objs) == 7, len(objs)
    seen = collections.Counter(s for o in objs for s in o if KERNEL.match(s))
    assert len(seen) >= 150, len(seen)  # (the disassembly was read: the parent of this test had 173)
    twice = sorted(s for s, k in seen.items() if k != 1)
    assert not twice, twice
    # each unit brings kernels of its own, and the templates of prims.h stay with khst.hip
    assert all(any(KERNEL.match(s) for s in o) for o in objs)
    prims = [k for k, o in enumerate(objs) if any(s.startswith("_ZN4khst") and KERNEL.match(s) for s in o)]
    assert prims == [0], prims
