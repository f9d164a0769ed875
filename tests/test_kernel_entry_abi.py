"""CPU-side check of the per-kernel test entries: libsdp.so exports every sdpk_* that include/sdp_kernels.h declares,
the test binding covers them all, and the stable boundary (include/sdp.h, prefix sdp_) holds no sdpk_ entry."""
import os
import re
import subprocess

from conftest import PKG_DIR, REPO

import kernel_lib as KL
import test_lib_abi as ABI

HEADER = os.path.join(REPO, "include", "sdp_kernels.h")
LIB = os.path.join(PKG_DIR, "sdp", "_lib", "libsdp.so")


def declared():
    src = open(HEADER).read()
    return sorted(set(re.findall(r"^\s*(?:int|size_t)\s+(sdpk_\w+)\s*\(", src, re.M)))


def test_library_exports_every_declared_kernel_entry():
    d = declared()
    assert len(d) == 23, d
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (sdpk_\w+)", out))
    assert exported == set(d), (sorted(exported - set(d)), sorted(set(d) - exported))
    assert set(KL.SIGS) == set(d)


def test_stable_boundary_is_unchanged():
    from sdp import _lib
    assert not [s for s in ABI.declared() if s.startswith("sdpk")]
    assert set(_lib.exported_symbols()) == set(ABI.declared())
    assert not [s for s in _lib.exported_symbols() if s.startswith("sdpk")]
    assert "sdpk_" not in open(os.path.join(REPO, "include", "sdp.h")).read()
