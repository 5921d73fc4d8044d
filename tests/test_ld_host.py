"""Host-side checks of the windowed LD entry point (xsi_hip_decode_ld): the C prototype and window macro compile as
strict C99, the library exports the symbol and names the "ld" stage, argument errors come back before any device
work, and the new kernels use no scratch (no GPU needed)."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from xsqueezeit_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

C_SNIPPET = r"""
#include "xsi_hip.h"
int use_ld(xsi_hip_ctx* ctx, const void* f, uint64_t len, uint32_t* n11, float* r2);
int use_ld(xsi_hip_ctx* ctx, const void* f, uint64_t len, uint32_t* n11, float* r2) {
    uint64_t rows = 0;
    return xsi_hip_decode_ld(ctx, f, len, 0, 1, XSI_LD_MAX_WINDOW / 64u, n11, r2, 100, &rows);
}
"""


def test_ld_prototype_compiles_as_c99(tmp_path):
    gcc = shutil.which("gcc")
    if not gcc:
        pytest.skip("no gcc")
    src = tmp_path / "ld.c"
    src.write_text(C_SNIPPET)
    r = subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only",
                        "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_ld_symbol_and_stage():
    L = binding.lib()
    assert "xsi_hip_decode_ld" in binding.SYMBOLS
    assert hasattr(L, "xsi_hip_decode_ld")
    assert binding.LD_MAX_WINDOW == 65536
    names = [L.xsi_hip_stage_name(i).decode() for i in range(32)]
    assert "ld" in names
    # appended: the stages before it keep their indices
    assert names.index("ld") == names.index("score") + 1


def test_ld_argument_errors_without_device():
    """Null context / file, both outputs null, window 0 and window above the maximum are refused with XSI_ERR_ARG
    before the context is touched (a fake non-null context pointer would crash if it were dereferenced)."""
    L = binding.lib()
    buf = (ctypes.c_uint32 * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    fake = ctypes.c_void_p(8)  # never dereferenced: every case below fails its argument check first
    rows = ctypes.c_uint64(12345)
    cases = [
        (None, p, p, p, 4),                          # null context
        (fake, None, p, p, 4),                       # null file
        (fake, p, None, None, 4),                    # both outputs null
        (fake, p, p, None, 0),                       # window 0
        (fake, p, None, p, 0),
        (fake, p, p, p, binding.LD_MAX_WINDOW + 1),  # window above the maximum
        (fake, p, p, p, 0xFFFFFFFF),
    ]
    for ctx, f, n11, r2, window in cases:
        assert L.xsi_hip_decode_ld(ctx, f, 4096, 0, 1, window, n11, r2, 8, ctypes.byref(rows)) == binding.XSI_ERR_ARG
        assert b"decode_ld" in L.xsi_hip_last_error()
    assert rows.value == 12345  # nothing written on a refused call


def test_ld_kernels_use_no_scratch():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "xsi_ld.hip"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = [ln for ln in r.stdout.splitlines() if "k_ld_" in ln]
    assert len(lines) >= 2, r.stdout
    for ln in lines:
        assert "spill v0 s0" in ln and "scratch 0" in ln, ln


def test_ld_r2_formula_reference():
    """The numpy form of the header's r2 formula (what the GPU tests compare with) on hand-checked values."""
    from ld_ref import r2_ref
    N = 10
    n11 = np.array([[2, 0], [5, 3]], dtype=np.int64)
    ni = np.array([2, 5], dtype=np.int64)
    nj = np.array([[2, 0], [5, 10]], dtype=np.int64)
    r2 = r2_ref(N, n11, ni[:, None], nj)
    assert r2.dtype == np.float32
    assert r2[0, 0] == np.float32(1.0)   # identical lines
    assert np.isnan(r2[0, 1]) and np.isnan(r2[1, 1])  # monomorphic partner
    assert r2[1, 0] == np.float32(1.0)
