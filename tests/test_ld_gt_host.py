"""Host-side checks of the general windowed LD entry point (xsi_hip_decode_ld_gt): the C prototype compiles as strict
C99, the library exports the symbol, argument errors come back before any device work, and the numpy reference the GPU
tests compare with gives hand-checked pairwise-complete counts (no GPU needed)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from xsqueezeit_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

C_SNIPPET = r"""
#include "xsi_hip.h"
int use_ld_gt(xsi_hip_ctx* ctx, const void* f, uint64_t len, const uint32_t* nal, uint32_t* n11, float* r2, uint32_t* nc);
int use_ld_gt(xsi_hip_ctx* ctx, const void* f, uint64_t len, const uint32_t* nal, uint32_t* n11, float* r2, uint32_t* nc) {
    uint64_t rows = 0;
    return xsi_hip_decode_ld_gt(ctx, f, len, 0, 1, nal, 10, XSI_LD_MAX_WINDOW / 64u, n11, r2, nc, 100, &rows);
}
"""


def test_ld_gt_prototype_compiles_as_c99(tmp_path):
    gcc = shutil.which("gcc")
    if not gcc:
        pytest.skip("no gcc")
    src = tmp_path / "ld_gt.c"
    src.write_text(C_SNIPPET)
    r = subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only",
                        "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_ld_gt_symbol():
    L = binding.lib()
    assert "xsi_hip_decode_ld_gt" in binding.SYMBOLS
    assert hasattr(L, "xsi_hip_decode_ld_gt")


def test_ld_gt_argument_errors_without_device():
    """Null context / file / allele numbers, all three outputs null, window 0 and window above the maximum are refused
    with XSI_ERR_ARG before the context is touched (a fake non-null context pointer would crash if dereferenced)."""
    L = binding.lib()
    buf = (ctypes.c_uint32 * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    nal = (ctypes.c_uint32 * 4)(2, 2, 2, 2)
    fake = ctypes.c_void_p(8)
    rows = ctypes.c_uint64(12345)
    cases = [
        (None, p, nal, p, p, p, 4),                          # null context
        (fake, None, nal, p, p, p, 4),                       # null file
        (fake, p, None, p, p, p, 4),                         # null allele numbers
        (fake, p, nal, None, None, None, 4),                 # all outputs null
        (fake, p, nal, p, None, None, 0),                    # window 0
        (fake, p, nal, None, None, p, 0),
        (fake, p, nal, p, p, p, binding.LD_MAX_WINDOW + 1),  # window above the maximum
        (fake, p, nal, None, p, None, 0xFFFFFFFF),
    ]
    for ctx, f, al, n11, r2, nc, window in cases:
        assert L.xsi_hip_decode_ld_gt(ctx, f, 4096, 0, 1, al, 4, window, n11, r2, nc, 8,
                                      ctypes.byref(rows)) == binding.XSI_ERR_ARG
        assert b"decode_ld_gt" in L.xsi_hip_last_error()
    assert rows.value == 12345  # nothing written on a refused call


def _g(alleles, phased=False):
    """htslib int32 values of allele indices (-1 missing, None end-of-vector)."""
    out = []
    for a in alleles:
        out.append(-(2 ** 31) + 1 if a is None else ((a + 1) << 1) | int(phased))
    return np.array(out, dtype=np.int32)


def test_ld_gt_reference_hand_checked():
    from ld_gt_ref import band_gt, gt_matrices
    from ld_ref import SENTINEL
    n = 3   # 6 haplotypes
    dec = [
        (_g([1, 0, 1, -1, 0, 0]), None),        # line 0: haplotype 3 missing
        (_g([1, 0, 0, 1, 1, 0]), None),         # line 1: fully called
        (_g([1, -1, 0]), None),                 # line 2: fully haploid, sample 1 missing (haplotypes 2, 3)
        (_g([-1, -1, -1, -1, None, None]), None),  # line 3: nothing called
        (_g([2, 1, 0, 2, 1, 0]), None),         # line 4: tri-allelic -> binary lines 4 (ALT 1), 5 (ALT 2)
    ]
    nal = [2, 2, 2, 2, 3]
    X, C = gt_matrices(dec, nal, n)
    assert X.shape == (6, 6)
    assert list(C[2]) == [1, 1, 0, 0, 1, 1] and list(X[2]) == [1, 0, 0, 0, 0, 0]
    assert list(X[4]) == [0, 1, 0, 0, 1, 0] and list(X[5]) == [1, 0, 0, 1, 0, 0] and C[4].all() and C[5].all()
    n11, r2, nc = band_gt(X, C, range(6), 2)
    # (0, 1): called on both = haplotypes {0, 1, 2, 4, 5}; X0 = {0, 2}, X1 = {0, 3, 4} -> a = |X0 & C1| = 2, b = |C0 & X1|
    # = {0, 4} = 2, n11 = 1; r2 = (5*1 - 2*2)^2 / (2*3 * 2*3) = 1/36
    assert nc[0, 0] == 5 and n11[0, 0] == 1
    assert r2[0, 0] == np.float32(1.0 / 36.0)
    # (1, 2): the haploid line's called set {0, 1, 4, 5}; X1 & C2 = {0, 4}, C1 & X2 = {0}, n11 = 1
    # r2 = (4*1 - 2*1)^2 / (2*2 * 1*3) = 4/12
    assert nc[1, 0] == 4 and n11[1, 0] == 1
    assert r2[1, 0] == np.float32(4.0 / 12.0)
    # (0, 2): called on both = {0, 1, 4, 5}; a = |X0 & C2| = 1, b = |C0 & X2| = 1, n11 = 1 -> r2 = (4 - 1)^2 / (3 * 3) = 1
    assert nc[0, 1] == 4 and n11[0, 1] == 1 and r2[0, 1] == np.float32(1.0)
    # every pair with line 3: nothing called on both -> n_called 0, n11 0, r2 NaN
    assert nc[2, 0] == 0 and n11[2, 0] == 0 and np.isnan(r2[2, 0])
    assert nc[3, 0] == 0 and nc[3, 1] == 0 and np.isnan(r2[3]).all() and (n11[3] == 0).all()
    # two ALT alleles of one record: both fully called, disjoint carriers -> n11 = 0, r2 = (6*0 - 2*2)^2 / (2*4 * 2*4)
    assert nc[4, 0] == 6 and n11[4, 0] == 0 and r2[4, 0] == np.float32(16.0 / 64.0)
    # past the last line: sentinels
    assert n11[5, 0] == SENTINEL and nc[5, 1] == SENTINEL and np.isnan(r2[5]).all()
