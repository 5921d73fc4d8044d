"""numpy reference of xsi_hip_decode_ld_gt: carrier and called matrices of oracle-decoded rows, the four pairwise-complete
counts of every pair in the band and the header's r2 formula with N -> n_called, n_i -> a, n_j -> b, step for step, so
the GPU output can be compared with `==`."""
import numpy as np

from ld_ref import SENTINEL


def gt_matrices(dec, nal, n_samples):
    """(X, C): [n_bin x N] uint8 carriers and called haplotypes, binary lines in file order (ALT 1 .. n_allele - 1 of each
    BCF line).  A fully haploid line's sample s is haplotype 2s; 2s + 1 carries nothing and has the call status of 2s."""
    N = 2 * n_samples
    xs, cs = [], []
    for (g, _), na in zip(dec, nal):
        al = (np.asarray(g).astype(np.int64) >> 1) - 1   # missing: -1, end-of-vector: far below
        called = al >= 0
        for k in range(1, na):
            x = np.zeros(N, dtype=np.uint8)
            c = np.zeros(N, dtype=np.uint8)
            if len(g) == n_samples:
                x[0::2] = al == k
                c[0::2] = called
                c[1::2] = called
            else:
                x[:] = al == k
                c[:] = called
            xs.append(x)
            cs.append(c)
    return np.stack(xs), np.stack(cs)


def r2_pairwise(nc, n11, a, b):
    """decode_ld's formula with N -> n_called, n_i -> a, n_j -> b; every step one correctly rounded float64 operation,
    then float32; NaN where den == 0."""
    nc, n11, a, b = (np.asarray(v, dtype=np.int64) for v in (nc, n11, a, b))
    num = (nc * n11 - a * b).astype(np.float64)
    den = (a * (nc - a)).astype(np.float64) * (b * (nc - b)).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r2 = (num * num / den).astype(np.float32)
    return np.where(den == 0.0, np.float32(np.nan), r2).astype(np.float32)


def band_gt(X, C, rows, window):
    """(n11, r2, n_called), each [len(rows) x window], for rows `rows` against lines r + 1 .. r + window; partners past the
    last line get the sentinel (n11, n_called) and NaN (r2)."""
    X64, C64 = X.astype(np.int64), C.astype(np.int64)
    n_lines = X.shape[0]
    rows = np.asarray(rows, dtype=np.int64)
    n11 = np.full((len(rows), window), SENTINEL, dtype=np.uint32)
    ncl = np.full((len(rows), window), SENTINEL, dtype=np.uint32)
    r2 = np.full((len(rows), window), np.nan, dtype=np.float32)
    for i, r in enumerate(rows):
        p = np.arange(r + 1, min(r + 1 + window, n_lines))
        if len(p) == 0:
            continue
        m = len(p)
        c11 = X64[p] @ X64[r]
        a = C64[p] @ X64[r]     # |X_i & C_j|
        b = X64[p] @ C64[r]     # |C_i & X_j|
        nc = C64[p] @ C64[r]
        n11[i, :m] = c11
        ncl[i, :m] = nc
        r2[i, :m] = r2_pairwise(nc, c11, a, b)
    return n11, r2, ncl
