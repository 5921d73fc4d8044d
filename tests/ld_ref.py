"""numpy reference of xsi_hip_decode_ld: the haplotype carrier matrix of oracle-decoded rows, its band of pair counts
and the header's r2 formula, step for step, so the GPU output can be compared with `==`."""
import numpy as np

SENTINEL = 0xFFFFFFFF


def carrier_matrix(dec, n_samples):
    """[n_lines x N] uint8 ALT carriers of bi-allelic oracle-decoded rows; a fully haploid line's sample s at
    haplotype 2s."""
    N = 2 * n_samples
    X = np.zeros((len(dec), N), dtype=np.uint8)
    for r, (g, _) in enumerate(dec):
        hit = ((g.astype(np.int64) >> 1) - 1) == 1
        if len(g) == n_samples:
            X[r, 0::2] = hit
        else:
            X[r, :] = hit
    return X


def r2_ref(N, n11, ni, nj):
    """The header's formula in its order: every step one correctly rounded float64 operation, then float32."""
    n11, ni, nj = (np.asarray(a, dtype=np.int64) for a in (n11, ni, nj))
    num = (np.int64(N) * n11 - ni * nj).astype(np.float64)
    den = (ni * (np.int64(N) - ni)).astype(np.float64) * (nj * (np.int64(N) - nj)).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r2 = (num * num / den).astype(np.float32)
    return np.where(den == 0.0, np.float32(np.nan), r2).astype(np.float32)


def band(X, rows, window):
    """(n11 [len(rows) x window] uint32, r2 float32) for rows `rows` of X against lines r + 1 .. r + window; partners past
    X's last line get the sentinel / NaN."""
    X64 = X.astype(np.int64)
    n_lines, N = X.shape
    cnt = X64.sum(1)
    rows = np.asarray(rows, dtype=np.int64)
    n11 = np.full((len(rows), window), SENTINEL, dtype=np.uint32)
    r2 = np.full((len(rows), window), np.nan, dtype=np.float32)
    for i, r in enumerate(rows):
        p = np.arange(r + 1, min(r + 1 + window, n_lines))
        if len(p) == 0:
            continue
        c = X64[p] @ X64[r]
        n11[i, :len(p)] = c
        r2[i, :len(p)] = r2_ref(N, c, cnt[r], cnt[p])
    return n11, r2


def same_r2(a, b):
    """Bit-identical float32 arrays, NaN where the other is NaN."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))
