"""GPU tests of the general windowed LD (xsi_hip_decode_ld_gt): pairwise-complete n11, n_called and r2 on blocks with
multi-allelic lines, missing and end-of-vector values and fully haploid lines, compared with `==` (r2 bit for bit)
against numpy on the oracle-decoded rows, and bit identity with xsi_hip_decode_ld where both entry points apply."""
import ctypes

import numpy as np
import pytest

from xsqueezeit_amd import binding
from ld_gt_ref import band_gt, gt_matrices
from ld_ref import SENTINEL, same_r2
from test_oracle import _random_lines

pytestmark = pytest.mark.gpu

GUARD = 0x7A7A7A7A


class LDG:
    def __init__(self, ref, nal):
        import gpu_util as G
        self.G, self.torch, self.L = G, G.torch_mod(), binding.lib()
        self.ref, self.nal = ref, np.asarray(nal, dtype=np.uint32)
        self.d_file = G.dev_u8(np.frombuffer(ref, dtype=np.uint8))

    def call(self, first, n_blocks, window, cap, nal=None, outs=(True, True, True), file_len=None):
        torch = self.torch
        nal = np.ascontiguousarray(self.nal if nal is None else nal, dtype=np.uint32)
        o1 = torch.full((cap * window + 7,), GUARD, dtype=torch.int32, device="cuda") if outs[0] else None
        o2 = torch.full((cap * window + 7,), -1.0, dtype=torch.float32, device="cuda") if outs[1] else None
        o3 = torch.full((cap * window + 7,), GUARD, dtype=torch.int32, device="cuda") if outs[2] else None
        rows = ctypes.c_uint64(0)
        rc = self.L.xsi_hip_decode_ld_gt(self.G.ctx().handle, self.d_file.data_ptr(),
                                         len(self.ref) if file_len is None else file_len, first, n_blocks,
                                         nal.ctypes.data_as(ctypes.c_void_p), len(nal), window,
                                         o1.data_ptr() if o1 is not None else None,
                                         o2.data_ptr() if o2 is not None else None,
                                         o3.data_ptr() if o3 is not None else None, cap, ctypes.byref(rows))
        return rc, int(rows.value), o1, o2, o3

    def run(self, first, n_blocks, window, cap, nal=None, outs=(True, True, True)):
        rc, rows, o1, o2, o3 = self.call(first, n_blocks, window, cap, nal, outs)
        binding.check(rc)
        res = []
        for o, guard in ((o1, GUARD), (o2, -1.0), (o3, GUARD)):
            if o is None:
                res.append(None)
                continue
            h = o.cpu().numpy()
            if h.dtype == np.int32:
                h = h.view(np.uint32)
                assert (h[rows * window:] == GUARD).all()   # nothing written past the rows
            else:
                assert (h[rows * window:] == -1.0).all()
            res.append(h[:rows * window].reshape(rows, window))
        return (rows, *res)


def _general_file(rng, n=421, block_len=48):
    """Multi-allelic lines with missing and end-of-vector values and non-default phase; every 7th line with ALT 1 the
    majority allele (negated sparse); block 2 fully haploid lines next to plain diploid lines with missing values."""
    from test_gpu_score import _general_file as gf
    return gf(rng, n, block_len)


@pytest.fixture(scope="module")
def general():
    rng = np.random.default_rng(4242)
    n, block_len = 421, 48
    ref, dec, nal = _general_file(rng, n, block_len)
    X, C = gt_matrices(dec, nal, n)
    assert not C.all() and X.shape[0] > len(nal)   # missing values and multi-allelic lines are there
    hap = [i for i, (g, _) in enumerate(dec) if len(g) == n]
    assert hap
    return LDG(ref, nal), X, C, (len(nal) + block_len - 1) // block_len, block_len


@pytest.mark.parametrize("window", [1, 33, 200, 1000])
def test_ld_gt_whole_file_exact(general, window):
    S, X, C, nb, _ = general
    n_bin = X.shape[0]
    assert window != 1000 or window > n_bin
    e1, e2, e3 = band_gt(X, C, range(n_bin), window)
    rows, n11, r2, nc = S.run(0, nb, window, n_bin + 3)
    assert rows == n_bin
    assert np.array_equal(n11, e1), window
    assert np.array_equal(nc, e3), window
    assert same_r2(r2, e2), window
    past = (np.arange(n_bin)[:, None] + 1 + np.arange(window)[None, :]) >= n_bin
    assert (n11[past] == SENTINEL).all() and (nc[past] == SENTINEL).all() and np.isnan(r2[past]).all()
    assert (n11[~past] != SENTINEL).all() and (nc[~past] <= X.shape[1]).all()
    assert (nc[~past] < X.shape[1]).any()
    # each output alone gives the same values
    assert np.array_equal(S.run(0, nb, window, n_bin, outs=(True, False, False))[1], e1)
    assert same_r2(S.run(0, nb, window, n_bin, outs=(False, True, False))[2], e2)
    assert np.array_equal(S.run(0, nb, window, n_bin, outs=(False, False, True))[3], e3)


def test_ld_gt_same_bits_as_decode_ld():
    """On blocks decode_ld takes (bi-allelic, fully called; haploid and negated sparse lines), n11 and r2 are the same
    bits and n_called is N off the sentinels."""
    from test_gpu_ld import LD, _ld_file
    rng = np.random.default_rng(2024)
    n, n_lines, block_len = 701, 900, 128
    ref, dec, nb = _ld_file(rng, n, n_lines, block_len)
    P = LD(ref)
    S = LDG(ref, [2] * n_lines)
    for window in (1, 33, 300):
        _, a1, a2 = P.run(0, nb, window, n_lines)
        rows, n11, r2, nc = S.run(0, nb, window, n_lines)
        assert rows == n_lines
        assert np.array_equal(n11, a1), window
        assert np.array_equal(r2.view(np.uint32), a2.view(np.uint32)), window
        past = n11 == SENTINEL
        assert (nc[past] == SENTINEL).all() and (nc[~past] == 2 * n).all()


@pytest.mark.parametrize("window", [1, 33, 200])
def test_ld_gt_split_budget_lookahead_invariance(general, window):
    S, X, C, nb, block_len = general
    n_bin = X.shape[0]
    nal = S.nal
    _, one1, one2, one3 = S.run(0, nb, window, n_bin)
    bin_of = np.concatenate([[0], np.cumsum(nal.astype(np.int64) - 1)])
    parts = [[], [], []]
    for b0, b1 in ((0, 1), (1, 3), (3, nb)):
        l0 = b0 * block_len
        rows, a, b, c = S.run(b0, b1 - b0, window, n_bin, nal=nal[l0:])
        assert rows == bin_of[min(b1 * block_len, len(nal))] - bin_of[l0]
        for p, v in zip(parts, (a, b, c)):
            p.append(v)
    assert np.array_equal(np.concatenate(parts[0]), one1), window
    assert same_r2(np.concatenate(parts[1]), one2), window
    assert np.array_equal(np.concatenate(parts[2]), one3), window
    # exactly the BCF lines read: block 1 alone, its look-ahead into the multi-allelic / missing blocks after it
    end, lines = 2, 0
    while lines < window and end < nb:
        lines += bin_of[min((end + 1) * block_len, len(nal))] - bin_of[end * block_len]
        end += 1
    need = nal[block_len:min(end * block_len, len(nal))]
    r0, r1 = bin_of[block_len], bin_of[2 * block_len]
    rows, a, b, c = S.run(1, 1, window, n_bin, nal=need)
    assert np.array_equal(a, one1[r0:r1]) and same_r2(b, one2[r0:r1]) and np.array_equal(c, one3[r0:r1]), window
    # one block per range: the look-ahead lines composed again for every range
    ctx = S.G.ctx().handle
    binding.check(S.L.xsi_hip_ctx_set_workspace_budget(ctx, 1 << 16))
    try:
        _, a, b, c = S.run(0, nb, window, n_bin)
    finally:
        binding.check(S.L.xsi_hip_ctx_set_workspace_budget(ctx, 0))
    assert np.array_equal(a, one1) and same_r2(b, one2) and np.array_equal(c, one3), window


def test_ld_gt_mixed_tiles():
    """A clean file but for one line with a single missing haplotype and one line with every value missing: decode_ld
    refuses it; fully called tiles and four-count tiles meet in one call."""
    from oracle import oracle
    from test_gpu_ld import LD
    rng = np.random.default_rng(77)
    n, n_lines, block_len = 300, 420, 128
    lines = _random_lines(rng, n, n_lines, phase=True)
    gt = lines[150][0].copy()
    gt[37] &= 1
    lines[150] = (gt, 2)
    lines[260] = (np.tile(np.array([0, 1], dtype=np.int32), n), 2)
    ref = oracle.encode_file(lines, n, block_len=block_len, mac_thr=5, default_phased=oracle.default_phased_of(lines, n))
    dec = oracle.decode_file(ref, [2] * n_lines, block_len=block_len)
    X, C = gt_matrices(dec, [2] * n_lines, n)
    assert C[150].sum() == 2 * n - 1 and C[260].sum() == 0
    nb = (n_lines + block_len - 1) // block_len
    assert LD(ref).call(0, nb, 8, n_lines)[0] == binding.XSI_ERR_UNSUPPORTED
    S = LDG(ref, [2] * n_lines)
    for window in (1, 100, 200):
        e1, e2, e3 = band_gt(X, C, range(n_lines), window)
        rows, n11, r2, nc = S.run(0, nb, window, n_lines)
        assert np.array_equal(n11, e1) and np.array_equal(nc, e3) and same_r2(r2, e2), window
        p = np.arange(n_lines)[:, None] + 1 + np.arange(window)[None, :]
        r = np.broadcast_to(np.arange(n_lines)[:, None], p.shape)
        inside = p < n_lines
        clean = inside & (r != 150) & (p != 150) & (r != 260) & (p != 260)
        assert (nc[clean] == 2 * n).all()
        empty = inside & ((r == 260) | (p == 260))
        assert empty.any() and (nc[empty] == 0).all() and (n11[empty] == 0).all() and np.isnan(r2[empty]).all()
        one = inside & ((r == 150) | (p == 150)) & ~empty
        assert one.any() and (nc[one] == 2 * n - 1).all()


def test_ld_gt_large_n():
    """140 000 haplotypes (u32 A_T) over a few blocks with ~1 % missing values, against numpy on sampled rows."""
    from oracle import oracle
    rng = np.random.default_rng(140)
    n, n_lines, block_len = 70000, 24, 8
    lines = _random_lines(rng, n, n_lines, missing=True, phase=True)
    ref = oracle.encode_file(lines, n, block_len=block_len, mac_thr=50, default_phased=oracle.default_phased_of(lines, n))
    dec = oracle.decode_file(ref, [2] * n_lines, block_len=block_len)
    X, C = gt_matrices(dec, [2] * n_lines, n)
    S = LDG(ref, [2] * n_lines)
    nb = n_lines // block_len
    sample = [0, 3, 7, 8, 15, 20, 23]
    for window in (1, 10, 30):
        e1, e2, e3 = band_gt(X, C, sample, window)
        rows, n11, r2, nc = S.run(0, nb, window, n_lines)
        assert rows == n_lines
        assert np.array_equal(n11[sample], e1) and np.array_equal(nc[sample], e3), window
        assert same_r2(r2[sample], e2), window


def test_ld_gt_refusals(general):
    S, X, C, nb, block_len = general
    nal = S.nal
    n_bin = X.shape[0]
    # n_lines short of the look-ahead: block 0 alone with a window reaching into block 1
    rc = S.call(0, 1, 4, n_bin, nal=nal[:block_len])[0]
    assert rc == binding.XSI_ERR_ARG
    err = S.L.xsi_hip_last_error()
    assert b"decode_ld_gt" in err and b"reads %d BCF lines" % (2 * block_len) in err
    # and short of the requested blocks themselves
    assert S.call(0, 2, 1, n_bin, nal=nal[:block_len])[0] == binding.XSI_ERR_ARG
    # more lines than the file holds from the first block on
    assert S.call(1, 1, 4, n_bin, nal=np.concatenate([nal[block_len:], [2]]))[0] == binding.XSI_ERR_ARG
    # allele numbers that do not add up on a look-ahead block (block 1 read only for block 0's last rows)
    bad = nal.copy()
    i = block_len + int(np.nonzero(bad[block_len:2 * block_len] > 2)[0][0])
    bad[i] -= 1
    assert S.call(0, 1, 4, n_bin, nal=bad)[0] == binding.XSI_ERR_ARG
    assert b"look-ahead block 1" in S.L.xsi_hip_last_error()
    # ... which a call that does not read that block never sees
    bad3 = nal.copy()
    i3 = 3 * block_len + int(np.nonzero(bad3[3 * block_len:4 * block_len] > 2)[0][0])
    bad3[i3] -= 1
    bins0 = int((nal[:block_len] - 1).sum())
    assert S.run(0, 1, 4, bins0, nal=bad3)[0] == bins0
    # capacity below the row count
    assert S.call(0, 1, 4, bins0 - 1)[0] == binding.XSI_ERR_CAPACITY
    assert S.call(0, 2, 4, bins0, outs=(False, False, True))[0] == binding.XSI_ERR_CAPACITY
    # a zstd image (header flag set)
    z = bytearray(S.ref)
    z[17] |= 4
    assert LDG(bytes(z), nal).call(0, 1, 4, n_bin)[0] == binding.XSI_ERR_UNSUPPORTED
