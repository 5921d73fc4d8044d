"""GPU tests of the windowed haplotype LD (xsi_hip_decode_ld): pair counts n11 and r2 for every line against the
`window` lines after it, compared with `==` (r2 bit for bit) against numpy on the oracle-decoded or generator bits."""
import ctypes

import numpy as np
import pytest

from xsqueezeit_amd import binding
from ld_ref import SENTINEL, band, carrier_matrix, r2_ref, same_r2
from test_oracle import _random_lines

pytestmark = pytest.mark.gpu


class LD:
    def __init__(self, ref):
        import gpu_util as G
        self.G, self.torch, self.L = G, G.torch_mod(), binding.lib()
        self.ref = ref
        self.d_file = G.dev_u8(np.frombuffer(ref, dtype=np.uint8))

    def call(self, first, n_blocks, window, cap, n11=True, r2=True):
        torch = self.torch
        o1 = torch.full((cap * window + 7,), 0x7A7A7A7A, dtype=torch.int32, device="cuda") if n11 else None
        o2 = torch.full((cap * window + 7,), -1.0, dtype=torch.float32, device="cuda") if r2 else None
        rows = ctypes.c_uint64(0)
        rc = self.L.xsi_hip_decode_ld(self.G.ctx().handle, self.d_file.data_ptr(), len(self.ref), first, n_blocks, window,
                                      o1.data_ptr() if n11 else None, o2.data_ptr() if r2 else None, cap, ctypes.byref(rows))
        return rc, int(rows.value), o1, o2

    def run(self, first, n_blocks, window, cap, n11=True, r2=True):
        rc, rows, o1, o2 = self.call(first, n_blocks, window, cap, n11, r2)
        binding.check(rc)
        a = b = None
        if n11:
            h = o1.cpu().numpy().view(np.uint32)
            assert (h[rows * window:] == 0x7A7A7A7A).all()  # nothing written past the rows
            a = h[:rows * window].reshape(rows, window)
        if r2:
            h = o2.cpu().numpy()
            assert (h[rows * window:] == -1.0).all()
            b = h[:rows * window].reshape(rows, window)
        return rows, a, b


def _ld_file(rng, n=701, n_lines=900, block_len=128):
    """Bi-allelic, fully called, mixed phase; every 9th line with the ALT allele in the majority (negated sparse);
    lines 120 .. 169 fully haploid (across a block boundary), some of them majority-ALT; a few monomorphic lines."""
    from oracle import oracle
    lines = _random_lines(rng, n, n_lines, phase=True)
    for i in range(0, n_lines, 9):
        gt = lines[i][0]
        flip = ((gt >> 1) - 1) ^ 1
        lines[i] = ((((flip + 1) << 1) | (gt & 1)).astype(np.int32), 2)
    for i in range(120, 170):
        al = (rng.random(n) < (0.97 if i % 5 == 0 else 0.15)).astype(np.int32)
        lines[i] = (((al + 1) << 1).astype(np.int32), 2)
    for i in (7, 300, 301):   # no ALT carrier: r2 NaN against every partner
        lines[i] = ((np.full(2 * n, 2, dtype=np.int32) | np.tile([0, 1], n).astype(np.int32)), 2)
    ref = oracle.encode_file(lines, n, block_len=block_len, mac_thr=14, default_phased=oracle.default_phased_of(lines, n))
    dec = oracle.decode_file(ref, [2] * n_lines, block_len=block_len)
    return ref, dec, (n_lines + block_len - 1) // block_len


@pytest.fixture(scope="module")
def small():
    rng = np.random.default_rng(2024)
    n, n_lines, block_len = 701, 900, 128   # 8 blocks, the last one short
    ref, dec, nb = _ld_file(rng, n, n_lines, block_len)
    X = carrier_matrix(dec, n)
    assert X[120:170, 1::2].sum() == 0 and X[120:170].sum() > 0
    return LD(ref), X, nb, block_len


@pytest.mark.parametrize("window", [1, 31, 32, 33, 200, 300, 700])
def test_ld_whole_file_exact(small, window):
    S, X, nb, _ = small
    n_lines = X.shape[0]
    exp1, exp2 = band(X, range(n_lines), window)
    rows, n11, r2 = S.run(0, nb, window, n_lines + 3)
    assert rows == n_lines
    assert np.array_equal(n11, exp1), window
    assert same_r2(r2, exp2), window
    # sentinels exactly where the partner lies past the file's last line
    past = (np.arange(n_lines)[:, None] + 1 + np.arange(window)[None, :]) >= n_lines
    assert (n11[past] == SENTINEL).all() and np.isnan(r2[past]).all()
    assert (n11[~past] != SENTINEL).all()
    # each output alone gives the same values
    _, a, _ = S.run(0, nb, window, n_lines, r2=False)
    assert np.array_equal(a, exp1)
    _, _, b = S.run(0, nb, window, n_lines, n11=False)
    assert same_r2(b, exp2)


def test_ld_r2_nan_on_monomorphic_lines(small):
    S, X, nb, _ = small
    rows, n11, r2 = S.run(0, nb, 40, X.shape[0])
    assert np.isnan(r2[7]).all() and (n11[7] == 0).all()
    assert np.isnan(r2[300]).all() and np.isnan(r2[301]).all()
    assert np.isnan(r2[299, 0]) and np.isnan(r2[299, 1])   # partners 300, 301
    assert np.isfinite(r2[299, 2:]).any()


@pytest.mark.parametrize("window", [1, 33, 200, 300])
def test_ld_split_and_budget_invariance(small, window):
    S, X, nb, block_len = small
    n_lines = X.shape[0]
    _, one1, one2 = S.run(0, nb, window, n_lines)
    parts1, parts2 = [], []
    for b0, b1 in ((0, 2), (2, 5), (5, nb)):
        rows, a, b = S.run(b0, b1 - b0, window, n_lines)
        assert rows == min(b1 * block_len, n_lines) - b0 * block_len
        parts1.append(a)
        parts2.append(b)
    assert np.array_equal(np.concatenate(parts1), one1), window
    assert same_r2(np.concatenate(parts2), one2), window
    # one block per range: the look-ahead lines decoded again for every range
    ctx = S.G.ctx().handle
    binding.check(S.L.xsi_hip_ctx_set_workspace_budget(ctx, 1 << 16))
    try:
        _, a, b = S.run(0, nb, window, n_lines)
    finally:
        binding.check(S.L.xsi_hip_ctx_set_workspace_budget(ctx, 0))
    assert np.array_equal(a, one1) and same_r2(b, one2), window
    # a middle block alone: its partners come from the blocks after it
    rows, a, b = S.run(2, 1, window, block_len)
    assert np.array_equal(a, one1[2 * block_len:3 * block_len]) and same_r2(b, one2[2 * block_len:3 * block_len])


def test_ld_timing_stage(small):
    S, X, nb, _ = small
    ctx = S.G.ctx()
    ctx.set_timing(True)
    try:
        S.run(0, nb, 64, X.shape[0])
        st = ctx.timing()
    finally:
        ctx.set_timing(False)
    assert st["ld"][1] > 0 and st["ld"][0] > 0.0


def _synth_file(torch, L, ctx, n_haps, block_len, n_blocks, seed):
    from xsqueezeit_amd import synth
    n, S_ = n_haps // 2, block_len * n_blocks
    thr = max(1, int(n_haps * 0.001))
    stride = synth.row_stride_bytes(n_haps)
    p = binding.EncodeParams(n, block_len, thr, 1, 0, 0)
    d_bits = torch.empty(S_ * stride, dtype=torch.uint8, device="cuda")
    binding.check(L.xsi_hip_synth_packed(ctx.handle, seed, 0, S_, n_haps, d_bits.data_ptr(), stride))
    cap = int(L.xsi_hip_encode_bound(ctypes.byref(p), S_, S_))
    d_file = torch.zeros(256 + cap + 8 * n_blocks + 64, dtype=torch.uint8, device="cuda")
    d_off = torch.zeros(n_blocks, dtype=torch.int64, device="cuda")
    res = binding.EncodeResult()
    binding.check(L.xsi_hip_encode_packed(ctx.handle, ctypes.byref(p), d_bits.data_ptr(), S_, stride,
                                          d_file[256:].data_ptr(), cap, d_off.data_ptr(), ctypes.byref(res)))
    nb = res.blocks_bytes
    io = 256 + nb + ((-(256 + nb)) % 8)
    so = io + 8 * n_blocks
    hf = binding.HeaderFields(n, 2, block_len, thr, 1, 0, S_, S_, io, so)
    hdr = (ctypes.c_uint8 * 256)()
    binding.check(L.xsi_hip_make_header(ctypes.byref(hf), hdr))
    d_file[:256] = torch.frombuffer(bytearray(hdr), dtype=torch.uint8).to("cuda")
    d_file[io:so] = d_off.view(torch.uint8)
    shifts = torch.arange(8, dtype=torch.uint8, device="cuda")
    X = ((d_bits.view(S_, stride).unsqueeze(-1) >> shifts) & 1).reshape(S_, -1)[:, :n_haps]
    return d_file, so, X


@pytest.mark.parametrize("n_haps,block_len,n_blocks", [(5008, 256, 3), (140000, 128, 3)])
def test_ld_synth_files(n_haps, block_len, n_blocks):
    """Generator bits through the GPU encoder; 140 000 haplotypes take u32 A_T and the long-row decode chain."""
    import gpu_util as G
    torch = G.torch_mod()
    L = binding.lib()
    ctx = G.ctx()
    d_file, flen, Xd = _synth_file(torch, L, ctx, n_haps, block_len, n_blocks, 11)
    S_ = Xd.shape[0]
    Xf = Xd.to(torch.float64)
    gram = (Xf @ Xf.T).round().to(torch.int64).cpu().numpy()   # counts below 2^53: exact
    cnt = Xd.to(torch.int64).sum(1).cpu().numpy()
    for window in (1, 100, 300):
        n11 = torch.zeros(S_ * window, dtype=torch.int32, device="cuda")
        r2 = torch.zeros(S_ * window, dtype=torch.float32, device="cuda")
        rows = ctypes.c_uint64(0)
        binding.check(L.xsi_hip_decode_ld(ctx.handle, d_file.data_ptr(), flen, 0, n_blocks, window, n11.data_ptr(),
                                          r2.data_ptr(), S_, ctypes.byref(rows)))
        assert rows.value == S_
        got1 = n11.cpu().numpy().view(np.uint32).reshape(S_, window)
        got2 = r2.cpu().numpy().reshape(S_, window)
        p = np.arange(S_)[:, None] + 1 + np.arange(window)[None, :]
        ok = p < S_
        pc = np.minimum(p, S_ - 1)
        exp1 = np.where(ok, gram[np.arange(S_)[:, None], pc], SENTINEL).astype(np.uint32)
        exp2 = np.where(ok, r2_ref(n_haps, exp1.astype(np.int64), cnt[:, None], cnt[pc]), np.float32(np.nan))
        assert np.array_equal(got1, exp1), (n_haps, window)
        assert same_r2(got2, exp2), (n_haps, window)


def test_ld_refusals():
    from oracle import oracle
    rng = np.random.default_rng(7)
    n, block_len = 90, 32
    lines = _random_lines(rng, n, 2 * block_len, phase=True)
    lines += _random_lines(rng, n, 1, multi=True)                  # block 2: a multi-allelic line
    while lines[-1][1] < 3:
        lines[-1:] = _random_lines(rng, n, 1, multi=True)
    lines += _random_lines(rng, n, block_len - 1, phase=True)
    lines += _random_lines(rng, n, block_len, phase=True)          # block 3: plain
    lines += _random_lines(rng, n, 3, missing=True)                # block 4: missing entries
    ref = oracle.encode_file(lines, n, block_len=block_len, mac_thr=3, default_phased=oracle.default_phased_of(lines, n))
    S = LD(ref)
    # requested blocks with a multi-allelic / missing line
    assert S.call(2, 1, 4, 200)[0] == binding.XSI_ERR_UNSUPPORTED
    assert b"block 2" in S.L.xsi_hip_last_error()
    assert S.call(4, 1, 4, 200)[0] == binding.XSI_ERR_UNSUPPORTED
    # look-ahead-only blocks: block 1's last rows need block 2's first line, block 3's need block 4's
    assert S.call(1, 1, 1, 200)[0] == binding.XSI_ERR_UNSUPPORTED
    assert b"look-ahead block 2" in S.L.xsi_hip_last_error()
    assert S.call(3, 1, 1, 200)[0] == binding.XSI_ERR_UNSUPPORTED
    assert S.call(0, 1, 40, 200)[0] == binding.XSI_ERR_UNSUPPORTED   # window past block 1 into block 2
    # a look-ahead that stops in front of the bad block is fine
    rows, a, _ = S.run(0, 1, block_len, block_len)
    assert rows == block_len
    # capacity below the row count
    assert S.call(0, 1, 4, block_len - 1)[0] == binding.XSI_ERR_CAPACITY
    assert S.call(0, 2, 4, 2 * block_len - 1, r2=False)[0] == binding.XSI_ERR_CAPACITY
    # a zstd image (header flag set)
    z = bytearray(ref)
    z[17] |= 4
    assert LD(bytes(z)).call(0, 1, 4, 200)[0] == binding.XSI_ERR_UNSUPPORTED
