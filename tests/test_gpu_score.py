"""GPU tests of the weighted genotype scores (xsi_hip_decode_score / xsi_hip_decode_score_gt): out[i][k] = sum over
binary lines r of dosage(i, r) * w[r][k].  Dyadic weights (integers in +-2^20 times 2^-10) make every partial sum
exact, so the comparisons against numpy / torch are `==`; random normal weights are checked with rtol 1e-12."""
import ctypes

import numpy as np
import pytest

from xsqueezeit_amd import binding
from test_oracle import _random_lines

pytestmark = pytest.mark.gpu

ACC, PER_HAP = binding.SCORE_ACCUMULATE, binding.SCORE_PER_HAPLOTYPE


def _dyadic(rng, shape, bits=20, scale=10):
    return rng.integers(-(2 ** bits), 2 ** bits + 1, size=shape).astype(np.float64) * 2.0 ** -scale


def _dosage_matrix(dec, nal, n, per_hap):
    """[n_out x n_bin] dosages of oracle-decoded rows, by the header's rules (missing / eov carry no allele)."""
    cols = []
    for (g, _), na in zip(dec, nal):
        al = (g.astype(np.int64) >> 1) - 1
        haploid = len(g) == n
        for k in range(1, na):
            hit = (al == k).astype(np.float64)
            if per_hap:
                col = np.zeros(2 * n)
                if haploid:
                    col[0::2] = hit
                else:
                    col[:] = hit
            else:
                col = hit if haploid else hit[0::2] + hit[1::2]
            cols.append(col)
    return np.stack(cols, axis=1)


class Scorer:
    def __init__(self, ref, nal=None):
        import gpu_util as G
        self.G, self.torch, self.L = G, G.torch_mod(), binding.lib()
        self.ref = ref
        self.d_file = G.dev_u8(np.frombuffer(ref, dtype=np.uint8))
        self.nal = None if nal is None else np.ascontiguousarray(nal, dtype=np.uint32)

    def call(self, w, first=0, n_blocks=1, flags=0, out=None, rows=None, gt=False, nal=None, n_weight_lines=None):
        torch = self.torch
        d_w = torch.from_numpy(np.ascontiguousarray(w)).cuda()
        K = w.shape[1]
        if out is None:
            out = torch.full((rows, K), np.nan, dtype=torch.float64, device="cuda")
        nwl = w.shape[0] if n_weight_lines is None else n_weight_lines
        if gt:
            nal = self.nal if nal is None else np.ascontiguousarray(nal, dtype=np.uint32)
            rc = self.L.xsi_hip_decode_score_gt(self.G.ctx().handle, self.d_file.data_ptr(), len(self.ref), first, n_blocks,
                                                nal.ctypes.data, len(nal), d_w.data_ptr(), nwl, K, out.data_ptr(),
                                                out.shape[0], flags)
        else:
            rc = self.L.xsi_hip_decode_score(self.G.ctx().handle, self.d_file.data_ptr(), len(self.ref), first, n_blocks,
                                             d_w.data_ptr(), nwl, K, out.data_ptr(), out.shape[0], flags)
        return rc, out

    def run(self, w, **kw):
        rc, out = self.call(w, **kw)
        binding.check(rc)
        return out.cpu().numpy()


def _plane_file(rng, n=700, n_lines=500, block_len=128):
    """Bi-allelic, fully called, mixed phase; every 9th line with the ALT allele in the majority (negated sparse)."""
    from oracle import oracle
    lines = _random_lines(rng, n, n_lines, phase=True)
    for i in range(0, n_lines, 9):
        gt = lines[i][0]
        flip = ((gt >> 1) - 1) ^ 1
        lines[i] = ((((flip + 1) << 1) | (gt & 1)).astype(np.int32), 2)
    ref = oracle.encode_file(lines, n, block_len=block_len, mac_thr=14, default_phased=oracle.default_phased_of(lines, n))
    dec = oracle.decode_file(ref, [2] * n_lines, block_len=block_len)
    return ref, dec, (n_lines + block_len - 1) // block_len


def test_score_plane_path_exact():
    rng = np.random.default_rng(5150)
    n, n_lines = 700, 500
    ref, dec, nb = _plane_file(rng, n, n_lines)
    S = Scorer(ref, [2] * n_lines)
    for per_hap in (False, True):
        X = _dosage_matrix(dec, [2] * n_lines, n, per_hap)
        rows = X.shape[0]
        for K in (1, 3, 8, 21):   # vector form, MFMA form, partial MFMA tile
            w = _dyadic(rng, (n_lines, K))
            got = S.run(w, n_blocks=nb, flags=PER_HAP if per_hap else 0, rows=rows + 5)
            assert np.array_equal(got[:rows], X @ w), (per_hap, K)
            assert np.isnan(got[rows:]).all()
            # general path on the same file: the same bits
            got_gt = S.run(w, n_blocks=nb, flags=PER_HAP if per_hap else 0, rows=rows, gt=True)
            assert np.array_equal(got_gt, got[:rows]), (per_hap, K)
        # random normal weights: rtol 1e-12
        for K in (2, 17):
            w = rng.normal(0.0, 1.0, size=(n_lines, K))
            got = S.run(w, n_blocks=nb, flags=PER_HAP if per_hap else 0, rows=rows)
            assert np.allclose(got, X @ w, rtol=1e-12, atol=1e-9)


def test_score_haploid_block_both_paths():
    """A block of fully haploid lines (compact sample bits) between diploid blocks, both output modes, both forms."""
    from oracle import oracle
    rng = np.random.default_rng(77)
    n, block_len = 333, 40
    lines = _random_lines(rng, n, block_len, phase=True)
    for i in range(block_len):
        al = (rng.random(n) < (0.99 if i % 6 == 0 else 0.2)).astype(np.int32)   # some majority-ALT haploid lines
        lines.append((((al + 1) << 1).astype(np.int32), 2))
    lines.extend(_random_lines(rng, n, 25, phase=True))
    nal = [2] * len(lines)
    ref = oracle.encode_file(lines, n, block_len=block_len, mac_thr=6, default_phased=oracle.default_phased_of(lines, n))
    dec = oracle.decode_file(ref, nal, block_len=block_len)
    S = Scorer(ref, nal)
    for per_hap in (False, True):
        X = _dosage_matrix(dec, nal, n, per_hap)
        for K in (1, 4, 5, 16, 19):
            w = _dyadic(rng, (len(lines), K))
            fl = PER_HAP if per_hap else 0
            got = S.run(w, n_blocks=3, flags=fl, rows=X.shape[0])
            assert np.array_equal(got, X @ w), (per_hap, K)
            assert np.array_equal(S.run(w, n_blocks=3, flags=fl, rows=X.shape[0], gt=True), got)
            # the haploid block alone
            w1 = np.ascontiguousarray(w[block_len:2 * block_len])
            got1 = S.run(w1, first=1, n_blocks=1, flags=fl, rows=X.shape[0])
            assert np.array_equal(got1, X[:, block_len:2 * block_len] @ w1), (per_hap, K)


def _general_file(rng, n=421, block_len=48):
    from oracle import oracle
    lines = []
    for b in range(5):
        for i in range(block_len if b < 4 else 17):
            if b == 2:     # fully haploid and plain diploid lines
                if i % 3 == 0:
                    al = (rng.random(n) < 0.4).astype(np.int32)
                    lines.append((((al + 1) << 1).astype(np.int32), 2))
                else:
                    lines.extend(_random_lines(rng, n, 1, missing=(i % 4 == 1)))
            else:
                lines.extend(_random_lines(rng, n, 1, multi=True, missing=(i % 3 == 0), eov=(i % 5 == 0), phase=True))
                if i % 7 == 0:   # ALT 1 the majority allele: a negated sparse line
                    gt, na = lines[-1]
                    keep = (gt == oracle.INT32_VECTOR_END) | ((gt >> 1) == 0)
                    al = (gt >> 1) - 1
                    sw = np.where(al == 0, 1, np.where(al == 1, 0, al))
                    g2 = (((sw + 1) << 1) | (gt & 1)).astype(np.int32)
                    lines[-1] = (np.where(keep, gt, g2).astype(np.int32), na)
    nal = [na for _, na in lines]
    ref = oracle.encode_file(lines, n, block_len=block_len, mac_thr=9, default_phased=oracle.default_phased_of(lines, n))
    return ref, oracle.decode_file(ref, nal, block_len=block_len), nal


def test_score_general_path_and_determinism():
    rng = np.random.default_rng(909)
    n, block_len = 421, 48
    ref, dec, nal = _general_file(rng, n, block_len)
    n_bin = sum(a - 1 for a in nal)
    S = Scorer(ref, nal)
    for per_hap in (False, True):
        fl = PER_HAP if per_hap else 0
        X = _dosage_matrix(dec, nal, n, per_hap)
        rows = X.shape[0]
        for K in (1, 5, 8, 21):
            w = _dyadic(rng, (n_bin, K))
            one = S.run(w, n_blocks=5, flags=fl, rows=rows, gt=True)
            assert np.array_equal(one, X @ w), (per_hap, K)
            # repeated call
            assert np.array_equal(S.run(w, n_blocks=5, flags=fl, rows=rows, gt=True), one)
            # the range split into 3 calls with ACCUMULATE
            cuts_blk = [0, 2, 3, 5]
            out = S.torch.full((rows, K), np.nan, dtype=S.torch.float64, device="cuda")
            for c in range(3):
                b0, b1 = cuts_blk[c], cuts_blk[c + 1]
                l0, l1 = b0 * block_len, min(b1 * block_len, len(nal))
                r0, r1 = sum(a - 1 for a in nal[:l0]), sum(a - 1 for a in nal[:l1])
                S.call(np.ascontiguousarray(w[r0:r1]), first=b0, n_blocks=b1 - b0, flags=fl | (ACC if c else 0), out=out,
                       gt=True, nal=nal[l0:l1])
            assert np.array_equal(out.cpu().numpy(), one), (per_hap, K)
            # one block per range (tiny workspace budget)
            binding.check(S.L.xsi_hip_ctx_set_workspace_budget(S.G.ctx().handle, 1 << 16))
            try:
                small = S.run(w, n_blocks=5, flags=fl, rows=rows, gt=True)
            finally:
                binding.check(S.L.xsi_hip_ctx_set_workspace_budget(S.G.ctx().handle, 0))
            assert np.array_equal(small, one), (per_hap, K)
            # accumulating onto a nonzero output adds to it
            base = _dyadic(rng, (rows, K))
            out = S.torch.from_numpy(base.copy()).cuda()
            rc, out = S.call(w, n_blocks=5, flags=fl | ACC, out=out, gt=True)
            binding.check(rc)
            assert np.array_equal(out.cpu().numpy(), base + one)
        w = rng.normal(0.0, 1.0, size=(n_bin, 3))
        assert np.allclose(S.run(w, n_blocks=5, flags=fl, rows=rows, gt=True), X @ w, rtol=1e-12, atol=1e-9)


def test_score_plane_path_determinism():
    rng = np.random.default_rng(31337)
    ref, dec, nb = _plane_file(rng, 650, 600, 128)
    S = Scorer(ref)
    for K in (3, 24):
        w = _dyadic(rng, (600, K))
        wn = rng.normal(0.0, 1.0, size=(600, K))   # determinism holds for any weights, not only exact ones
        for ww in (w, wn):
            one = S.run(ww, n_blocks=nb, rows=650)
            assert np.array_equal(S.run(ww, n_blocks=nb, rows=650), one)
            out = S.torch.zeros((650, K), dtype=S.torch.float64, device="cuda")
            for c, (b0, b1) in enumerate([(0, 1), (1, 3), (3, nb)]):
                S.call(np.ascontiguousarray(ww[b0 * 128:min(b1 * 128, 600)]), first=b0, n_blocks=b1 - b0,
                       flags=ACC if c else 0, out=out)
            assert np.array_equal(out.cpu().numpy(), one), K
            binding.check(S.L.xsi_hip_ctx_set_workspace_budget(S.G.ctx().handle, 1 << 16))
            try:
                assert np.array_equal(S.run(ww, n_blocks=nb, rows=650), one), K
            finally:
                binding.check(S.L.xsi_hip_ctx_set_workspace_budget(S.G.ctx().handle, 0))
            assert np.array_equal(S.run(ww, n_blocks=nb, rows=650, gt=True, nal=[2] * 600), one), K


def test_score_transpose_identity_with_decode_dot():
    """sum_r sum_k W[r,k] dot(Y)[r,j] == sum_i sum_k score(W)[i,k] Y[i,j], exactly (small dyadic values)."""
    rng = np.random.default_rng(4711)
    n, n_lines = 700, 500
    ref, dec, nb = _plane_file(rng, n, n_lines)
    S = Scorer(ref)
    torch = S.torch
    for K, J in ((3, 2), (16, 9)):
        W = _dyadic(rng, (n_lines, K), bits=8, scale=4)
        Y = _dyadic(rng, (n, J), bits=8, scale=4)
        d_y = torch.from_numpy(Y).cuda()
        D = torch.zeros((n_lines, J), dtype=torch.float64, device="cuda")
        binding.check(S.L.xsi_hip_decode_dot(S.G.ctx().handle, S.d_file.data_ptr(), len(ref), 0, nb, d_y.data_ptr(), J,
                                             D.data_ptr(), n_lines, None))
        Sc = S.run(W, n_blocks=nb, rows=n)
        assert np.array_equal(W.T @ D.cpu().numpy(), Sc.T @ Y)


def test_score_nonfinite_weights_reach_carriers_only():
    rng = np.random.default_rng(2718)
    n, n_lines = 700, 500
    ref, dec, nb = _plane_file(rng, n, n_lines)
    S = Scorer(ref, [2] * n_lines)
    for per_hap in (False, True):
        X = _dosage_matrix(dec, [2] * n_lines, n, per_hap)
        counts = (X > 0).sum(0)
        a, b = [int(i) for i in np.nonzero((counts > 0) & (counts < X.shape[0] // 3))[0][:2]]
        for K in (2, 16):
            w = _dyadic(rng, (n_lines, K))
            w[a, 0] = np.nan
            w[b, K - 1] = np.inf
            for gt in (False, True):
                got = S.run(w, n_blocks=nb, flags=PER_HAP if per_hap else 0, rows=X.shape[0], gt=gt)
                wf = w.copy()
                wf[a, 0] = 0.0
                wf[b, K - 1] = 0.0
                exp = X @ wf
                bad = np.zeros_like(exp, dtype=bool)
                bad[X[:, a] > 0, 0] = True
                bad[X[:, b] > 0, K - 1] = True
                assert np.isnan(got[X[:, a] > 0, 0]).all()
                assert not np.isfinite(got[bad]).any()
                assert np.array_equal(got[~bad], exp[~bad]), (per_hap, K, gt)


@pytest.mark.parametrize("n_haps,block_len,n_blocks", [(64976, 1024, 3), (140000, 1024, 2)])
def test_score_large_haplotype_counts(n_haps, block_len, n_blocks):
    """u16 and u32 A_T files from the bench generator; expected = torch float64 matmul of the encoder's input bits."""
    import gpu_util as G
    from xsqueezeit_amd import synth
    torch = G.torch_mod()
    L = binding.lib()
    ctx = G.ctx()
    n, S_ = n_haps // 2, block_len * n_blocks
    thr = max(1, int(n_haps * 0.001))
    stride = synth.row_stride_bytes(n_haps)
    p = binding.EncodeParams(n, block_len, thr, 1, 0, 0)
    d_bits = torch.empty(S_ * stride, dtype=torch.uint8, device="cuda")
    binding.check(L.xsi_hip_synth_packed(ctx.handle, 7, 0, S_, n_haps, d_bits.data_ptr(), stride))
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
    # input bits -> float64 dosages [lines x haps], by chunks of lines
    shifts = torch.arange(8, dtype=torch.uint8, device="cuda")
    rng = np.random.default_rng(n_haps)
    for K in (1, 16):
        w = torch.from_numpy(_dyadic(rng, (S_, K))).cuda()
        exp_h = torch.zeros((n_haps, K), dtype=torch.float64, device="cuda")
        for l0 in range(0, S_, 512):
            rows = d_bits[l0 * stride:(l0 + 512) * stride].view(-1, stride)
            bits = ((rows.unsqueeze(-1) >> shifts) & 1).reshape(rows.shape[0], -1)[:, :n_haps].to(torch.float64)
            exp_h += bits.T @ w[l0:l0 + 512]
        exp_s = exp_h.view(n, 2, K).sum(1)
        for fl, exp in ((0, exp_s), (PER_HAP, exp_h)):
            out = torch.full((exp.shape[0], K), np.nan, dtype=torch.float64, device="cuda")
            binding.check(L.xsi_hip_decode_score(ctx.handle, d_file.data_ptr(), so, 0, n_blocks, w.data_ptr(), S_, K,
                                                 out.data_ptr(), exp.shape[0], fl))
            assert torch.equal(out, exp), (K, fl)


def test_score_refusals():
    rng = np.random.default_rng(99)
    ref, dec, nal = _general_file(rng, 90, 48)
    n_bin = sum(a - 1 for a in nal)
    S = Scorer(ref, nal)
    w = _dyadic(rng, (n_bin, 2))
    # plane path on multi-allelic / missing blocks
    rc, _ = S.call(w, n_blocks=5, rows=90)
    assert rc == binding.XSI_ERR_UNSUPPORTED
    # wrong n_weight_lines
    rc, _ = S.call(w, n_blocks=5, rows=90, gt=True, n_weight_lines=n_bin - 1)
    assert rc == binding.XSI_ERR_ARG
    # sum(n_allele - 1) mismatch (same BCF line count)
    bad = np.asarray(nal, dtype=np.uint32).copy()
    bad[3] += 1
    rc, _ = S.call(w, n_blocks=5, rows=90, gt=True, nal=bad)
    assert rc == binding.XSI_ERR_ARG
    # a shifted allele number that keeps the total but breaks a block
    bad2 = np.asarray(nal, dtype=np.uint32).copy()
    i = int(np.nonzero(bad2[:48] > 2)[0][0])
    bad2[i] -= 1
    bad2[100] += 1
    rc, _ = S.call(w, n_blocks=5, rows=90, gt=True, nal=bad2)
    assert rc == binding.XSI_ERR_ARG
    # n_lines not matching the blocks
    rc, _ = S.call(w, n_blocks=5, rows=90, gt=True, nal=nal[:-1])
    assert rc == binding.XSI_ERR_ARG
    # out_rows too small (per sample, then per haplotype)
    rc, _ = S.call(w, n_blocks=5, rows=89, gt=True)
    assert rc == binding.XSI_ERR_CAPACITY
    rc, _ = S.call(w, n_blocks=5, rows=179, gt=True, flags=PER_HAP)
    assert rc == binding.XSI_ERR_CAPACITY
    ref_p, _, nb = _plane_file(rng, 100, 200, 64)
    P = Scorer(ref_p)
    wp = _dyadic(rng, (200, 1))
    rc, _ = P.call(wp, n_blocks=nb, rows=99)
    assert rc == binding.XSI_ERR_CAPACITY
    rc, _ = P.call(wp, n_blocks=nb, rows=100, n_weight_lines=201)
    assert rc == binding.XSI_ERR_ARG
    # a zstd image (header flag set) is refused on both paths
    z = bytearray(ref_p)
    z[17] |= 4
    Z = Scorer(bytes(z), [2] * 200)
    rc, _ = Z.call(wp, n_blocks=nb, rows=100)
    assert rc == binding.XSI_ERR_UNSUPPORTED
    rc, _ = Z.call(wp, n_blocks=nb, rows=100, gt=True)
    assert rc == binding.XSI_ERR_UNSUPPORTED
