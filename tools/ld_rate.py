#!/usr/bin/env python3
"""Rate of xsi_hip_decode_ld (windowed haplotype LD: pair counts and r2 on the decoded blocks) on the bench generator's
matrix, against xsi_hip_decode_dot at K = 1 on the same file (the cost of decoding the planes) and against the route a
caller has without it: xsi_hip_decode_packed one block at a time -> unpack to float64 in torch -> banded matmul.
Prints one JSON line per shape and window.

--gt: xsi_hip_decode_ld_gt instead.  Per shape it times decode_ld_gt and decode_ld on the bench file (bi-allelic, every
value called), then builds a general file from the same bits (int32 rows in torch, ~1 % of the values missing on every
line, ~1 % tri-allelic lines, xsi_hip_encode_gt) and times decode_ld_gt on it against the route without it:
xsi_hip_decode_gt a few blocks at a time -> carrier / called masks in torch -> four banded matmuls, extrapolated."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from score_rate import build_file, timed  # noqa: E402

# int8 matrix-core peak of the MI355X, dense (2x the bf16 rate per clock): one pair-bit is one MAC of that form
I8_MFMA_MACS = 2.5e15


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="5008x1000000,64976x262144", help="comma-separated HAPSxSITES")
    ap.add_argument("--windows", default="32,256,1024")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--baseline-blocks", type=int, default=8, help="blocks timed for the decode_packed + torch route")
    ap.add_argument("--gt", action="store_true", help="time xsi_hip_decode_ld_gt (see above)")
    ap.add_argument("--missing", type=float, default=0.01, help="--gt: share of missing values on every line")
    ap.add_argument("--multi", type=float, default=0.01, help="--gt: share of tri-allelic lines")
    args = ap.parse_args()
    if args.gt:
        return main_gt(args)
    import torch
    from xsqueezeit_amd import binding, synth
    L = binding.lib()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    ctx = binding.Context(0, stream.cuda_stream)
    windows = [int(w) for w in args.windows.split(",")]
    name = torch.cuda.get_device_name(0)
    for shape in args.shapes.split(","):
        N, S = (int(x) for x in shape.split("x"))
        d_file, flen, n_blocks, d_bits, stride = build_file(L, binding, synth, ctx, torch, dev, N, S)
        del d_bits
        torch.cuda.empty_cache()
        y = torch.randn((N // 2, 1), dtype=torch.float64, device=dev)
        dout = torch.zeros((S, 1), dtype=torch.float64, device=dev)

        def dot():
            binding.check(L.xsi_hip_decode_dot(ctx.handle, d_file.data_ptr(), flen, 0, n_blocks, y.data_ptr(), 1,
                                               dout.data_ptr(), S, None))
        ms_dot = timed(dot, args.reps)
        del y, dout
        # the route without decode_ld: the first blocks (and one more for the look-ahead) as packed rows
        nbb = min(args.baseline_blocks, n_blocks)
        nbd = min(nbb + 1, n_blocks)
        rows_buf = torch.empty(nbd * 8192 * stride, dtype=torch.uint8, device=dev)
        shifts = torch.arange(8, dtype=torch.uint8, device=dev)
        nrow = ctypes.c_uint64(0)
        for W in windows:
            n11 = torch.empty(S * W, dtype=torch.int32, device=dev)
            r2 = torch.empty(S * W, dtype=torch.float32, device=dev)
            rows = ctypes.c_uint64(0)

            def ld(nb=n_blocks, o1=n11, o2=r2):
                binding.check(L.xsi_hip_decode_ld(ctx.handle, d_file.data_ptr(), flen, 0, nb, W, o1.data_ptr(),
                                                  o2.data_ptr(), S, ctypes.byref(rows)))
            ms_ld = timed(ld, args.reps)
            ctx.set_timing(True)
            ld()
            torch.cuda.synchronize()
            st = ctx.timing()
            ctx.set_timing(False)
            stage_ms = st.get("ld", (0.0, 0))[0]
            pair_bits = float(N) * S * W
            band_b = torch.empty((nbb * 8192, W), dtype=torch.float64, device=dev)

            def baseline():
                lines = 0
                for b in range(nbd):
                    binding.check(L.xsi_hip_decode_packed(ctx.handle, d_file.data_ptr(), flen, b, 1,
                                                          rows_buf[lines * stride:].data_ptr(), stride, 8192,
                                                          ctypes.byref(nrow), None))
                    lines += int(nrow.value)
                n_rows = min(nbb * 8192, lines)
                for r0 in range(0, n_rows, 1024):
                    r1 = min(r0 + 1024, n_rows)
                    c1 = min(r1 + W, lines)
                    bits = ((rows_buf[r0 * stride:c1 * stride].view(c1 - r0, stride).unsqueeze(-1) >> shifts) & 1)
                    X = bits.reshape(c1 - r0, -1)[:, :N].to(torch.float64)
                    G = X[:r1 - r0] @ X[1:].T  # G[i, k] = pair (r0 + i, r0 + 1 + k)
                    if G.shape[1] < (r1 - r0 - 1) + W:
                        G = torch.nn.functional.pad(G, (0, (r1 - r0 - 1) + W - G.shape[1]), value=-1.0)
                    band_b[r0:r1] = G.as_strided((r1 - r0, W), (G.stride(0) + 1, 1))
                return n_rows, lines
            ms_base_part = timed(baseline, 1)
            n_rows, lines = baseline()
            torch.cuda.synchronize()
            ms_base = ms_base_part * n_blocks / nbb
            # decode_ld on the same blocks against the baseline's band (partners it decoded)
            o1 = torch.empty(n_rows * W, dtype=torch.int32, device=dev)
            binding.check(L.xsi_hip_decode_ld(ctx.handle, d_file.data_ptr(), flen, 0, nbb, W, o1.data_ptr(), None,
                                              n_rows, ctypes.byref(rows)))
            got = o1.view(n_rows, W).to(torch.int64)
            p = torch.arange(n_rows, device=dev)[:, None] + 1 + torch.arange(W, device=dev)[None, :]
            have = p < lines
            ok = bool(torch.equal(got[have], band_b[:n_rows][have].round().to(torch.int64)))
            print(json.dumps({"tool": "ld_rate", "device": name, "shape": "%dx%d" % (N, S), "haps": N, "sites": S,
                              "blocks": n_blocks, "window": W, "ld_ms": ms_ld, "ld_stage_ms": stage_ms,
                              "ld_stage_pair_bits_per_s": pair_bits / (stage_ms * 1e-3) if stage_ms > 0 else None,
                              "ld_stage_kernel_share_of_i8_mfma_peak":
                                  pair_bits / (stage_ms * 1e-3) / I8_MFMA_MACS if stage_ms > 0 else None,
                              "decode_dot_k1_ms": ms_dot, "ld_over_decode_dot": ms_ld / ms_dot,
                              "baseline_packed_torch_ms": ms_base, "baseline_blocks_timed": nbb,
                              "ld_speedup_over_baseline": ms_base / ms_ld, "matches_baseline": ok}), flush=True)
            del n11, r2, band_b, o1, got, p, have
            torch.cuda.empty_cache()
        del d_file, rows_buf
        torch.cuda.empty_cache()


def stage_run(ctx, torch, fn):
    """One call with the context's stage timing on: {stage: ms}."""
    ctx.set_timing(True)
    fn()
    torch.cuda.synchronize()
    st = ctx.timing()
    ctx.set_timing(False)
    return {k: v[0] for k, v in st.items() if v[1]}


def general_file(L, binding, ctx, torch, dev, d_bits, stride, N, S, missing, multi, seed=5, block_len=8192):
    """The bench bits as int32 rows with missing values and tri-allelic lines -> xsi_hip_encode_gt -> a file image.
    Returns (d_file, file_len, n_blocks, allele numbers)."""
    import numpy as np
    n = N // 2
    thr = int(N * 0.001)
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    d_gt = torch.empty((S, N), dtype=torch.int32, device=dev)
    shifts = torch.arange(8, device=dev, dtype=torch.uint8)
    odd = (torch.arange(N, device=dev) & 1).to(torch.int32)
    tri = torch.rand(S, generator=g, device=dev) < multi
    for r0 in range(0, S, 4096):
        rows = d_bits[r0 * stride:(r0 + 4096) * stride].view(-1, stride)
        m = rows.shape[0]
        al = ((rows.unsqueeze(-1) >> shifts) & 1).reshape(m, -1)[:, :N].to(torch.int32)
        # tri-allelic lines: 2 % of the haplotypes carry ALT 2
        al = torch.where(tri[r0:r0 + m, None] & (torch.rand((m, N), generator=g, device=dev) < 0.02), 2, al)
        gt = ((al + 1) << 1) | odd
        gt = torch.where(torch.rand((m, N), generator=g, device=dev) < missing, odd, gt)  # missing, phase bit kept
        d_gt[r0:r0 + m] = gt
        del rows, al, gt
    nal = np.where(tri.cpu().numpy(), 3, 2).astype(np.uint32)
    ngt = np.full(S, N, dtype=np.uint32)
    p = binding.EncodeParams(n, block_len, thr, 1, 0, 0)
    cap = int(L.xsi_hip_encode_gt_bound(ctypes.byref(p), S, S))
    n_blocks = (S + block_len - 1) // block_len
    d_file = torch.empty(cap + 256 + 8 * n_blocks + 64, dtype=torch.uint8, device=dev)
    d_off = torch.zeros(n_blocks, dtype=torch.int64, device=dev)
    res = binding.EncodeResult()
    binding.check(L.xsi_hip_encode_gt(ctx.handle, ctypes.byref(p), d_gt.data_ptr(), N, S, ngt.ctypes.data,
                                      nal.ctypes.data, d_file[256:].data_ptr(), cap, d_off.data_ptr(), ctypes.byref(res)))
    torch.cuda.synchronize()
    del d_gt
    nb = res.blocks_bytes
    io = 256 + nb + (-(256 + nb)) % 8
    so = io + 8 * n_blocks
    hf = binding.HeaderFields(n, 2, block_len, thr, 1, 0, int((nal - 1).sum()), S, io, so)
    hdr = (ctypes.c_uint8 * 256)()
    binding.check(L.xsi_hip_make_header(ctypes.byref(hf), hdr))
    d_file[:256] = torch.frombuffer(bytearray(hdr), dtype=torch.uint8).to(dev)
    d_file[256 + nb:io] = 0
    d_file[io:so] = d_off.view(torch.uint8)
    torch.cuda.empty_cache()
    return d_file, so, n_blocks, nal


def main_gt(args):
    import numpy as np
    import torch
    from xsqueezeit_amd import binding, synth
    L = binding.lib()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    ctx = binding.Context(0, stream.cuda_stream)
    windows = [int(w) for w in args.windows.split(",")]
    name = torch.cuda.get_device_name(0)
    rows = ctypes.c_uint64(0)
    for shape in args.shapes.split(","):
        N, S = (int(x) for x in shape.split("x"))
        # 1. the bench file: every value called, bi-allelic
        d_file, flen, n_blocks, d_bits, stride = build_file(L, binding, synth, ctx, torch, dev, N, S)
        nal2 = np.full(S, 2, dtype=np.uint32)
        clean = {}
        for W in windows:
            n11 = torch.empty(S * W, dtype=torch.int32, device=dev)
            r2 = torch.empty(S * W, dtype=torch.float32, device=dev)
            ncl = torch.empty(S * W, dtype=torch.int32, device=dev)

            def ld():
                binding.check(L.xsi_hip_decode_ld(ctx.handle, d_file.data_ptr(), flen, 0, n_blocks, W, n11.data_ptr(),
                                                  r2.data_ptr(), S, ctypes.byref(rows)))

            def ldg():
                binding.check(L.xsi_hip_decode_ld_gt(ctx.handle, d_file.data_ptr(), flen, 0, n_blocks,
                                                     nal2.ctypes.data, S, W, n11.data_ptr(), r2.data_ptr(),
                                                     ncl.data_ptr(), S, ctypes.byref(rows)))
            ms_ld, ms_ldg = timed(ld, args.reps), timed(ldg, args.reps)
            st_ld, st_ldg = stage_run(ctx, torch, ld), stage_run(ctx, torch, ldg)
            clean[W] = (ms_ld, ms_ldg, st_ld.get("ld", 0.0), st_ldg.get("ld", 0.0), st_ldg.get("gt_unpack", 0.0))
            del n11, r2, ncl
            torch.cuda.empty_cache()
        del d_file
        torch.cuda.empty_cache()
        # 2. the general file from the same bits
        d_file, flen, n_blocks, nal = general_file(L, binding, ctx, torch, dev, d_bits, stride, N, S, args.missing,
                                                   args.multi)
        del d_bits
        torch.cuda.empty_cache()
        n_bin = int((nal - 1).sum())
        bin_parent = torch.from_numpy(np.repeat(np.arange(S), nal - 1)).to(dev)
        bin_alt = torch.from_numpy(np.concatenate([np.arange(1, a) for a in nal]).astype(np.int32)).to(dev)
        nbb = min(args.baseline_blocks, n_blocks)
        nbd = min(nbb + 1, n_blocks)
        gt_buf = torch.empty((nbd * 8192, N), dtype=torch.int32, device=dev)
        for W in windows:
            n11 = torch.empty(n_bin * W, dtype=torch.int32, device=dev)
            r2 = torch.empty(n_bin * W, dtype=torch.float32, device=dev)
            ncl = torch.empty(n_bin * W, dtype=torch.int32, device=dev)

            def ldg():
                binding.check(L.xsi_hip_decode_ld_gt(ctx.handle, d_file.data_ptr(), flen, 0, n_blocks, nal.ctypes.data,
                                                     S, W, n11.data_ptr(), r2.data_ptr(), ncl.data_ptr(), n_bin,
                                                     ctypes.byref(rows)))
            ms_ldg = timed(ldg, args.reps)
            st = stage_run(ctx, torch, ldg)
            band = torch.empty((4, nbb * 8192 * 2, W), dtype=torch.float64, device=dev)

            def baseline():
                nl = min(nbd * 8192, S)
                binding.check(L.xsi_hip_decode_gt(ctx.handle, d_file.data_ptr(), flen, 0, nbd, nal.ctypes.data, nl,
                                                  gt_buf.data_ptr(), N, None, None, 0))
                b_lines = int((nal[:nl] - 1).sum())
                n_rows = int((nal[:min(nbb * 8192, S)] - 1).sum())
                for r0 in range(0, n_rows, 1024):
                    r1 = min(r0 + 1024, n_rows)
                    c1 = min(r1 + W, b_lines)
                    al = (gt_buf[bin_parent[r0:c1]] >> 1) - 1
                    X = (al == bin_alt[r0:c1, None]).to(torch.float64)
                    C = (al >= 0).to(torch.float64)
                    for q, (A_, B_) in enumerate(((X, X), (X, C), (C, X), (C, C))):
                        G = A_[:r1 - r0] @ B_[1:].T
                        if G.shape[1] < (r1 - r0 - 1) + W:
                            G = torch.nn.functional.pad(G, (0, (r1 - r0 - 1) + W - G.shape[1]), value=-1.0)
                        band[q, r0:r1] = G.as_strided((r1 - r0, W), (G.stride(0) + 1, 1))
                return n_rows, b_lines
            ms_base_part = timed(baseline, 1)
            n_rows, b_lines = baseline()
            torch.cuda.synchronize()
            ms_base = ms_base_part * n_blocks / nbb
            p = torch.arange(n_rows, device=dev)[:, None] + 1 + torch.arange(W, device=dev)[None, :]
            have = p < b_lines
            ok = bool(torch.equal(n11.view(n_bin, W)[:n_rows].to(torch.int64)[have], band[0, :n_rows][have].round().to(torch.int64))
                      and torch.equal(ncl.view(n_bin, W)[:n_rows].to(torch.int64)[have], band[3, :n_rows][have].round().to(torch.int64)))
            ms_ld, ms_ldg_clean, ld_stage, ldg_stage_clean, unpack_clean = clean[W]
            ldg_stage = st.get("ld", 0.0)
            print(json.dumps({"tool": "ld_rate", "mode": "gt", "device": name, "shape": "%dx%d" % (N, S), "haps": N,
                              "sites": S, "blocks": n_blocks, "window": W,
                              "all_called": {"decode_ld_ms": ms_ld, "decode_ld_stage_ld_ms": ld_stage,
                                             "decode_ld_gt_ms": ms_ldg_clean, "decode_ld_gt_stage_ld_ms": ldg_stage_clean,
                                             "decode_ld_gt_stage_gt_unpack_ms": unpack_clean,
                                             "stage_ld_ratio": ldg_stage_clean / ld_stage if ld_stage else None},
                              "general": {"missing": args.missing, "multi": args.multi, "binary_lines": n_bin,
                                          "decode_ld_gt_ms": ms_ldg, "stage_ld_ms": ldg_stage,
                                          "stage_gt_unpack_ms": st.get("gt_unpack", 0.0),
                                          "stage_gt_compose_ms": st.get("gt_compose", 0.0),
                                          "stage_ld_over_all_called": ldg_stage / ldg_stage_clean if ldg_stage_clean else None},
                              "baseline_decode_gt_torch_ms": ms_base, "baseline_blocks_timed": nbb,
                              "speedup_over_baseline": ms_base / ms_ldg, "matches_baseline": ok}), flush=True)
            del n11, r2, ncl, band, p, have
            torch.cuda.empty_cache()
        del d_file, gt_buf
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
