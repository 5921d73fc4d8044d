#!/usr/bin/env python3
"""Rate of xsi_hip_decode_ld (windowed haplotype LD: pair counts and r2 on the decoded blocks) on the bench generator's
matrix, against xsi_hip_decode_dot at K = 1 on the same file (the cost of decoding the planes) and against the route a
caller has without it: xsi_hip_decode_packed one block at a time -> unpack to float64 in torch -> banded matmul.
Prints one JSON line per shape and window."""
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
    args = ap.parse_args()
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


if __name__ == "__main__":
    main()
