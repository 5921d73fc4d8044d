#!/usr/bin/env python3
"""Rate of xsi_hip_decode_score (weighted genotype scores, X^T.W on decoded blocks) on the bench generator's matrix,
against xsi_hip_decode_dot (X.Y) on the same file and K, and against the route a caller has without it:
xsi_hip_decode_packed one block at a time -> unpack to float64 in torch -> torch.matmul.  Prints one JSON line."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build_file(L, binding, synth, ctx, torch, dev, N, S, block_len=8192):
    n = N // 2
    thr = int(N * 0.001)
    stride = synth.row_stride_bytes(N)
    p = binding.EncodeParams(n, block_len, thr, 1, 0, 0)
    n_blocks = (S + block_len - 1) // block_len
    d_bits = torch.empty(S * stride, dtype=torch.uint8, device=dev)
    binding.check(L.xsi_hip_synth_packed(ctx.handle, 42, 0, S, N, d_bits.data_ptr(), stride))
    cap = int(L.xsi_hip_encode_bound(ctypes.byref(p), S, S))
    d_file = torch.empty(256 + cap + 8 * n_blocks + 64, dtype=torch.uint8, device=dev)
    d_off = torch.zeros(n_blocks, dtype=torch.int64, device=dev)
    res = binding.EncodeResult()
    binding.check(L.xsi_hip_encode_packed(ctx.handle, ctypes.byref(p), d_bits.data_ptr(), S, stride,
                                          d_file[256:].data_ptr(), cap, d_off.data_ptr(), ctypes.byref(res)))
    nb = res.blocks_bytes
    io = 256 + nb + (-(256 + nb)) % 8
    so = io + 8 * n_blocks
    hf = binding.HeaderFields(n, 2, block_len, thr, 1, 0, S, S, io, so)
    hdr = (ctypes.c_uint8 * 256)()
    binding.check(L.xsi_hip_make_header(ctypes.byref(hf), hdr))
    d_file[:256] = torch.frombuffer(bytearray(hdr), dtype=torch.uint8).to(dev)
    d_file[256 + nb:io] = 0
    d_file[io:so] = d_off.view(torch.uint8)
    return d_file, so, n_blocks, d_bits, stride


def timed(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="5008x1000000,64976x262144", help="comma-separated HAPSxSITES")
    ap.add_argument("--ks", default="1,4,16,64")
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
    ks = [int(k) for k in args.ks.split(",")]
    result = {"tool": "score_rate", "device": torch.cuda.get_device_name(0), "shapes": []}
    for shape in args.shapes.split(","):
        N, S = (int(x) for x in shape.split("x"))
        n = N // 2
        d_file, flen, n_blocks, d_bits, stride = build_file(L, binding, synth, ctx, torch, dev, N, S)
        del d_bits
        torch.cuda.empty_cache()
        plane_bytes = 4.0 * ((N + 63) // 64) * 2 * S  # the planes the contraction reads (one per binary line)
        entry = {"haps": N, "sites": S, "blocks": n_blocks, "plane_bytes": plane_bytes, "k": []}
        for K in ks:
            w = torch.randn((S, K), dtype=torch.float64, device=dev)
            out = torch.zeros((n, K), dtype=torch.float64, device=dev)
            y = torch.randn((n, K), dtype=torch.float64, device=dev)
            dout = torch.zeros((S, K), dtype=torch.float64, device=dev)

            def score():
                binding.check(L.xsi_hip_decode_score(ctx.handle, d_file.data_ptr(), flen, 0, n_blocks, w.data_ptr(), S, K,
                                                     out.data_ptr(), n, 0))

            def dot():
                binding.check(L.xsi_hip_decode_dot(ctx.handle, d_file.data_ptr(), flen, 0, n_blocks, y.data_ptr(), K,
                                                   dout.data_ptr(), S, None))
            ms_score = timed(score, args.reps)
            ms_dot = timed(dot, args.reps)
            ctx.set_timing(True)
            score()
            torch.cuda.synchronize()
            st = ctx.timing()
            ctx.set_timing(False)
            stage_ms = st.get("score", (0.0, 0))[0]
            # baseline: decode_packed one block at a time, unpack to float64, torch.matmul
            nbb = min(args.baseline_blocks, n_blocks)
            rows_buf = torch.empty(8192 * stride, dtype=torch.uint8, device=dev)
            shifts = torch.arange(8, dtype=torch.uint8, device=dev)
            acc = torch.zeros((N, K), dtype=torch.float64, device=dev)
            nrow = ctypes.c_uint64(0)

            def baseline():
                acc.zero_()
                for b in range(nbb):
                    binding.check(L.xsi_hip_decode_packed(ctx.handle, d_file.data_ptr(), flen, b, 1, rows_buf.data_ptr(),
                                                          stride, 8192, ctypes.byref(nrow), None))
                    r = int(nrow.value)
                    rows = rows_buf[:r * stride].view(r, stride)
                    bits = ((rows.unsqueeze(-1) >> shifts) & 1).reshape(r, -1)[:, :N].to(torch.float64)
                    acc.add_(bits.T @ w[b * 8192:b * 8192 + r])
            ms_base_part = timed(baseline, 1)
            ms_base = ms_base_part * n_blocks / nbb
            ok = True
            if K <= 16:  # the score of the first blocks against the baseline's
                o1 = torch.zeros((n, K), dtype=torch.float64, device=dev)
                binding.check(L.xsi_hip_decode_score(ctx.handle, d_file.data_ptr(), flen, 0, nbb, w.data_ptr(),
                                                     min(S, nbb * 8192), K, o1.data_ptr(), n, 0))
                ok = bool(torch.allclose(o1, acc.view(n, 2, K).sum(1), rtol=1e-10, atol=1e-8))
            entry["k"].append({"K": K, "score_ms": ms_score, "dot_ms": ms_dot, "score_over_dot": ms_score / ms_dot,
                               "score_stage_ms": stage_ms,
                               "score_stage_plane_TBps": plane_bytes / (stage_ms * 1e-3) / 1e12 if stage_ms > 0 else None,
                               "baseline_packed_torch_ms": ms_base, "baseline_blocks_timed": nbb,
                               "matches_baseline": ok})
            del w, out, y, dout, rows_buf, acc
            torch.cuda.empty_cache()
        result["shapes"].append(entry)
        del d_file
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
