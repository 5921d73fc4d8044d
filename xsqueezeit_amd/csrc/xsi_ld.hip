// xsi_ld.hip — windowed haplotype linkage disequilibrium on the decoded blocks: the banded part of X.X^T.
// n11[r][j] = haplotypes carrying the ALT allele of binary line r and of line r + 1 + j (0 <= j < window), and
// r2[r][j] from n11 and the two lines' ALT counts, for LD pruning, clumping, LD-score regression and fine-mapping.
//
// Data path: ALT-carrier bit planes of a range of blocks plus the look-ahead lines after it (decode_planes with the
// negation applied) -> k_ld_prep: one haplotype-order plane per line (a fully haploid line's sample s spread to
// haplotype 2s, bits past N cleared, padded to whole LD_KC-word chunks) and its ALT count -> k_ld_popc: the band of
// pair counts by v_and + v_bcnt, r2 in float64 from the exact integers.  Everything is integer up to the one r2
// formula, so the output is the same bits for any workspace budget and any split of the block range.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "../../include/xsi_hip.h"
#include "xsi_ctx.hpp"
#include "xsi_device.hpp"
#include "xsi_kernels.hpp"

using namespace xsi;

#define HIP_TRY(expr)                                                                                        \
    do {                                                                                                     \
        hipError_t _e = (expr);                                                                              \
        if (_e != hipSuccess) return set_error(XSI_ERR_HIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                                               __FILE__, __LINE__);                                          \
    } while (0)
#define WS(ptr, name, bytes)                          \
    do {                                              \
        void* _p;                                     \
        int _rc = ws_ensure(ctx, name, (bytes), &_p); \
        if (_rc) return _rc;                          \
        ptr = reinterpret_cast<decltype(ptr)>(_p);    \
    } while (0)

namespace xsi {

constexpr uint32_t LD_T = 64;   // lines per tile side: a workgroup owns 64 row lines x 64 partner lines
constexpr uint32_t LD_KC = 32;  // plane words per LDS chunk (1024 haplotypes); the prepared planes are whole chunks

// One workgroup per line of the range: plane -> haplotype-order plane of kw words, ALT count.  A fully haploid line
// holds compact sample bits (bit s = sample s); word w of its haplotype plane takes the 16 samples of half (w & 1) of
// compact word w / 2, sample i of them to bit 2i.  Bits at N and above (the plane stride's padding, the complement of a
// negated line) are cleared, so they never count.
__global__ void __launch_bounds__(256) k_ld_prep(const uint32_t* __restrict__ planes, uint32_t stride_w,
                                                 const uint8_t* __restrict__ kind, uint32_t N, uint32_t n_samples,
                                                 uint32_t kw, uint32_t* __restrict__ bits, uint32_t* __restrict__ cnt) {
    __shared__ uint32_t part[4];
    const uint32_t l = blockIdx.x, tid = threadIdx.x;
    const bool hap = (kind[l] & KIND_HAPLOID) != 0u;
    const uint32_t* src = planes + (size_t)l * stride_w;
    uint32_t* dst = bits + (size_t)l * kw;
    uint32_t ones = 0;
    for (uint32_t w = tid; w < kw; w += 256u) {
        uint32_t v = 0;
        if (hap) {
            const uint32_t cw = w >> 1, s0 = 32u * cw + 16u * (w & 1u);
            if (cw < stride_w && s0 < n_samples) {
                uint32_t h = (src[cw] >> (16u * (w & 1u))) & 0xFFFFu;
                if (n_samples - s0 < 16u) h &= (1u << (n_samples - s0)) - 1u;
                h = (h | (h << 8)) & 0x00FF00FFu;  // bit i -> bit 2i
                h = (h | (h << 4)) & 0x0F0F0F0Fu;
                h = (h | (h << 2)) & 0x33333333u;
                h = (h | (h << 1)) & 0x55555555u;
                v = h;
            }
        } else if (w < stride_w && 32u * w < N) {
            v = src[w];
            if (N - 32u * w < 32u) v &= (1u << (N - 32u * w)) - 1u;
        }
        dst[w] = v;
        ones += (uint32_t)__popc(v);
    }
    for (int o = 32; o > 0; o >>= 1) ones += (uint32_t)__shfl_xor((int)ones, o, 64);
    if ((tid & 63u) == 0u) part[tid >> 6] = ones;
    __syncthreads();
    if (tid == 0) cnt[l] = part[0] + part[1] + part[2] + part[3];
}

// v_bcnt_u32_b32 with its accumulator operand: one instruction per pair and word.  Written as popc + add, the compiler
// emits v_bcnt with 0 and sums pairs of counts with v_add3_u32, half an instruction more per pair and word.
__device__ __forceinline__ uint32_t bcnt_add(uint32_t x, uint32_t acc) {
    uint32_t r;
    asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(acc));
    return r;
}

struct LdArgs {
    const uint32_t* bits;  // [n_avail][kw] prepared planes, range-relative lines
    const uint32_t* cnt;   // [n_avail] ALT counts
    uint32_t kw, N, window;
    uint32_t n_rows;       // lines of the range that get output rows
    uint32_t n_avail;      // lines held (range + look-ahead); a partner at or past it lies past the file's last line
    uint32_t* n11;         // [n_rows][window] or null
    float* r2;             // [n_rows][window] or null
};

// Band tile: workgroup (x, y) takes row lines [i0, i0 + 64), i0 = 64 x, and partner lines [c0, c0 + 64),
// c0 = i0 + 1 + 64 y: the partners of the tile's rows span i0 + 1 .. i0 + 63 + window, ceil((63 + window) / 64) tiles.
// Per chunk of LD_KC words both sides go to LDS word-major ([k][line]); thread (ty, tx) = (tid >> 4, tid & 15) owns rows
// 4 ty .. 4 ty + 3 and partners 4 tx .. 4 tx + 3, and per word reads one 16-byte row quad (the 16 lanes of a row share it)
// and one partner quad: 16 v_and + 16 v_bcnt (accumulating) per two LDS reads.  Pairs outside the band (j < 0 or j >= window) are
// computed and dropped, rows at or past n_rows are not written.
__global__ void __launch_bounds__(256) k_ld_popc(LdArgs A) {
    __shared__ __attribute__((aligned(16))) uint32_t sr[LD_KC][LD_T];
    __shared__ __attribute__((aligned(16))) uint32_t sc[LD_KC][LD_T];
    const uint32_t tid = threadIdx.x, tx = tid & 15u, ty = tid >> 4;
    const uint32_t i0 = blockIdx.x * LD_T, c0 = i0 + 1u + blockIdx.y * LD_T;
    uint32_t acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0u;
    if (c0 < A.n_avail) {  // a tile wholly past the file's end only writes sentinels
        for (uint32_t k0 = 0; k0 < A.kw; k0 += LD_KC) {
            // 64 lines x 8 quads a side, two per thread: lane -> line, so the LDS stores of a wave hit 64 banks
#pragma unroll
            for (uint32_t h = 0; h < 2u; ++h) {
                const uint32_t q = tid + 256u * h, line = q & (LD_T - 1u), u = q >> 6;
                uint4 rv = make_uint4(0u, 0u, 0u, 0u), cv = make_uint4(0u, 0u, 0u, 0u);
                if (i0 + line < A.n_avail) rv = *reinterpret_cast<const uint4*>(A.bits + (size_t)(i0 + line) * A.kw + k0 + 4u * u);
                if (c0 + line < A.n_avail) cv = *reinterpret_cast<const uint4*>(A.bits + (size_t)(c0 + line) * A.kw + k0 + 4u * u);
                sr[4u * u + 0u][line] = rv.x;
                sr[4u * u + 1u][line] = rv.y;
                sr[4u * u + 2u][line] = rv.z;
                sr[4u * u + 3u][line] = rv.w;
                sc[4u * u + 0u][line] = cv.x;
                sc[4u * u + 1u][line] = cv.y;
                sc[4u * u + 2u][line] = cv.z;
                sc[4u * u + 3u][line] = cv.w;
            }
            __syncthreads();
#pragma unroll 8
            for (uint32_t k = 0; k < LD_KC; ++k) {
                const uint4 rq = *reinterpret_cast<const uint4*>(&sr[k][4u * ty]);
                const uint4 cq = *reinterpret_cast<const uint4*>(&sc[k][4u * tx]);
                const uint32_t rw[4] = {rq.x, rq.y, rq.z, rq.w}, cw[4] = {cq.x, cq.y, cq.z, cq.w};
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b) acc[a][b] = bcnt_add(rw[a] & cw[b], acc[a][b]);
            }
            __syncthreads();
        }
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const uint32_t r = i0 + 4u * ty + (uint32_t)a;
        if (r >= A.n_rows) continue;
        const uint32_t ni = A.cnt[r];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const uint32_t c = c0 + 4u * tx + (uint32_t)b;
            if (c <= r || c - r - 1u >= A.window) continue;
            const size_t e = (size_t)r * A.window + (c - r - 1u);
            if (c >= A.n_avail) {
                if (A.n11) A.n11[e] = 0xFFFFFFFFu;
                if (A.r2) A.r2[e] = __builtin_nanf("");
                continue;
            }
            const uint32_t n11 = acc[a][b];
            if (A.n11) A.n11[e] = n11;
            if (A.r2) {
                // one correctly rounded operation per step, in the order of the header: numpy gives the same bits
                const uint32_t nj = A.cnt[c];
                const double num = (double)((int64_t)A.N * n11 - (int64_t)ni * nj);
                const double den = (double)((int64_t)ni * (A.N - ni)) * (double)((int64_t)nj * (A.N - nj));
                A.r2[e] = den == 0.0 ? __builtin_nanf("") : (float)(num * num / den);
            }
        }
    }
}

// The plane path's coverage (as decode_dot / decode_score): bi-allelic, fully called lines only.
static int ld_block_ok(const DecBlock& b, uint64_t block, bool lookahead) {
    if (b.n_bin != b.n_bcf || b.off_line_missing != VAL_UNDEFINED || b.off_line_eov != VAL_UNDEFINED)
        return set_error(XSI_ERR_UNSUPPORTED, "decode_ld: %sblock %llu has multi-allelic lines or missing / end-of-vector entries; "
                         "LD on the ALT-carrier planes covers bi-allelic, fully called lines only",
                         lookahead ? "look-ahead " : "", (unsigned long long)block);
    return XSI_OK;
}

}  // namespace xsi

extern "C" {

int xsi_hip_decode_ld(xsi_hip_ctx* ctx, const void* d_file, uint64_t file_len, uint64_t first_block, uint64_t n_blocks,
                      uint32_t window, uint32_t* d_n11, float* d_r2, uint64_t capacity_lines, uint64_t* h_n_bin) {
    if (!ctx || !d_file) return set_error(XSI_ERR_ARG, "decode_ld: null argument");
    if (!d_n11 && !d_r2) return set_error(XSI_ERR_ARG, "decode_ld: both outputs are null");
    if (!window || window > XSI_LD_MAX_WINDOW)
        return set_error(XSI_ERR_ARG, "decode_ld: window %u outside 1 .. %u", window, (unsigned)XSI_LD_MAX_WINDOW);
    if (file_len < 256) return set_error(XSI_ERR_FORMAT, "file image shorter than the 256-byte header");
    HIP_TRY(hipSetDevice(ctx->device));
    DecodePlan P;
    int rc = decode_prepare(ctx, d_file, file_len, first_block, n_blocks, &P, /*counts_only=*/true);
    if (rc) return rc;
    for (uint32_t b = 0; b < P.n_blocks; ++b)
        if ((rc = ld_block_ok(P.blocks_h[b], first_block + b, false))) return rc;
    if (h_n_bin) *h_n_bin = P.n_bin;
    if (P.n_bin > capacity_lines)
        return set_error(XSI_ERR_CAPACITY, "decode_ld: %u binary lines, capacity %llu", P.n_bin, (unsigned long long)capacity_lines);
    // binary lines of every block the call may read: the requested ones, then the look-ahead blocks after them, as many
    // as hold `window` lines, never past the file's last block (counted 1, 2, 4, ... blocks at a time)
    std::vector<uint32_t> bins(P.n_blocks);
    for (uint32_t b = 0; b < P.n_blocks; ++b) bins[b] = P.blocks_h[b].n_bin;
    const uint64_t file_blocks = P.file_blocks;
    {
        uint64_t next = first_block + n_blocks, lines = 0, chunk = 1;
        while (lines < window && next < file_blocks) {
            const uint64_t nb = std::min<uint64_t>(chunk, std::min<uint64_t>(file_blocks - next, 0xFFFFFFull));
            DecodePlan Q;
            if ((rc = decode_prepare(ctx, d_file, file_len, next, nb, &Q, /*counts_only=*/true))) return rc;
            for (uint32_t b = 0; b < Q.n_blocks && lines < window; ++b, ++next) {
                if ((rc = ld_block_ok(Q.blocks_h[b], next, true))) return rc;
                bins.push_back(Q.blocks_h[b].n_bin);
                lines += Q.blocks_h[b].n_bin;
            }
            chunk *= 2;
        }
    }
    if (!P.n_bin) return XSI_OK;
    const uint32_t N = P.L.N, stride_w = P.L.y_stride64 * 2u;
    const uint32_t kw = (((N + 31u) / 32u) + LD_KC - 1u) / LD_KC * LD_KC;
    // per binary line: its plane, the decode's expanded WAH row, the prepared plane and its count; the look-ahead lines
    // of a range come on top (decoded again for every range: at most `window` lines more)
    const auto cuts = score_ranges(P, ws_budget_now(ctx) / 2, 0, 4ull * (2ull * stride_w + kw + 1u), 0);
    uint64_t row0 = 0;
    for (size_t c = 0; c + 1 < cuts.size(); ++c) {
        uint32_t rows = 0;
        for (uint32_t b = cuts[c]; b < cuts[c + 1]; ++b) rows += bins[b];
        size_t ext = cuts[c + 1];
        uint64_t more = 0;
        while (more < window && ext < bins.size()) more += bins[ext++];
        if (!rows) continue;  // blocks without binary lines: no rows, nothing to decode
        DecodePlan R;
        if ((rc = decode_prepare(ctx, d_file, file_len, first_block + cuts[c], ext - cuts[c], &R))) return rc;
        if ((uint64_t)R.n_bin != rows + more) return set_error(XSI_ERR_FORMAT, "decode_ld: block line counts changed between reads");
        uint32_t *planes, *bits, *cnt;
        WS(planes, "ld.planes", 4ull * stride_w * R.n_bin);
        WS(bits, "ld.bits", 4ull * kw * R.n_bin);
        WS(cnt, "ld.cnt", 4ull * R.n_bin + 64);
        if ((rc = decode_planes(ctx, d_file, R, planes, stride_w, /*apply_negation=*/1))) return rc;
        stage_mark(ctx, XSI_ST_LD);
        k_ld_prep<<<dim3(R.n_bin), dim3(256), 0, ctx->stream>>>(planes, stride_w, R.L.kind, N, R.L.n_samples, kw, bits, cnt);
        HIP_TRY(hipGetLastError());
        LdArgs A{bits, cnt, kw, N, window, rows, R.n_bin, d_n11 ? d_n11 + row0 * window : nullptr,
                 d_r2 ? d_r2 + row0 * window : nullptr};
        const dim3 grid((rows + LD_T - 1u) / LD_T, (LD_T - 1u + window + LD_T - 1u) / LD_T);
        k_ld_popc<<<grid, dim3(256), 0, ctx->stream>>>(A);
        HIP_TRY(hipGetLastError());
        stage_mark(ctx, -1);
        row0 += rows;
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    stage_collect(ctx);
    return XSI_OK;
}

}  // extern "C"
