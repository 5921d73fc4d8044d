// xsi_ld.hip — windowed haplotype linkage disequilibrium on the decoded blocks: the banded part of X.X^T.
// n11[r][j] = haplotypes carrying the ALT allele of binary line r and of line r + 1 + j (0 <= j < window), and
// r2[r][j] from n11 and the two lines' ALT counts, for LD pruning, clumping, LD-score regression and fine-mapping.
//
// Data path: ALT-carrier bit planes of a range of blocks plus the look-ahead lines after it (decode_planes with the
// negation applied) -> k_ld_prep: one haplotype-order plane per line (a fully haploid line's sample s spread to
// haplotype 2s, bits past N cleared, padded to whole LD_KC-word chunks) and its ALT count -> k_ld_popc: the band of
// pair counts by v_and + v_bcnt, r2 in float64 from the exact integers.  Everything is integer up to the one r2
// formula, so the output is the same bits for any workspace budget and any split of the block range.
//
// General path (xsi_hip_decode_ld_gt, any block): int32 rows composed in HBM (decode_all_planes + compose_lines, as
// decode_score_gt) -> k_ld_gt_prep: per binary line a carrier plane and a called plane of k_ld_prep's layout, its
// carrier and called counts and a "fully called" flag -> per 64 x 64 tile one of two pair kernels: k_ld_popc<true> on
// tiles whose lines are all fully called (n11 alone, exactly decode_ld's form), k_ld_popc4 on the others (n11, a, b and
// n_called over the haplotypes called on both lines, r2 from those).
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
    // general path only (null for decode_ld)
    const uint32_t* called;  // [n_avail][kw] called planes
    const uint8_t* full;     // [n_avail] 1: every haplotype of the line is called
    uint32_t* n_called;      // [n_rows][window] or null
};

// General path: are the tile's 64 row lines and 64 partner lines all fully called?  Lines past the file's end count as
// such (they only get sentinels).  Both pair kernels ask, each takes the tiles the other leaves.
__device__ __forceinline__ bool ld_tile_clean(const LdArgs& A, uint32_t i0, uint32_t c0) {
    const uint32_t tid = threadIdx.x, l = (tid < LD_T ? i0 : c0) + (tid & (LD_T - 1u));
    return __syncthreads_and(tid >= 2u * LD_T || l >= A.n_avail || A.full[l] != 0u) != 0;
}

// Band tile: workgroup (x, y) takes row lines [i0, i0 + 64), i0 = 64 x, and partner lines [c0, c0 + 64),
// c0 = i0 + 1 + 64 y: the partners of the tile's rows span i0 + 1 .. i0 + 63 + window, ceil((63 + window) / 64) tiles.
// Per chunk of LD_KC words both sides go to LDS word-major ([k][line]); thread (ty, tx) = (tid >> 4, tid & 15) owns rows
// 4 ty .. 4 ty + 3 and partners 4 tx .. 4 tx + 3, and per word reads one 16-byte row quad (the 16 lanes of a row share it)
// and one partner quad: 16 v_and + 16 v_bcnt (accumulating) per two LDS reads.  Pairs outside the band (j < 0 or j >= window) are
// computed and dropped, rows at or past n_rows are not written.
// GT (general path): only fully called tiles, where a = n_i, b = n_j and n_called = N; others are left to k_ld_popc4.
template <bool GT>
__global__ void __launch_bounds__(256) k_ld_popc(LdArgs A) {
    __shared__ __attribute__((aligned(16))) uint32_t sr[LD_KC][LD_T];
    __shared__ __attribute__((aligned(16))) uint32_t sc[LD_KC][LD_T];
    const uint32_t tid = threadIdx.x, tx = tid & 15u, ty = tid >> 4;
    const uint32_t i0 = blockIdx.x * LD_T, c0 = i0 + 1u + blockIdx.y * LD_T;
    if (GT && !ld_tile_clean(A, i0, c0)) return;
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
                if (GT && A.n_called) A.n_called[e] = 0xFFFFFFFFu;
                continue;
            }
            const uint32_t n11 = acc[a][b];
            if (A.n11) A.n11[e] = n11;
            if (GT && A.n_called) A.n_called[e] = A.N;
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

// General path, one workgroup per binary line l (BCF line parent[l], ALT alt[l]): its int32 row -> carrier plane (value's
// allele == alt) and called plane (value neither missing nor end-of-vector) of kw words in haplotype order, as k_ld_prep
// lays them out: a fully haploid line's sample s at haplotype 2s, whose partner 2s + 1 carries nothing and has the call
// status of 2s; bits at N and above and the padding words cleared.  Every wave turns 64 values into plane words by a
// ballot: 2 words of a diploid line, 4 of a haploid one (16 samples each, spread to the even bits).  Also writes the
// carrier count, the called count and full[l] = (called count == N).
__global__ void __launch_bounds__(256) k_ld_gt_prep(const int32_t* __restrict__ rows, uint64_t row_stride,
                                                    const uint32_t* __restrict__ line_ngt,
                                                    const uint32_t* __restrict__ bin_parent,
                                                    const uint32_t* __restrict__ bin_alt, uint32_t N, uint32_t n_samples,
                                                    uint32_t kw, uint32_t* __restrict__ bits, uint32_t* __restrict__ called,
                                                    uint32_t* __restrict__ cnt, uint32_t* __restrict__ ccnt,
                                                    uint8_t* __restrict__ full) {
    __shared__ uint32_t part[2][4];
    const uint32_t l = blockIdx.x, lane = lane_id(), wv = threadIdx.x >> 6;
    const uint32_t parent = bin_parent[l];
    const int32_t alt = (int32_t)bin_alt[l];
    const uint32_t nv = line_ngt[parent];
    const bool hap = nv == n_samples;
    const int32_t* row = rows + (size_t)parent * row_stride;
    uint32_t* dx = bits + (size_t)l * kw;
    uint32_t* dc = called + (size_t)l * kw;
    uint32_t ones = 0, calls = 0;
    const uint32_t per = hap ? 4u : 2u;  // plane words per 64 values
    for (uint32_t c = wv; per * c < kw; c += 4u) {
        const uint32_t idx = c * 64u + lane;
        const int32_t al = idx < nv ? (row[idx] >> 1) - 1 : -1;  // missing: -1, end-of-vector: far below
        const uint64_t mx = __ballot(idx < nv && al == alt), mc = __ballot(al >= 0);
        ones += (uint32_t)__popcll(mx);
        calls += (uint32_t)__popcll(mc) * (hap ? 2u : 1u);
        if (!hap) {
            if (lane < 2u) {
                dx[2u * c + lane] = (uint32_t)(mx >> (32u * lane));
                dc[2u * c + lane] = (uint32_t)(mc >> (32u * lane));
            }
        } else if (lane < 4u) {
            auto spread = [](uint32_t h) {  // bit i -> bit 2i
                h = (h | (h << 8)) & 0x00FF00FFu;
                h = (h | (h << 4)) & 0x0F0F0F0Fu;
                h = (h | (h << 2)) & 0x33333333u;
                return (h | (h << 1)) & 0x55555555u;
            };
            const uint32_t hx = spread((uint32_t)(mx >> (16u * lane)) & 0xFFFFu);
            const uint32_t hc = spread((uint32_t)(mc >> (16u * lane)) & 0xFFFFu);
            dx[4u * c + lane] = hx;
            dc[4u * c + lane] = hc | (hc << 1);
        }
    }
    if (lane == 0) {
        part[0][wv] = ones;
        part[1][wv] = calls;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t o = part[0][0] + part[0][1] + part[0][2] + part[0][3];
        const uint32_t k = part[1][0] + part[1][1] + part[1][2] + part[1][3];
        cnt[l] = o;
        ccnt[l] = k;
        full[l] = k == N ? 1u : 0u;
    }
}

// General path, the tiles k_ld_popc<true> leaves: per pair the four counts over the haplotypes called on both lines,
//   n11 = |X_i & X_j|, a = |X_i & C_j|, b = |C_i & X_j|, n_called = |C_i & C_j|,
// 4 v_and + 4 accumulating v_bcnt per pair and word.  Same tiling as k_ld_popc (64 x 64 pairs, 4 x 4 per thread), carrier
// and called words of both sides in LDS (32 KB); r2 is the header's formula with N -> n_called, n_i -> a, n_j -> b.
__global__ void __launch_bounds__(256) k_ld_popc4(LdArgs A) {
    __shared__ __attribute__((aligned(16))) uint32_t sr[2][LD_KC][LD_T];  // [carrier, called][k][line]
    __shared__ __attribute__((aligned(16))) uint32_t sc[2][LD_KC][LD_T];
    const uint32_t tid = threadIdx.x, tx = tid & 15u, ty = tid >> 4;
    const uint32_t i0 = blockIdx.x * LD_T, c0 = i0 + 1u + blockIdx.y * LD_T;
    if (ld_tile_clean(A, i0, c0)) return;
    uint32_t n11[4][4], na[4][4], nb[4][4], nc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) n11[a][b] = na[a][b] = nb[a][b] = nc[a][b] = 0u;
    for (uint32_t k0 = 0; k0 < A.kw; k0 += LD_KC) {
#pragma unroll
        for (uint32_t h = 0; h < 4u; ++h) {
            const uint32_t q = tid + 256u * h, line = q & (LD_T - 1u), u = (q >> 6) & 7u, p = q >> 9;
            const uint32_t* src = p ? A.called : A.bits;
            uint4 rv = make_uint4(0u, 0u, 0u, 0u), cv = make_uint4(0u, 0u, 0u, 0u);
            if (i0 + line < A.n_avail) rv = *reinterpret_cast<const uint4*>(src + (size_t)(i0 + line) * A.kw + k0 + 4u * u);
            if (c0 + line < A.n_avail) cv = *reinterpret_cast<const uint4*>(src + (size_t)(c0 + line) * A.kw + k0 + 4u * u);
            sr[p][4u * u + 0u][line] = rv.x;
            sr[p][4u * u + 1u][line] = rv.y;
            sr[p][4u * u + 2u][line] = rv.z;
            sr[p][4u * u + 3u][line] = rv.w;
            sc[p][4u * u + 0u][line] = cv.x;
            sc[p][4u * u + 1u][line] = cv.y;
            sc[p][4u * u + 2u][line] = cv.z;
            sc[p][4u * u + 3u][line] = cv.w;
        }
        __syncthreads();
#pragma unroll 2
        for (uint32_t k = 0; k < LD_KC; ++k) {
            const uint4 rq = *reinterpret_cast<const uint4*>(&sr[0][k][4u * ty]);
            const uint4 rk = *reinterpret_cast<const uint4*>(&sr[1][k][4u * ty]);
            const uint4 cq = *reinterpret_cast<const uint4*>(&sc[0][k][4u * tx]);
            const uint4 ck = *reinterpret_cast<const uint4*>(&sc[1][k][4u * tx]);
            const uint32_t rx[4] = {rq.x, rq.y, rq.z, rq.w}, rc[4] = {rk.x, rk.y, rk.z, rk.w};
            const uint32_t cx[4] = {cq.x, cq.y, cq.z, cq.w}, cc[4] = {ck.x, ck.y, ck.z, ck.w};
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    n11[a][b] = bcnt_add(rx[a] & cx[b], n11[a][b]);
                    na[a][b] = bcnt_add(rx[a] & cc[b], na[a][b]);
                    nb[a][b] = bcnt_add(rc[a] & cx[b], nb[a][b]);
                    nc[a][b] = bcnt_add(rc[a] & cc[b], nc[a][b]);
                }
        }
        __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const uint32_t r = i0 + 4u * ty + (uint32_t)a;
        if (r >= A.n_rows) continue;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const uint32_t c = c0 + 4u * tx + (uint32_t)b;
            if (c <= r || c - r - 1u >= A.window) continue;
            const size_t e = (size_t)r * A.window + (c - r - 1u);
            if (c >= A.n_avail) {
                if (A.n11) A.n11[e] = 0xFFFFFFFFu;
                if (A.r2) A.r2[e] = __builtin_nanf("");
                if (A.n_called) A.n_called[e] = 0xFFFFFFFFu;
                continue;
            }
            if (A.n11) A.n11[e] = n11[a][b];
            if (A.n_called) A.n_called[e] = nc[a][b];
            if (A.r2) {
                const uint32_t M = nc[a][b], ni = na[a][b], nj = nb[a][b];
                const double num = (double)((int64_t)M * n11[a][b] - (int64_t)ni * nj);
                const double den = (double)((int64_t)ni * (M - ni)) * (double)((int64_t)nj * (M - nj));
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
                 d_r2 ? d_r2 + row0 * window : nullptr, nullptr, nullptr, nullptr};
        const dim3 grid((rows + LD_T - 1u) / LD_T, (LD_T - 1u + window + LD_T - 1u) / LD_T);
        k_ld_popc<false><<<grid, dim3(256), 0, ctx->stream>>>(A);
        HIP_TRY(hipGetLastError());
        stage_mark(ctx, -1);
        row0 += rows;
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    stage_collect(ctx);
    return XSI_OK;
}

}  // extern "C"

namespace xsi {

// One range of the general path: blocks R (requested ones, then look-ahead ones), h_n_allele from R's first BCF line,
// rows = R's binary lines that get output rows.  Int32 rows -> carrier / called planes -> the two pair kernels.
static int ld_gt_range(xsi_hip_ctx* ctx, const void* d_file, DecodePlan& R, const uint32_t* h_n_allele, uint32_t rows,
                       uint32_t window, uint32_t kw, const LdArgs& out) {
    hipStream_t s = ctx->stream;
    const uint32_t n_bcf = R.n_bcf, N = R.L.N;
    std::vector<uint32_t> first_bin(n_bcf), parent(R.n_bin), alt(R.n_bin);
    for (uint32_t l = 0, acc = 0; l < n_bcf; ++l) {  // allele numbers checked against every block by the caller
        first_bin[l] = acc;
        for (uint32_t k = 1; k < h_n_allele[l]; ++k, ++acc) {
            parent[acc] = l;
            alt[acc] = k;
        }
    }
    uint32_t *d_first_bin, *d_nallele, *d_line_ngt, *d_parent, *d_alt, *bits, *called, *cnt, *ccnt;
    uint8_t* full;
    int32_t* d_rows;
    WS(d_first_bin, "gt.bcf_first_bin", 4ull * n_bcf);
    WS(d_nallele, "gt.bcf_nallele", 4ull * n_bcf);
    WS(d_line_ngt, "gt.line_ngt", 4ull * n_bcf);
    WS(d_parent, "dot.bin_parent", 4ull * R.n_bin + 4);
    WS(d_alt, "dot.bin_alt", 4ull * R.n_bin + 4);
    WS(d_rows, "dot.rows", 4ull * N * n_bcf);
    WS(bits, "ld.bits", 4ull * kw * R.n_bin);
    WS(called, "ld.called", 4ull * kw * R.n_bin);
    WS(cnt, "ld.cnt", 4ull * R.n_bin + 64);
    WS(ccnt, "ld.ccnt", 4ull * R.n_bin + 64);
    WS(full, "ld.full", (size_t)R.n_bin + 64);
    HIP_TRY(hipMemcpyAsync(d_first_bin, first_bin.data(), 4ull * n_bcf, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_nallele, h_n_allele, 4ull * n_bcf, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_parent, parent.data(), 4ull * R.n_bin, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_alt, alt.data(), 4ull * R.n_bin, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));  // local vectors: the copies must have left host memory
    DecodedPlanes DPn;
    int rc = decode_all_planes(ctx, d_file, R, &DPn);
    if (rc) return rc;
    rc = compose_lines(ctx, R, DPn, d_first_bin, d_nallele, n_bcf, d_rows, N, d_line_ngt, nullptr, 0);
    if (rc) return rc;
    stage_mark(ctx, XSI_ST_GT_UNPACK);
    k_ld_gt_prep<<<dim3(R.n_bin), dim3(256), 0, s>>>(d_rows, N, d_line_ngt, d_parent, d_alt, N, R.L.n_samples, kw, bits,
                                                     called, cnt, ccnt, full);
    HIP_TRY(hipGetLastError());
    stage_mark(ctx, XSI_ST_LD);
    LdArgs A = out;
    A.bits = bits;
    A.cnt = cnt;
    A.called = called;
    A.full = full;
    A.n_rows = rows;
    A.n_avail = R.n_bin;
    const dim3 grid((rows + LD_T - 1u) / LD_T, (LD_T - 1u + window + LD_T - 1u) / LD_T);
    k_ld_popc<true><<<grid, dim3(256), 0, s>>>(A);
    HIP_TRY(hipGetLastError());
    k_ld_popc4<<<grid, dim3(256), 0, s>>>(A);
    HIP_TRY(hipGetLastError());
    stage_mark(ctx, -1);
    HIP_TRY(hipStreamSynchronize(s));  // the next range reuses the workspace
    return XSI_OK;
}

}  // namespace xsi

extern "C" {

int xsi_hip_decode_ld_gt(xsi_hip_ctx* ctx, const void* d_file, uint64_t file_len, uint64_t first_block, uint64_t n_blocks,
                         const uint32_t* h_n_allele, uint64_t n_lines, uint32_t window, uint32_t* d_n11, float* d_r2,
                         uint32_t* d_n_called, uint64_t capacity_lines, uint64_t* h_n_bin) {
    if (!ctx || !d_file || !h_n_allele) return set_error(XSI_ERR_ARG, "decode_ld_gt: null argument");
    if (!d_n11 && !d_r2 && !d_n_called) return set_error(XSI_ERR_ARG, "decode_ld_gt: all three outputs are null");
    if (!window || window > XSI_LD_MAX_WINDOW)
        return set_error(XSI_ERR_ARG, "decode_ld_gt: window %u outside 1 .. %u", window, (unsigned)XSI_LD_MAX_WINDOW);
    if (file_len < 256) return set_error(XSI_ERR_FORMAT, "file image shorter than the 256-byte header");
    HIP_TRY(hipSetDevice(ctx->device));
    DecodePlan P;
    int rc = decode_prepare(ctx, d_file, file_len, first_block, n_blocks, &P, /*counts_only=*/true);
    if (rc) return rc;
    // BCF and binary lines of every block the call reads: the requested ones, then the look-ahead blocks (as decode_ld)
    std::vector<uint32_t> bins(P.n_blocks), bcfs(P.n_blocks);
    for (uint32_t b = 0; b < P.n_blocks; ++b) {
        bins[b] = P.blocks_h[b].n_bin;
        bcfs[b] = P.blocks_h[b].n_bcf;
    }
    const uint64_t file_blocks = P.file_blocks;
    uint64_t next = first_block + n_blocks;
    {
        uint64_t lines = 0, chunk = 1;
        while (lines < window && next < file_blocks) {
            const uint64_t nb = std::min<uint64_t>(chunk, std::min<uint64_t>(file_blocks - next, 0xFFFFFFull));
            DecodePlan Q;
            if ((rc = decode_prepare(ctx, d_file, file_len, next, nb, &Q, /*counts_only=*/true))) return rc;
            for (uint32_t b = 0; b < Q.n_blocks && lines < window; ++b, ++next) {
                bins.push_back(Q.blocks_h[b].n_bin);
                bcfs.push_back(Q.blocks_h[b].n_bcf);
                lines += Q.blocks_h[b].n_bin;
            }
            chunk *= 2;
        }
    }
    uint64_t need = 0;
    for (uint32_t v : bcfs) need += v;
    if (n_lines < need)
        return set_error(XSI_ERR_ARG, "decode_ld_gt: the call reads %llu BCF lines (%u requested blocks and %llu look-ahead blocks), "
                         "n_lines is %llu", (unsigned long long)need, P.n_blocks, (unsigned long long)(bins.size() - P.n_blocks),
                         (unsigned long long)n_lines);
    if (n_lines > need) {  // no more than the lines left in the file
        uint64_t left = need;
        for (uint64_t b = next; b < file_blocks;) {
            const uint64_t nb = std::min<uint64_t>(file_blocks - b, 0xFFFFFFull);
            DecodePlan Q;
            if ((rc = decode_prepare(ctx, d_file, file_len, b, nb, &Q, /*counts_only=*/true))) return rc;
            left += Q.n_bcf;
            b += nb;
        }
        if (n_lines > left)
            return set_error(XSI_ERR_ARG, "decode_ld_gt: n_lines is %llu, the file holds %llu BCF lines from block %llu on",
                             (unsigned long long)n_lines, (unsigned long long)left, (unsigned long long)first_block);
    }
    std::vector<uint64_t> line0(bins.size() + 1, 0);  // first BCF line of every block read, relative to h_n_allele
    for (size_t b = 0; b < bins.size(); ++b) {
        uint64_t sum = 0;
        for (uint64_t l = line0[b]; l < line0[b] + bcfs[b]; ++l) {
            if (h_n_allele[l] < 2)
                return set_error(XSI_ERR_ARG, "decode_ld_gt: line %llu has fewer than 2 alleles", (unsigned long long)l);
            sum += h_n_allele[l] - 1;
        }
        if (sum != bins[b])
            return set_error(XSI_ERR_ARG, "decode_ld_gt: allele numbers of %sblock %llu give %llu binary lines, the block has %u",
                             b < P.n_blocks ? "" : "look-ahead ", (unsigned long long)(first_block + b), (unsigned long long)sum,
                             bins[b]);
        line0[b + 1] = line0[b] + bcfs[b];
    }
    if (h_n_bin) *h_n_bin = P.n_bin;
    if (P.n_bin > capacity_lines)
        return set_error(XSI_ERR_CAPACITY, "decode_ld_gt: %u binary lines, capacity %llu", P.n_bin, (unsigned long long)capacity_lines);
    if (!P.n_bin) return XSI_OK;
    const uint32_t N = P.L.N, stride_w = P.L.y_stride64 * 2u;
    const uint32_t kw = (((N + 31u) / 32u) + LD_KC - 1u) / LD_KC * LD_KC;
    // per BCF line: its int32 row; per binary line: its decoded plane, up to 3 side planes, the carrier and called planes
    // and their counts; the look-ahead lines of a range come on top
    const auto cuts = score_ranges(P, ws_budget_now(ctx) / 2, 4ull * N, 4ull * (4ull * stride_w + 2ull * kw + 3u), 0);
    uint64_t row0 = 0;
    for (size_t c = 0; c + 1 < cuts.size(); ++c) {
        uint32_t rows = 0;
        for (uint32_t b = cuts[c]; b < cuts[c + 1]; ++b) rows += bins[b];
        size_t ext = cuts[c + 1];
        uint64_t more = 0;
        while (more < window && ext < bins.size()) more += bins[ext++];
        if (!rows) continue;
        DecodePlan R;
        if ((rc = decode_prepare(ctx, d_file, file_len, first_block + cuts[c], ext - cuts[c], &R))) return rc;
        if ((uint64_t)R.n_bin != rows + more || (uint64_t)R.n_bcf != line0[ext] - line0[cuts[c]])
            return set_error(XSI_ERR_FORMAT, "decode_ld_gt: block line counts changed between reads");
        LdArgs A{nullptr, nullptr, kw, N, window, rows, R.n_bin, d_n11 ? d_n11 + row0 * window : nullptr,
                 d_r2 ? d_r2 + row0 * window : nullptr, nullptr, nullptr, d_n_called ? d_n_called + row0 * window : nullptr};
        if ((rc = ld_gt_range(ctx, d_file, R, h_n_allele + line0[cuts[c]], rows, window, kw, A))) return rc;
        row0 += rows;
    }
    stage_collect(ctx);
    return XSI_OK;
}

}  // extern "C"
