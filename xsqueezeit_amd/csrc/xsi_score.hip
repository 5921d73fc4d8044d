// xsi_score.hip — weighted genotype scores on the decoded blocks: the transpose of xsi_hip_decode_dot.
// out[i][k] = sum over binary lines r of dosage(i, r) * w[r][k] (i = sample, or haplotype), the product
// polygenic scores (PLINK --score) and iterative solvers (randomized PCA, CG) need next to X.y.
//
// Data path: ALT-carrier bit planes of a range of blocks (decode_planes with the negation applied, or int32 rows
// composed on the general path and turned back into planes of exactly that layout) -> per-block partial sums
// S_b (k_score_vec / k_score_mfma, SCORE_SPLIT line slices per block) -> k_score_fold: out = (acc ? out : 0)
// + S_b0 + S_b1 + ... in block order.  Every S_b depends only on its block's planes, its weights and K, so the
// result is the same bits for any range cut (workspace budget), any split of the request into ACCUMULATE calls
// and either entry point.
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

// Line slices per block: wave w of a workgroup takes lines [n w / 4, n (w + 1) / 4) of its block and writes a partial
// of its own; the fold adds the four in slice order.  A constant, so the order never depends on the range.
constexpr uint32_t SCORE_SPLIT = 4;

struct ScoreArgs {
    const uint32_t* planes;  // [n_bin][stride_w], range-relative binary lines
    uint32_t stride_w;
    const uint8_t* kind;     // KIND_HAPLOID: the line's plane holds compact sample bits
    const DecBlock* blocks;  // first_bin, n_bin of every block of the range
    const double* w;         // [n_bin][K], the range's first line at row 0
    uint32_t K, N, n_samples, n_out;
    double* part;            // [block][SCORE_SPLIT][n_out][K]
};

// Few scores: a lane owns one 16-haplotype half-word of the diploid rows (8 samples) - on a fully haploid line the
// byte of the same 8 samples' compact bits - and walks its slice of the block's lines.  Reads are coalesced (128 B
// per wave and line), the line's KB weights are wave-uniform (scalar loads), accumulators float64 in VGPRs.  A line
// whose stripe is zero for the whole wave is skipped; a weight is only ever added where the dosage is nonzero, so
// non-finite weights reach the carriers of their line and no one else.
template <int KB, bool HAP>
__global__ void __launch_bounds__(256) k_score_vec(ScoreArgs A, uint32_t k0) {
    constexpr int R = HAP ? 16 : 8;  // output rows per lane
    constexpr uint32_t U = 8;        // lines in flight per lane
    const uint32_t b = blockIdx.y;
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t lane = lane_id();
    const uint32_t j = blockIdx.x * 64u + lane;
    const uint32_t nb = A.blocks[b].n_bin, fb = A.blocks[b].first_bin;
    const uint32_t lo = fb + (uint32_t)((uint64_t)nb * wv / SCORE_SPLIT), hi = fb + (uint32_t)((uint64_t)nb * (wv + 1u) / SCORE_SPLIT);
    const bool dip_ok = j * 16u < A.N, hap_ok = j * 8u < A.n_samples;
    double acc[R][KB];
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
        for (int k = 0; k < KB; ++k) acc[i][k] = 0.0;
    for (uint32_t r0 = lo; r0 < hi; r0 += U) {
        uint32_t v[U];
        bool hpl[U];
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) {
            const uint32_t r = r0 + u;
            v[u] = 0u;
            hpl[u] = false;
            if (r < hi) {
                hpl[u] = (A.kind[r] & KIND_HAPLOID) != 0u;
                const uint32_t* row = A.planes + (size_t)r * A.stride_w;
                if (hpl[u]) {
                    if (hap_ok) v[u] = reinterpret_cast<const uint8_t*>(row)[j];
                } else if (dip_ok) {
                    v[u] = reinterpret_cast<const uint16_t*>(row)[j];
                }
            }
        }
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) {
            const uint32_t r = r0 + u;
            if (r >= hi || __ballot(v[u] != 0u) == 0ull) continue;
            double wk[KB];
#pragma unroll
            for (int k = 0; k < KB; ++k) wk[k] = A.w[(size_t)r * A.K + k0 + (uint32_t)k];
            const uint32_t x = v[u];
            if (hpl[u]) {
#pragma unroll
                for (int s = 0; s < 8; ++s)
                    if ((x >> s) & 1u)
#pragma unroll
                        for (int k = 0; k < KB; ++k) acc[HAP ? 2 * s : s][k] += wk[k];
            } else if (HAP) {
#pragma unroll
                for (int h = 0; h < R; ++h)
                    if ((x >> h) & 1u)
#pragma unroll
                        for (int k = 0; k < KB; ++k) acc[h][k] += wk[k];
            } else {
#pragma unroll
                for (int s = 0; s < 8; ++s) {
                    const uint32_t d = ((x >> (2 * s)) & 1u) + ((x >> (2 * s + 1)) & 1u);
                    if (d)
#pragma unroll
                        for (int k = 0; k < KB; ++k) acc[s][k] += (double)d * wk[k];
                }
            }
        }
    }
    double* out = A.part + ((size_t)b * SCORE_SPLIT + wv) * (size_t)A.n_out * A.K;
#pragma unroll
    for (int i = 0; i < R; ++i) {
        const uint32_t row = j * (uint32_t)R + (uint32_t)i;
        if (row < A.n_out)
#pragma unroll
            for (int k = 0; k < KB; ++k) out[(size_t)row * A.K + k0 + (uint32_t)k] = acc[i][k];
    }
}

// Many scores: v_mfma_f64_16x16x4_f64 with A = dosages [16 rows x 4 lines], B = weights [4 lines x 16 scores].
// Lane l holds A[row l&15][line l>>4] and B[line l>>4][score l&15]; result register i of lane l is
// C[row (l>>4) + 4i][score l&15].  A wave owns 16 * SCORE_TILES = 64 output rows and 16 scores.  Its rows span at most
// 4 stripe words of a line, so one load covers 16 lines: lane l loads word (l&3) of line (l>>2), and only the words
// the wave's tiles read (4, 2 or 1 by the layout below; the others stay 0).  The next 16 lines are loaded while the
// current ones are contracted.  A run of 16 lines, or a group of 4, whose loaded words are all zero is skipped (the
// ballot sees only the wave's own columns), and so is an all-zero A tile.  Every tile takes its word of a line from the
// lane that loaded it (ds_bpermute).  Where the word sits and which bits a row reads depend on the line:
//   per sample, diploid : tile t = word t,      row m = bits 2m, 2m+1 (dosage 0..2)
//   per sample, haploid : tile t = word t/2,    row m = bit 16(t&1) + m
//   per haplotype, dipl.: tile t = word t/2,    row m = bit 16(t&1) + m
//   per haplotype, hapl.: tile t = word t/4,    row m = bit 8(t&3) + m/2 for even m (haplotype 2s), 0 for odd m
// so fully haploid lines need no scalar fall-back.  A group whose weights are not all finite is added row by row
// instead (0 * inf in the matrix core would reach non-carriers).  Groups are the 4-line steps from the slice's first
// line, each added in line order, whatever is skipped: the sums do not depend on the load scheme.
typedef double xsi_sd4 __attribute__((ext_vector_type(4)));
constexpr uint32_t SCORE_TILES = 4;  // 16-row tiles per wave: 64 rows, a multiple of 64 as the haploid layouts need
static_assert(SCORE_TILES == 4u, "k_score_mfma loads 4 stripe words per line (lane & 3) and reads words 0..3 of them");

template <bool HAP>
__global__ void __launch_bounds__(256) k_score_mfma(ScoreArgs A) {
    const uint32_t b = blockIdx.y, k0 = blockIdx.z * 16u;
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t lane = lane_id(), q = lane >> 4, m = lane & 15u;
    const uint32_t R0 = blockIdx.x * 16u * SCORE_TILES;
    const uint32_t nb = A.blocks[b].n_bin, fb = A.blocks[b].first_bin;
    const uint32_t lo = fb + (uint32_t)((uint64_t)nb * wv / SCORE_SPLIT), hi = fb + (uint32_t)((uint64_t)nb * (wv + 1u) / SCORE_SPLIT);
    const uint32_t col = k0 + m;
    const bool cvalid = col < A.K;
    // first stripe word of the wave and words its tiles read: diploid, haploid line
    const uint32_t base_dip = HAP ? R0 / 32u : R0 / 16u, base_hap = HAP ? R0 / 64u : R0 / 32u;
    const uint32_t nw_dip = HAP ? SCORE_TILES / 2u : SCORE_TILES, nw_hap = HAP ? SCORE_TILES / 4u : SCORE_TILES / 2u;
    // this lane's load: word (lane & 3) of line base + (lane >> 2); bit 0 of the flag = loaded line is haploid
    auto load = [&](uint32_t base, uint32_t& word, uint32_t& hflag) {
        const uint32_t r = base + (lane >> 2), ws = lane & 3u;
        word = 0u;
        hflag = 0u;
        if (r < hi) {
            hflag = (A.kind[r] & KIND_HAPLOID) != 0u ? 1u : 0u;
            const uint32_t wi = (hflag ? base_hap : base_dip) + ws;
            if (ws < (hflag ? nw_hap : nw_dip) && wi < A.stride_w) word = A.planes[(size_t)r * A.stride_w + wi];
        }
    };
    xsi_sd4 acc[SCORE_TILES];
#pragma unroll
    for (int t = 0; t < (int)SCORE_TILES; ++t) acc[t] = (xsi_sd4){0.0, 0.0, 0.0, 0.0};
    uint32_t nword, nflag;
    load(lo, nword, nflag);
    for (uint32_t base = lo; base < hi; base += 16u) {
        const uint32_t cword = nword, cflag = nflag;
        if (base + 16u < hi) load(base + 16u, nword, nflag);
        const uint64_t nz = __ballot(cword != 0u);
        if (nz == 0ull) continue;
#pragma unroll 1
        for (uint32_t sub = 0; sub < 4u; ++sub) {
            if (((nz >> (16u * sub)) & 0xFFFFull) == 0ull) continue;  // lines base + 4 sub .. + 3: nothing in the wave's rows
            const uint32_t r = base + 4u * sub + q;     // this lane's line of the group (A row, B row)
            const uint32_t owner = (4u * sub + q) << 2;  // first lane that loaded it
            const bool hpl = __shfl((int)cflag, (int)owner, 64) != 0;
            const double bv = (r < hi && cvalid) ? A.w[(size_t)r * A.K + col] : 0.0;
            const bool finite = __ballot(!__builtin_isfinite(bv)) == 0ull;
#pragma unroll
            for (int t = 0; t < (int)SCORE_TILES; ++t) {
                uint32_t src, bit;
                bool two = false, valid = true;
                if (!hpl && !HAP) {
                    src = (uint32_t)t;
                    bit = 2u * m;
                    two = true;
                } else if (!hpl || !HAP) {
                    src = (uint32_t)t >> 1;
                    bit = 16u * ((uint32_t)t & 1u) + m;
                } else {
                    src = (uint32_t)t >> 2;
                    bit = 8u * ((uint32_t)t & 3u) + (m >> 1);
                    valid = (m & 1u) == 0u;
                }
                const uint32_t wt = (uint32_t)__shfl((int)cword, (int)(owner | src), 64);
                uint32_t d = valid ? (wt >> bit) & 1u : 0u;
                if (two) d += (wt >> (bit + 1u)) & 1u;
                if (__ballot(d != 0u) == 0ull) continue;
                const double a = (double)d;
                if (finite) {
                    acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bv, acc[t], 0, 0, 0);
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int jl = 0; jl < 4; ++jl) {
                            const double di = __shfl(a, (int)(((uint32_t)jl << 4) | (q + 4u * (uint32_t)i)), 64);
                            const double wj = __shfl(bv, (int)(((uint32_t)jl << 4) | m), 64);
                            if (di != 0.0) acc[t][i] += di * wj;
                        }
                }
            }
        }
    }
    if (!cvalid) return;
    double* out = A.part + ((size_t)b * SCORE_SPLIT + wv) * (size_t)A.n_out * A.K;
#pragma unroll
    for (int t = 0; t < (int)SCORE_TILES; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t row = R0 + 16u * (uint32_t)t + q + 4u * (uint32_t)i;
            if (row < A.n_out) out[(size_t)row * A.K + col] = acc[t][i];
        }
}

// out[e] = (accumulate ? out[e] : 0) + S_b0[e] + S_b1[e] + ..., S_b = its slices added in slice order.
__global__ void __launch_bounds__(256) k_score_fold(const double* __restrict__ part, uint32_t n_blocks, uint64_t n_elem,
                                                    double* __restrict__ out, int accumulate) {
    const uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (e >= n_elem) return;
    double acc = accumulate ? out[e] : 0.0;
    for (uint32_t b = 0; b < n_blocks; ++b) {
        const double* p = part + (size_t)b * SCORE_SPLIT * n_elem + e;
        double s = p[0];
#pragma unroll
        for (uint32_t w = 1; w < SCORE_SPLIT; ++w) s += p[(size_t)w * n_elem];
        acc += s;
    }
    out[e] = acc;
}

// General path: composed int32 rows -> one ALT-carrier plane per binary line, in the plane path's layout (haplotype
// bits; compact sample bits on fully haploid lines; zero padding).  Missing and end-of-vector values never match.
// One workgroup per binary line, every wave turns 64 values into two plane words by a ballot.
__global__ void __launch_bounds__(256) k_score_rows_to_planes(const int32_t* __restrict__ rows, uint64_t row_stride,
                                                              const uint32_t* __restrict__ line_ngt,
                                                              const uint32_t* __restrict__ bin_parent,
                                                              const uint32_t* __restrict__ bin_alt, uint32_t n_samples,
                                                              uint32_t stride_w, uint32_t* __restrict__ planes,
                                                              uint8_t* __restrict__ kind) {
    const uint32_t l = blockIdx.x, lane = lane_id(), wv = threadIdx.x >> 6;
    const uint32_t parent = bin_parent[l];
    const int32_t alt = (int32_t)bin_alt[l];
    const uint32_t nv = line_ngt[parent];
    const bool haploid = nv == n_samples;
    const int32_t* row = rows + (size_t)parent * row_stride;
    uint32_t* out = planes + (size_t)l * stride_w;
    for (uint32_t c = wv; 2u * c < stride_w; c += 4u) {
        const uint32_t idx = c * 64u + lane;
        const bool hit = idx < nv && ((row[idx] >> 1) - 1) == alt;
        const uint64_t mask = __ballot(hit);
        if (lane == 0) {
            out[2u * c] = (uint32_t)mask;
            if (2u * c + 1u < stride_w) out[2u * c + 1u] = (uint32_t)(mask >> 32);
        }
    }
    if (threadIdx.x == 0) kind[l] = haploid ? (uint8_t)KIND_HAPLOID : (uint8_t)0;
}

// Planes of one range (P) -> partials -> folded into d_out.
static int score_contract(xsi_hip_ctx* ctx, const DecodePlan& P, const uint32_t* planes, uint32_t stride_w, const uint8_t* kind,
                          const double* d_w, uint32_t K, bool per_hap, double* d_out, bool accumulate) {
    hipStream_t s = ctx->stream;
    const uint32_t n_out = per_hap ? P.L.N : P.L.n_samples;
    const uint64_t n_elem = (uint64_t)n_out * K;
    double* part;
    WS(part, "score.part", 8ull * SCORE_SPLIT * n_elem * P.n_blocks);
    ScoreArgs A{planes, stride_w, kind, P.d_blocks, d_w, K, P.L.N, P.L.n_samples, n_out, part};
    stage_mark(ctx, XSI_ST_SCORE);
    const dim3 block(256);
    if (K >= 8u && !tuning_env("XSI_SCORE_SCALAR")) {
        const dim3 grid((n_out + 16u * SCORE_TILES - 1u) / (16u * SCORE_TILES), P.n_blocks, (K + 15u) / 16u);
        if (per_hap)
            k_score_mfma<true><<<grid, block, 0, s>>>(A);
        else
            k_score_mfma<false><<<grid, block, 0, s>>>(A);
    } else {
        const dim3 grid((n_out + (per_hap ? 1023u : 511u)) / (per_hap ? 1024u : 512u), P.n_blocks);
        uint32_t k0 = 0;
        for (; k0 + 4u <= K; k0 += 4u)
            per_hap ? k_score_vec<4, true><<<grid, block, 0, s>>>(A, k0) : k_score_vec<4, false><<<grid, block, 0, s>>>(A, k0);
        switch (K - k0) {
            case 3: per_hap ? k_score_vec<3, true><<<grid, block, 0, s>>>(A, k0) : k_score_vec<3, false><<<grid, block, 0, s>>>(A, k0); break;
            case 2: per_hap ? k_score_vec<2, true><<<grid, block, 0, s>>>(A, k0) : k_score_vec<2, false><<<grid, block, 0, s>>>(A, k0); break;
            case 1: per_hap ? k_score_vec<1, true><<<grid, block, 0, s>>>(A, k0) : k_score_vec<1, false><<<grid, block, 0, s>>>(A, k0); break;
            default: break;
        }
    }
    HIP_TRY(hipGetLastError());
    k_score_fold<<<dim3((unsigned)((n_elem + 255u) / 256u)), block, 0, s>>>(part, P.n_blocks, n_elem, d_out, accumulate ? 1 : 0);
    HIP_TRY(hipGetLastError());
    stage_mark(ctx, -1);
    return XSI_OK;
}

static int score_args(xsi_hip_ctx* ctx, const void* d_file, const double* d_w, uint32_t K, double* d_out, uint32_t flags,
                      uint64_t file_len, const char* who) {
    if (!ctx || !d_file || !d_w || !d_out) return set_error(XSI_ERR_ARG, "%s: null argument", who);
    if (!K) return set_error(XSI_ERR_ARG, "%s: n_scores must be > 0", who);
    if (flags & ~(uint32_t)(XSI_SCORE_ACCUMULATE | XSI_SCORE_PER_HAPLOTYPE))
        return set_error(XSI_ERR_ARG, "%s: unknown flag bits 0x%x", who, flags & ~(uint32_t)(XSI_SCORE_ACCUMULATE | XSI_SCORE_PER_HAPLOTYPE));
    if (file_len < 256) return set_error(XSI_ERR_FORMAT, "file image shorter than the 256-byte header");
    return XSI_OK;
}

// Ranges of whole blocks whose bytes (per BCF line, per binary line, per block) fit `budget`; at least one block each.
std::vector<uint32_t> score_ranges(const DecodePlan& P, uint64_t budget, uint64_t per_bcf, uint64_t per_bin, uint64_t per_block) {
    std::vector<uint32_t> cuts{0};
    uint64_t used = 0;
    for (uint32_t b = 0; b < P.n_blocks; ++b) {
        const uint64_t need = per_bcf * P.blocks_h[b].n_bcf + per_bin * P.blocks_h[b].n_bin + per_block;
        if (b > cuts.back() && (used + need > budget || b - cuts.back() >= 65535u)) {
            cuts.push_back(b);
            used = 0;
        }
        used += need;
    }
    cuts.push_back(P.n_blocks);
    return cuts;
}

}  // namespace xsi

extern "C" {

int xsi_hip_decode_score(xsi_hip_ctx* ctx, const void* d_file, uint64_t file_len, uint64_t first_block, uint64_t n_blocks,
                         const double* d_weights, uint64_t n_weight_lines, uint32_t n_scores, double* d_out, uint64_t out_rows,
                         uint32_t flags) {
    int rc = score_args(ctx, d_file, d_weights, n_scores, d_out, flags, file_len, "decode_score");
    if (rc) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    const bool per_hap = (flags & XSI_SCORE_PER_HAPLOTYPE) != 0u;
    DecodePlan P;
    rc = decode_prepare(ctx, d_file, file_len, first_block, n_blocks, &P, /*counts_only=*/true);
    if (rc) return rc;
    // as decode_dot: the planes alone say who carries the ALT allele only on bi-allelic, fully called lines
    for (auto& b : P.blocks_h)
        if (b.n_bin != b.n_bcf || b.off_line_missing != VAL_UNDEFINED || b.off_line_eov != VAL_UNDEFINED)
            return set_error(XSI_ERR_UNSUPPORTED, "decode_score: multi-allelic lines or missing / end-of-vector entries in the "
                             "requested blocks; use xsi_hip_decode_score_gt");
    if (n_weight_lines != P.n_bin)
        return set_error(XSI_ERR_ARG, "decode_score: the blocks hold %u binary lines, the weights %llu", P.n_bin,
                         (unsigned long long)n_weight_lines);
    const uint32_t n_out = per_hap ? P.L.N : P.L.n_samples;
    if (out_rows < n_out)
        return set_error(XSI_ERR_CAPACITY, "decode_score: %u output rows needed, %llu given", n_out, (unsigned long long)out_rows);
    const uint32_t stride_w = P.L.y_stride64 * 2u;
    // per binary line: its plane and the expanded WAH row of the decode; per block: the partial sums
    const auto cuts = score_ranges(P, ws_budget_now(ctx) / 2, 0, 3ull * 4ull * stride_w,
                                   8ull * SCORE_SPLIT * n_out * (uint64_t)n_scores);
    uint64_t bin0 = 0;
    for (size_t c = 0; c + 1 < cuts.size(); ++c) {
        DecodePlan R;
        DecodePlan* Q = &P;
        if (cuts.size() > 2) {  // one range: the plan of the whole request serves
            rc = decode_prepare(ctx, d_file, file_len, first_block + cuts[c], cuts[c + 1] - cuts[c], &R);
            Q = &R;
        } else {
            rc = decode_plan_scratch(ctx, &P);
        }
        if (rc) return rc;
        uint32_t* planes;
        WS(planes, "score.planes", 4ull * stride_w * (size_t)(Q->n_bin ? Q->n_bin : 1));
        rc = decode_planes(ctx, d_file, *Q, planes, stride_w, /*apply_negation=*/1);
        if (rc) return rc;
        rc = score_contract(ctx, *Q, planes, stride_w, Q->L.kind, d_weights + bin0 * n_scores, n_scores, per_hap, d_out,
                            c > 0 || (flags & XSI_SCORE_ACCUMULATE));
        if (rc) return rc;
        bin0 += Q->n_bin;
        if (cuts.size() > 2) HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    stage_collect(ctx);
    return XSI_OK;
}

}  // extern "C"

namespace xsi {

// One range of blocks through the composed rows.  h_n_allele covers exactly these blocks.
static int score_gt_range(xsi_hip_ctx* ctx, const void* d_file, DecodePlan& P, const uint32_t* h_n_allele, const double* d_w,
                          uint32_t K, bool per_hap, double* d_out, bool accumulate) {
    hipStream_t s = ctx->stream;
    const uint32_t n_bcf = P.n_bcf, N = P.L.N;
    std::vector<uint32_t> first_bin(n_bcf), parent(P.n_bin + 1u), alt(P.n_bin + 1u);
    {
        uint32_t l = 0;
        for (uint32_t b = 0; b < P.n_blocks; ++b) {
            uint32_t acc = P.blocks_h[b].first_bin;
            const uint32_t end = acc + P.blocks_h[b].n_bin;
            for (uint32_t i = 0; i < P.blocks_h[b].n_bcf; ++i, ++l) {
                first_bin[l] = acc;
                for (uint32_t k = 1; k < h_n_allele[l] && acc < end; ++k, ++acc) {
                    parent[acc] = l;
                    alt[acc] = k;
                }
                if (acc - first_bin[l] != h_n_allele[l] - 1) acc = end + 1;  // overran the block: caught below
            }
            if (acc != end)
                return set_error(XSI_ERR_ARG, "decode_score_gt: allele numbers of block %u do not add up to its %u binary lines", b,
                                 P.blocks_h[b].n_bin);
        }
    }
    uint32_t *d_first_bin, *d_nallele, *d_line_ngt, *d_parent, *d_alt, *planes;
    uint8_t* kind;
    int32_t* d_rows;
    const uint32_t stride_w = P.L.y_stride64 * 2u;
    WS(d_first_bin, "gt.bcf_first_bin", 4ull * n_bcf);
    WS(d_nallele, "gt.bcf_nallele", 4ull * n_bcf);
    WS(d_line_ngt, "gt.line_ngt", 4ull * n_bcf);
    WS(d_parent, "dot.bin_parent", 4ull * P.n_bin + 4);
    WS(d_alt, "dot.bin_alt", 4ull * P.n_bin + 4);
    WS(d_rows, "dot.rows", 4ull * N * (size_t)(n_bcf ? n_bcf : 1));
    WS(planes, "score.planes", 4ull * stride_w * (size_t)(P.n_bin ? P.n_bin : 1));
    WS(kind, "score.kind", (size_t)P.n_bin + 64);
    HIP_TRY(hipMemcpyAsync(d_first_bin, first_bin.data(), 4ull * n_bcf, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_nallele, h_n_allele, 4ull * n_bcf, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_parent, parent.data(), 4ull * P.n_bin, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_alt, alt.data(), 4ull * P.n_bin, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));  // local vectors: the copies must have left host memory
    DecodedPlanes DPn;
    int rc = decode_all_planes(ctx, d_file, P, &DPn);
    if (rc) return rc;
    rc = compose_lines(ctx, P, DPn, d_first_bin, d_nallele, n_bcf, d_rows, N, d_line_ngt, nullptr, 0);
    if (rc) return rc;
    if (P.n_bin) {
        stage_mark(ctx, XSI_ST_GT_UNPACK);
        k_score_rows_to_planes<<<dim3(P.n_bin), dim3(256), 0, s>>>(d_rows, N, d_line_ngt, d_parent, d_alt, P.L.n_samples, stride_w,
                                                                  planes, kind);
        HIP_TRY(hipGetLastError());
    }
    rc = score_contract(ctx, P, planes, stride_w, kind, d_w, K, per_hap, d_out, accumulate);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    return XSI_OK;
}

}  // namespace xsi

extern "C" {

int xsi_hip_decode_score_gt(xsi_hip_ctx* ctx, const void* d_file, uint64_t file_len, uint64_t first_block, uint64_t n_blocks,
                            const uint32_t* h_n_allele, uint64_t n_lines, const double* d_weights, uint64_t n_weight_lines,
                            uint32_t n_scores, double* d_out, uint64_t out_rows, uint32_t flags) {
    int rc = score_args(ctx, d_file, d_weights, n_scores, d_out, flags, file_len, "decode_score_gt");
    if (rc) return rc;
    if (!h_n_allele) return set_error(XSI_ERR_ARG, "decode_score_gt: null argument");
    HIP_TRY(hipSetDevice(ctx->device));
    const bool per_hap = (flags & XSI_SCORE_PER_HAPLOTYPE) != 0u;
    uint64_t n_bin_total = 0;
    for (uint64_t l = 0; l < n_lines; ++l) {
        if (h_n_allele[l] < 2)
            return set_error(XSI_ERR_ARG, "decode_score_gt: line %llu has fewer than 2 alleles", (unsigned long long)l);
        n_bin_total += h_n_allele[l] - 1;
    }
    DecodePlan P;
    rc = decode_prepare(ctx, d_file, file_len, first_block, n_blocks, &P, /*counts_only=*/true);
    if (rc) return rc;
    if (P.n_bcf != n_lines)
        return set_error(XSI_ERR_ARG, "decode_score_gt: blocks hold %u BCF lines, caller passed %llu", P.n_bcf, (unsigned long long)n_lines);
    if (n_bin_total != P.n_bin)
        return set_error(XSI_ERR_ARG, "decode_score_gt: allele numbers give %llu binary lines, the blocks hold %u",
                         (unsigned long long)n_bin_total, P.n_bin);
    {
        uint64_t l = 0;  // every block's lines must add up, not just the total: nothing is written before this holds
        for (uint32_t b = 0; b < P.n_blocks; ++b) {
            uint64_t bins = 0;
            for (uint32_t i = 0; i < P.blocks_h[b].n_bcf; ++i) bins += h_n_allele[l++] - 1;
            if (bins != P.blocks_h[b].n_bin)
                return set_error(XSI_ERR_ARG, "decode_score_gt: allele numbers of block %u give %llu binary lines, the block has %u", b,
                                 (unsigned long long)bins, P.blocks_h[b].n_bin);
        }
    }
    if (n_weight_lines != P.n_bin)
        return set_error(XSI_ERR_ARG, "decode_score_gt: the blocks hold %u binary lines, the weights %llu", P.n_bin,
                         (unsigned long long)n_weight_lines);
    const uint32_t n_out = per_hap ? P.L.N : P.L.n_samples;
    if (out_rows < n_out)
        return set_error(XSI_ERR_CAPACITY, "decode_score_gt: %u output rows needed, %llu given", n_out, (unsigned long long)out_rows);
    const uint32_t stride_w = P.L.y_stride64 * 2u;
    // per BCF line: its int32 row; per binary line: its decoded plane, up to 3 side planes and its carrier plane;
    // per block: the partial sums
    const auto cuts = score_ranges(P, ws_budget_now(ctx) / 2, 4ull * P.L.N, 5ull * 4ull * stride_w,
                                   8ull * SCORE_SPLIT * n_out * (uint64_t)n_scores);
    uint64_t bin0 = 0, line0 = 0;
    for (size_t c = 0; c + 1 < cuts.size(); ++c) {
        DecodePlan R;
        DecodePlan* Q = &P;
        if (cuts.size() > 2) {
            rc = decode_prepare(ctx, d_file, file_len, first_block + cuts[c], cuts[c + 1] - cuts[c], &R);
            Q = &R;
        } else {
            rc = decode_plan_scratch(ctx, &P);
        }
        if (rc) return rc;
        rc = score_gt_range(ctx, d_file, *Q, h_n_allele + line0, d_weights + bin0 * n_scores, n_scores, per_hap, d_out,
                            c > 0 || (flags & XSI_SCORE_ACCUMULATE));
        if (rc) return rc;
        bin0 += Q->n_bin;
        line0 += Q->n_bcf;
    }
    stage_collect(ctx);
    return XSI_OK;
}

}  // extern "C"
