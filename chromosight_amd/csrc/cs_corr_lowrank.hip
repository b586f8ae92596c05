// cs_corr_lowrank.hip -- separable evaluation of truncated-SVD templates (`--tsvd`): K' of rank r and Q' (the reconstruction of the
// template's squares) of rank r2, both up to 8 (cs_api.cpp build_args checks the ranks and factors the weight sets).
//
// The reference's factorised branch (detection.py:648-665, preprocessing.py:810-847) runs r row passes and r column passes.  Here
// every window sum of the coefficient separates the same way (cs_corr_sep.hip states the rank-1 case).  The float32 weight sets of
// build_args, Wa = K' - mean (rank ra <= r + 1) and Wb = Q' - 2 mean K' + mean^2 (rank rb <= r2 + r + 1), are factored themselves,
// Wa = sum_j ua_j va_j^T and Wb = sum_k ub_k vb_k^T, so that the kernel forms exactly the sums the full-template kernels form:
//     cs = sum S Wa,   s1 = sum S,   s2 = sum S^2,   nm = sum M,   ka = sum M Wa,   kb = sum M Wb
// (M: the 0/1 missing plane), each as sum_j sum_a u_j[a] (sum_b v_j[b] X[i+a][j+b]).  No sum is a difference of larger ones, so the
// float32 error model of the candidate screen (cs_device.h cand_screen_*) holds as for the other float32 kernels.  A term is a
// (source plane, row weights, column weights) triple: (S^2, 1, 1), (S, 1, 1), (S, va_j, ua_j), and with a mask (M, 1, 1),
// (M, va_j, ua_j), (M, vb_k, ub_k).  A horizontal pass over the staged rows writes up to four terms' row sums per staged pixel into
// LDS planes, a vertical pass over km rows finishes them into the lane's accumulators; as many rounds as the terms need:
// (ra + 2) (km + kn) multiply-adds per pixel without a mask, (2 ra + rb + 3) (km + kn) with one.
//
// The missing plane is staged pixel by pixel with the framed predicate of cs_device.h (missing_from_flags / missing_pred), so the
// band frame, the virtual frame of `full` mode, sym_upper and max_dist come out as in the runtime-size kernel.  Epilogue: the lean
// float32 forms of cs_corr_large.hip (thresholds, missing_tol, n_obs, the candidate screen).  Outputs: maps (dense / band, n_obs),
// plain cross-correlations (xcorr_only: the factors of the raw weights, signal terms only) and the candidate sink
// (CorrArgs::cand_keys, the contract of cs_corr_large.hip).  Signals: dense and band layouts, float32 or float64.  Bands of counts and
// lazily evaluated bands are refused (kLaunchDeclined): the `--tsvd` calls of the pipeline pass neither (detect_block reads block.full(), a
// float64 band or dense map), and a refused call takes the other kernels.
//
// Weight table (float32, behind the three weight sets at A.w + 3 km kn): nt = 1 + ra + rb rows of kn row weights [1, va_j, vb_k],
// then nt rows of km column weights [1, ua_j, ub_k] (cs_api.cpp append_lowrank_table).
#include "cs_device.h"
#include "cs_launch.h"

namespace cs {

namespace {

constexpr int LR_TW = 64;   // output columns per block (= lanes per wave)
constexpr int LR_RG = 4;    // output rows per lane
constexpr int LR_NW = 8;    // waves per block
constexpr int LR_TH = LR_RG * LR_NW;
constexpr int LR_MAX_RANK = 8;

size_t lr_smem(int km, int kn, bool masked, int nq)
{
    const size_t LH = LR_TH + km - 1, LW = LR_TW + kn - 1, LWP = (LW + 3) & ~(size_t)3;
    const size_t sig = 4 * LH * LWP;
    const size_t msk = masked ? ((LH * LWP + 15) & ~(size_t)15) : 0;
    const size_t flags = masked ? ((LH + LW + 15) & ~(size_t)15) : 0;
    return sig + msk + flags + 4 * (size_t)nq * LH * LR_TW;
}

// Row sums of NQ terms over the staged rows r = wv, wv + LR_NW, ... (two rows per step share the weight loads): plane q gets
// sum_b f(x[b]) hw[q][b], f(x) = x * x for q == 0 when SQ0, else x.  hw: wave-uniform rows of the weight table (scalar loads).
template <int NQ, bool SQ0, typename SRC>
__device__ __forceinline__ void lr_hpass(const SRC* __restrict__ plane, int LWP, int LH, int kn, const float* const* hw, float* H,
                                         int wv, int lane)
{
    for (int r = wv; r < LH; r += 2 * LR_NW) {
        const int r2 = min(r + LR_NW, LH - 1);
        const SRC* row = plane + r * LWP + lane;
        const SRC* row2 = plane + r2 * LWP + lane;
        float h[NQ], k[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) h[q] = k[q] = 0.0f;
#pragma unroll 4
        for (int b = 0; b < kn; ++b) {
            const float x = (float)row[b], y = (float)row2[b];
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                if (SQ0 && q == 0) {
                    h[0] = fmaf(x, x, h[0]);
                    k[0] = fmaf(y, y, k[0]);
                } else {
                    const float w = hw[q][b];
                    h[q] = fmaf(x, w, h[q]);
                    k[q] = fmaf(y, w, k[q]);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            H[((size_t)q * LH + r) * LR_TW + lane] = h[q];
            if (r + LR_NW < LH) H[((size_t)q * LH + r2) * LR_TW + lane] = k[q];
        }
    }
}

template <bool SQ0, typename SRC>
__device__ __forceinline__ void lr_hpass_n(int nq, const SRC* plane, int LWP, int LH, int kn, const float* const* hw, float* H, int wv,
                                           int lane)
{
    switch (nq) {                                       // (wave-uniform)
        case 1: lr_hpass<1, SQ0>(plane, LWP, LH, kn, hw, H, wv, lane); break;
        case 2: lr_hpass<2, SQ0>(plane, LWP, LH, kn, hw, H, wv, lane); break;
        case 3: lr_hpass<3, SQ0>(plane, LWP, LH, kn, hw, H, wv, lane); break;
        default: lr_hpass<4, SQ0>(plane, LWP, LH, kn, hw, H, wv, lane); break;
    }
}

// column sums of one plane for the lane's LR_RG output rows: out[i] = sum_a vw[a] H[tr0 + i + a][lane]
__device__ __forceinline__ void lr_vpass(const float* __restrict__ Hq, const float* __restrict__ vw, int km, int tr0, int lane,
                                         float* out)
{
    float t[LR_RG];
#pragma unroll
    for (int i = 0; i < LR_RG; ++i) t[i] = 0.0f;
#pragma unroll 4
    for (int a = 0; a < km; ++a) {
        const float w = vw[a];
#pragma unroll
        for (int i = 0; i < LR_RG; ++i) t[i] = fmaf(w, Hq[(tr0 + i + a) * LR_TW + lane], t[i]);
    }
#pragma unroll
    for (int i = 0; i < LR_RG; ++i) out[i] = t[i];
}

}  // namespace

template <bool MASKED>
__global__ __launch_bounds__(512) void corr_lowrank_kernel(const CorrArgs<float> A, const int nq_max)
{
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int km = A.km, kn = A.kn, kk = km * kn;
    const int kh = (km - 1) / 2, kw = (kn - 1) / 2;
    const int LH = LR_TH + km - 1;
    const int LW = LR_TW + kn - 1;
    const int LWP = (LW + 3) & ~3;
    float* sS = reinterpret_cast<float*>(smem_raw);
    char* p = smem_raw + 4 * (size_t)LH * LWP;
    uint8_t* sM = reinterpret_cast<uint8_t*>(p);
    uint8_t* rfl = sM + (MASKED ? (((size_t)LH * LWP + 15) & ~(size_t)15) : 0);
    uint8_t* cfl = rfl + LH;
    float* H = reinterpret_cast<float*>(rfl + (MASKED ? ((LH + LW + 15) & ~15) : 0));      // [nq_max][LH][LR_TW]

    int i0, j0;
    if (!tile_origin(A, blockIdx.x, blockIdx.y, &i0, &j0)) return;
    const int tid = threadIdx.x;
    // rows no window of the row range [row_begin, row_end) reaches are not part of the input contract (row-window slabs)
    const int p_lo = A.row_begin - kh, p_hi = A.row_end + (km - 1) - kh;

    const bool bins = MASKED && A.mask_mode == 1;
    if (bins) {
        for (int idx = tid; idx < LH + LW; idx += 512) {
            const bool is_row = idx < LH;
            const int x = is_row ? i0 - kh + idx : j0 - kw + (idx - LH);
            const int n = is_row ? A.ms : A.ns;
            const uint8_t* src = is_row ? A.miss_row : A.miss_col;
            rfl[idx] = (x >= 0 && x < n) ? src[x] : 0;
        }
        __syncthreads();
    }
    for (int idx = tid; idx < LH * LWP; idx += 512) {
        const int tr = idx / LWP;
        const int tc = idx - tr * LWP;
        const int pp = i0 - kh + tr;
        const int q = j0 - kw + tc;
        sS[idx] = (pp >= p_lo && pp < p_hi) ? load_signal(A, pp, q) : 0.0f;
        if (MASKED) {
            const bool m = bins ? missing_from_flags(A, pp, q, rfl[tr] != 0, cfl[min(tc, LW - 1)] != 0, false, true) : missing_pred(A, pp, q);
            sM[idx] = (tc < LW && m) ? 1 : 0;
        }
    }
    __syncthreads();

    const int lane = tid & 63;
    const int wv = tid >> 6;
    const int tr0 = wv * LR_RG;
    const int rc = A.w_lrc, rb = A.w_lrb, nt = 1 + rc + rb;
    const float* hw_tab = A.w + 3 * (size_t)kk;          // nt rows of kn
    const float* vw_tab = hw_tab + (size_t)nt * kn;      // nt rows of km
    // accumulators: sum S^2, sum S, sum S Wa, sum M, sum M Wa, sum M Wb
    float s2[LR_RG], s1[LR_RG], cs[LR_RG], nm[LR_RG], ka[LR_RG], kb[LR_RG];
#pragma unroll
    for (int i = 0; i < LR_RG; ++i) s2[i] = s1[i] = cs[i] = nm[i] = ka[i] = kb[i] = 0.0f;

    // ---- signal terms t = 0 (S^2), 1 (S), 2 + j (S, va_j, ua_j): table row max(0, t - 1); a plain cross-correlation needs the last
    //      ones only
    const int ns_terms = 2 + rc;
    for (int t0 = A.xcorr_only ? 2 : 0; t0 < ns_terms; t0 += nq_max) {
        const int nq = min(nq_max, ns_terms - t0);
        const float* hw[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) hw[q] = hw_tab + (size_t)max(0, min(t0 + q, ns_terms - 1) - 1) * kn;
        if (t0 > 0) __syncthreads();                     // (the previous round's vertical pass has read the planes)
        if (t0 == 0) lr_hpass_n<true>(nq, sS, LWP, LH, kn, hw, H, wv, lane);
        else lr_hpass_n<false>(nq, sS, LWP, LH, kn, hw, H, wv, lane);
        __syncthreads();
        for (int q = 0; q < nq; ++q) {
            const int t = t0 + q;
            float v[LR_RG];
            lr_vpass(H + (size_t)q * LH * LR_TW, vw_tab + (size_t)max(0, t - 1) * km, km, tr0, lane, v);
#pragma unroll
            for (int i = 0; i < LR_RG; ++i) {
                if (t == 0) s2[i] += v[i];
                else if (t == 1) s1[i] += v[i];
                else cs[i] += v[i];
            }
        }
    }
    if (MASKED) {
        // ---- mask terms t = 0 (M), 1 + j (M, va_j, ua_j), 1 + rc + k (M, vb_k, ub_k): table row t
        for (int t0 = 0; t0 < nt; t0 += nq_max) {
            const int nq = min(nq_max, nt - t0);
            const float* hw[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) hw[q] = hw_tab + (size_t)min(t0 + q, nt - 1) * kn;
            __syncthreads();
            lr_hpass_n<false>(nq, sM, LWP, LH, kn, hw, H, wv, lane);
            __syncthreads();
            for (int q = 0; q < nq; ++q) {
                const int t = t0 + q;
                float v[LR_RG];
                lr_vpass(H + (size_t)q * LH * LR_TW, vw_tab + (size_t)t * km, km, tr0, lane, v);
#pragma unroll
                for (int i = 0; i < LR_RG; ++i) {
                    if (t == 0) nm[i] += v[i];
                    else if (t <= rc) ka[i] += v[i];
                    else kb[i] += v[i];
                }
            }
        }
    }

    // ---- epilogue (the sums are those of the full-template kernels: cs = sum S Wa, ka = sum M Wa, kb = sum M Wb)
    const bool sinking = A.cand_keys != nullptr;
#pragma unroll
    for (int i = 0; i < LR_RG; ++i) {
        const int oi = i0 + tr0 + i;
        const int oj = j0 + lane;
        if (oi >= A.row_end || oj >= A.ns) continue;
        const int d = oj - oi;
        if (d < A.out_lo || d > A.out_hi) continue;
        const bool zero = pixel_forced_zero(A, oi, oj);
        float rr, nobs = A.ks.n;
        if (zero) {
            rr = 0.0f;
        } else if (A.xcorr_only) {
            rr = (fabsf(cs[i]) < A.ks.thr) ? 0.0f : cs[i];
        } else if (MASKED) {
            rr = pearson_masked_lean(cs[i], s1[i], s2[i], nm[i], ka[i], kb[i], A.ks);
            nobs = A.ks.n - nm[i];
        } else {
            rr = pearson_nomask_lean(cs[i], s1[i], s2[i], A.ks);
        }
        if (sinking) {
            // candidate sink: keys tag + row * ns + col of the pixels with a candidate value (the screen's sentinel included); the
            // counter runs on beyond the capacity so that the caller learns how much room a second call needs
            if (!zero && rr >= A.ks.cand_thr) {
                const unsigned long long pos = atomicAdd(A.cand_count, 1ull);
                if (pos < (unsigned long long)A.cand_cap)
                    A.cand_keys[pos] = A.cand_tag + (unsigned long long)oi * (unsigned long long)A.ns + (unsigned long long)oj;
            }
            continue;
        }
        store_pixel(A, oi, oj, rr, nobs);
    }
}

bool corr_lowrank_supports(const CorrArgs<float>& A)
{
    return A.w_lr >= 1 && A.w_lr <= LR_MAX_RANK && A.w_lr2 >= 0 && A.w_lr2 <= LR_MAX_RANK && A.w_lrc >= 1 && A.w_lrc <= LR_MAX_RANK + 1 &&
           A.w_lrb >= 0 && A.w_lrb <= 2 * LR_MAX_RANK + 1 && (A.xcorr_only || A.w_lrb >= 1) && A.km >= 1 && A.kn >= 1 && A.km <= 81 &&
           A.kn <= 81 && lr_smem(A.km, A.kn, A.mask_mode != 0, 1) <= 160 * 1024;
}

// 0: launched; kLaunchNoFit: the template is not one this kernel takes; kLaunchNeedMap: neither a map nor a candidate sink (or an
// argument table of the multi-block tile launch is wanted); kLaunchDeclined: a signal layout read by other kernels (bands of counts,
// lazily evaluated bands).
// Nothing is launched on a non-zero return, and A is left as it was.
int launch_corr_lowrank_f32(const CorrArgs<float>& A_in, hipStream_t stream)
{
    if (!corr_lowrank_supports(A_in)) return kLaunchNoFit;
    if (A_in.sig.counts || A_in.sig.layout == 2) return kLaunchDeclined;
    if (A_in.defer_args) return kLaunchNeedMap;
    const bool sink = !A_in.out.ptr && A_in.cand_keys && A_in.cand_count && A_in.ks.cand_cmin > 0.0f;
    if (!A_in.out.ptr && !sink) return kLaunchNeedMap;
    CorrArgs<float> A = A_in;
    A.tile_w = LR_TW;
    A.tile_h = LR_TH;
    A.tiles_y = (A.row_end - A.row_begin + LR_TH - 1) / LR_TH;
    if (A.out.layout == 1) {
        A.out_lo = A.out.band_lo;
        A.out_hi = A.out.band_lo + A.out.band_w - 1;
        const long long span = (long long)(A.out_hi - A.out_lo) + LR_TH + LR_TW - 1;
        A.tiles_x = (int)(span / LR_TW) + 2;
        const int max_x = (A.ns + LR_TW - 1) / LR_TW;
        if (A.tiles_x > max_x) A.tiles_x = max_x;
    } else {
        A.out_lo = -(1 << 30);
        A.out_hi = (1 << 30);
        A.tiles_x = (A.ns + LR_TW - 1) / LR_TW;
    }
    if (sink) {
        // only the scanned diagonals (the map path trims in the compaction); a tile list indexes another grid: every tile is walked
        // and the entry filters the candidates of unlisted tiles
        A.out_lo = std::max(A.out_lo, A.cand_dlo);
        A.out_hi = std::min(A.out_hi, A.cand_dhi);
        if (A.out_lo > A.out_hi) return 0;
    } else {
        A.cand_keys = nullptr;
    }
    A.cand_tiles = nullptr;
    A.cand_n_tiles = 0;
    if (A.tiles_x <= 0 || A.tiles_y <= 0) return 0;
    if (A.tiles_y > 65535) return kLaunchNoFit;
    const bool masked = A.mask_mode != 0;
    // planes per round: as many as keep two workgroups on a CU (80 KiB), else as many as fit one
    int nq = 4;
    while (nq > 1 && lr_smem(A.km, A.kn, masked, nq) > 80 * 1024) --nq;
    if (nq == 1)
        for (nq = 4; nq > 1 && lr_smem(A.km, A.kn, masked, nq) > 160 * 1024;) --nq;
    const size_t smem = lr_smem(A.km, A.kn, masked, nq);
    if (smem > 160 * 1024) return kLaunchNoFit;
    const void* kern = masked ? (const void*)corr_lowrank_kernel<true> : (const void*)corr_lowrank_kernel<false>;
    if (smem > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return (int)e;
    }
    dim3 grid(A.tiles_x, A.tiles_y), block(512);
    if (masked) hipLaunchKernelGGL(corr_lowrank_kernel<true>, grid, block, smem, stream, A, nq);
    else hipLaunchKernelGGL(corr_lowrank_kernel<false>, grid, block, smem, stream, A, nq);
    return (int)hipGetLastError();
}

}  // namespace cs
