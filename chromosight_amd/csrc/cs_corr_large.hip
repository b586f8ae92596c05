// cs_corr_large.hip -- sliding-window correlation on the matrix cores for templates with a side of 34 .. 81.
//
// The float32 class of the candidate calls (cs_candidates, cs_candidates_tiles, the detect flow) for the templates the
// 64 x 64-tile kernels cannot hold: the 81 x 81 `centromeres` template, `--win-size` and API templates of 34 .. 81, square or
// rectangular; any container (dense / band, float32 / float64), per-bin or explicit masks, row windows, full and valid modes.
// Map calls (n_obs, plain cross-correlations) run here only when asked for (CHROMOSIGHT_HIP_LARGE=1, cs_api.cpp).
// Same recasting as cs_corr_wide.hip (v_mfma_f32_16x16x32_f16, float16 head / tail pairs after a power-of-two scale per tile,
// float32 accumulation), with what the larger template changes:
//
//   * a 16-column output tile of a template row of kn weights reads 16 + kn - 1 staged columns: NP = ceil((kn + 15) / 32)
//     k = 32 Toeplitz passes per template row (B_p[k][n] = W[s][32 p + k - n]; NP = 2 up to kn = 49, 3 up to 81).  The A block
//     of pass p of column tile c is the block at column 16 (c + 2 p), so a wave reads 4 + 2 (NP - 1) head and as many tail
//     blocks per template row and issues 3 NP MFMAs per column tile (heads x heads, heads x tails, tails x heads);
//   * 64 x 64 output pixels stage (64 + 80)^2 pixels: float16 planes of 144 rows x 152 halfs (pitch 304 B = 19 16-byte slots,
//     odd: the 16 rows a ds_read_b128 group reads hit 16 distinct slots).  42.8 KB per plane: heads + tails 86 KB, 128 KB with
//     the 0/1 mask plane -- one workgroup per CU.  Staging is pixel by pixel with the full missing predicate (cs_device.h
//     missing_from_flags): 81 pixels per thread, the loads issued together; at 6561 multiply-adds per pixel the kernel is
//     bound by its MFMAs, not by the staging;
//   * km x NP x {head, tail} x 1 KiB of B fragments per weight set (1.5 MB for three sets at 81 x 81, L2-resident) are loaded
//     from global memory one template row ahead (image: cs_api.cpp ensure_wfrag_large);
//   * box sums (sum x, sum x^2, missing pixels) as in cs_corr_wide.hip: a horizontal all-ones Toeplitz pass over the wave's
//     15 + km input rows whose accumulators are the B operand of the vertical pass.  A scaled pixel is below 128, so a row of
//     81 squares / 32 stays below 41 472 and its float16 head is finite;
//   * masks: the missing predicate of every staged pixel is the 0/1 plane, and the mask-weighted template sums are two more
//     correlations of that plane (Wa, Wb).  16 x 16 blocks of the plane without a flagged pixel are skipped;
//   * a tile list (CorrArgs::cand_tiles, cs_candidates_tiles on a dense map): the workgroups take their tiles from it.
//
// One workgroup (4 waves) = one 64 x 64 output tile; wave w owns rows 16 w .. 16 w + 15 and four 16-column tiles.
#include "cs_device.h"
#include <algorithm>
#include <mutex>
#include <utility>
#include <vector>

#include "cs_launch.h"

namespace cs {

namespace {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int LG_T = 64;                      // output tile edge
constexpr int LG_R = 144;                     // staged rows / columns (tile + 80)
constexpr int LG_P = 152;                     // halfs per staged row
constexpr int LG_PLANE = LG_R * LG_P * 2;     // bytes of one float16 plane
constexpr int LG_PER_THREAD = (LG_R * LG_R) / 256;      // 81 staged pixels per thread
constexpr int LG_NRB = LG_R / 16;             // 16-row (16-column) blocks of the staged square
constexpr int LG_RED = 16 * 4;                // maximum, occupancy words of the plane (one per 16-row block)
constexpr int LG_SMEM_PLAIN = 2 * LG_PLANE + LG_RED;
constexpr int LG_SMEM_MASKED = 3 * LG_PLANE + LG_RED;
static_assert(LG_R * LG_R == 256 * LG_PER_THREAD, "staging loop");
static_assert(LG_SMEM_MASKED <= 160 * 1024, "one workgroup per CU");
static_assert(16 * 7 + 32 <= LG_R, "the blocks of three passes stay inside the staged columns");

__device__ __forceinline__ f4 mfma16(const h8& a, const h8& b, const f4& c)
{
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ h8 as_h8(const uint4& v) { return __builtin_bit_cast(h8, v); }

// the head / tail float16 pair of four float32 sums as the LOWER half of a B operand (slots e = 0 .. 3; 4 .. 7 zero)
__device__ __forceinline__ void split_low(const f4& v, h8& hi, h8& lo)
{
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const _Float16 h = (_Float16)v[e];
        hi[e] = h;
        lo[e] = (_Float16)(v[e] - (float)h);
        hi[e + 4] = (_Float16)0.0f;
        lo[e + 4] = (_Float16)0.0f;
    }
}

// candidate mode: windows far below the tile's scale are outside the error model of the float16 pairs
// (cs_corr_mfma.hip cand_range_guard)
__device__ __forceinline__ float large_range_guard(float r, float s2, float unscale, const KernelStats<float>& K)
{
    if (K.cand_cmin > 0.0f) r = ((int)(s2 > 0.0f) & (int)(s2 < K.n * (unscale * unscale) * 0.0625f)) ? 2.0f : r;
    return r;
}

}  // namespace

template <bool MASKED, int NP>
__global__ __launch_bounds__(256, 1) void corr_mfma_large_kernel(const CorrArgs<float> A, const MfmaLargeWeights E)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    _Float16* xh = reinterpret_cast<_Float16*>(smem);
    _Float16* xl = reinterpret_cast<_Float16*>(smem + LG_PLANE);
    _Float16* xm = reinterpret_cast<_Float16*>(smem + 2 * LG_PLANE);                      // MASKED only
    unsigned* red = reinterpret_cast<unsigned*>(smem + (MASKED ? 3 : 2) * LG_PLANE);     // [0] maximum, [1 + rb] plane blocks

    const int tid = threadIdx.x;
    const int lane = tid & 63, wv = tid >> 6;
    const int n = lane & 15, g = lane >> 4;
    const bool band_out = A.out.layout == 1;
    // ---- tile of this workgroup: XCD x (workgroups x, x + 8, ...) takes the x-th eighth of the tile list (row-major grid,
    //      or the caller's list of grid indices)
    const int n_tiles = A.cand_tiles ? A.cand_n_tiles : A.tiles_x * A.tiles_y;
    const int per = (int)gridDim.x >> 3;
    const int slot = (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
    if (slot >= n_tiles) return;
    const int t = A.cand_tiles ? A.cand_tiles[slot] : slot;
    if (t < 0 || t >= A.tiles_x * A.tiles_y) return;
    const int by = t / A.tiles_x;
    const int bx = t - by * A.tiles_x;
    const int I0 = A.row_begin + by * LG_T;
    if (I0 >= A.row_end) return;
    const int J0 = band_out ? I0 + A.out_lo + bx * LG_T : bx * LG_T;
    if (J0 >= A.ns || J0 + LG_T <= 0) return;
    if (J0 + LG_T - 1 - I0 < A.out_lo || J0 - (I0 + LG_T - 1) > A.out_hi) return;   // no produced diagonal
    const int km = A.km, kn = A.kn;
    const int RH = LG_T - 1 + km, RW = LG_T - 1 + kn;            // staged rows / columns the tile's windows reach
    const int P0 = I0 - (km - 1) / 2, Q0 = J0 - (kn - 1) / 2;
    // rows no window of the row range [row_begin, row_end) reaches are not part of the input contract
    const int p_lo = A.row_begin - (km - 1) / 2, p_hi = A.row_end + (km - 1) - (km - 1) / 2;

    if (tid < LG_RED / 4) red[tid] = 0u;
    const unsigned char* flags_r = A.miss_row;
    const unsigned char* flags_c = A.miss_col;

    // ---- stage 144 x 144 pixels, one at a time from clamped addresses, with the missing predicate in full.  First pass: the
    //      float32 value (0 at missing pixels) parks its upper / lower 16 bits in the head / tail planes and the predicate goes to
    //      the mask plane; second pass, after the tile's maximum is known: the same thread splits its own pixels in place (no
    //      array of 81 values in registers: the masked instances kept it in scratch)
    float amax = 0.0f;
#pragma unroll 9
    for (int k = 0; k < LG_PER_THREAD; ++k) {
        const int idx = tid + 256 * k;
        const int r = idx / LG_R, c = idx - r * LG_R;
        const int p = P0 + r, q = Q0 + c;
        const bool inside = (r < RH) & (c < RW) & (p >= 0) & (p < A.ms) & (q >= 0) & (q < A.ns) & (p >= p_lo) & (p < p_hi);
        const long long off = inside ? mat_offset(A.sig, p, q) : -1;
        const long long o = off >= 0 ? off : 0;            // element 0 of the buffer always exists
        float x = A.sig_is_f64 ? (float)reinterpret_cast<const double*>(A.sig.ptr)[o] : reinterpret_cast<const float*>(A.sig.ptr)[o];
        if (off < 0) x = 0.0f;
        const int ol = r * LG_P + c;
        if constexpr (MASKED) {
            bool mval = false, fr = false, fc = false;
            if (A.mask_mode == 2) {
                const long long om = inside ? mat_offset(A.mask, p, q) : -1;
                const unsigned char mv = reinterpret_cast<const unsigned char*>(A.mask.ptr)[om >= 0 ? om : 0];
                mval = om >= 0 && mv != 0;
            } else if (A.mask_mode == 1) {
                fr = flags_r[min(max(p, 0), A.ms - 1)] != 0;
                fc = flags_c[min(max(q, 0), A.ns - 1)] != 0;
            }
            const bool needed = (r < RH) & (c < RW) & (p >= p_lo) & (p < p_hi);
            // (mval: the explicit map's byte where the map stores the pixel, so `stored` has nothing left to say)
            const bool miss = needed && missing_from_flags(A, p, q, fr, fc, mval, true);
            if (miss) x = 0.0f;          // the reference requires 0 at missing pixels (check_missing_mask); enforce it
            reinterpret_cast<unsigned short*>(xm)[ol] = miss ? 0x3c00u : 0u;         // 0x3c00 = 1.0 in float16
        }
        const unsigned b = __float_as_uint(x);
        reinterpret_cast<unsigned short*>(xh)[ol] = (unsigned short)(b >> 16);
        reinterpret_cast<unsigned short*>(xl)[ol] = (unsigned short)(b & 0xffffu);
        amax = fmaxf(amax, fabsf(x));
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) amax = fmaxf(amax, __shfl_xor(amax, off));
    __syncthreads();      // the zeroed words and the mask plane are in LDS
    if (lane == 0) atomicMax(&red[0], __float_as_uint(amax));
    if constexpr (MASKED) {
        // 16 x 16 blocks of the plane that hold a 1: bit cb of word 1 + rb, one thread per block
        if (tid < LG_NRB * LG_NRB) {
            const int rb = tid / LG_NRB, cb = tid - rb * LG_NRB;
            unsigned any = 0u;
            for (int r = 16 * rb; r < 16 * rb + 16; ++r) {
                const uint4* row = reinterpret_cast<const uint4*>(xm + r * LG_P + 16 * cb);
                const uint4 a = row[0], b = row[1];
                any |= a.x | a.y | a.z | a.w | b.x | b.y | b.z | b.w;
            }
            if (any) atomicOr(&red[1 + rb], 1u << cb);
        }
    }
    __syncthreads();
    int ex = 0;
    {
        const int e = (int)((red[0] >> 23) & 0xffu);
        if (e != 0 && e != 255) ex = 6 - (e - 127);
        ex = max(-100, min(100, ex));
    }
    const float scale = __uint_as_float((unsigned)(ex + 127) << 23);
    const float unscale = __uint_as_float((unsigned)(127 - ex) << 23);
    // (the occupancy words stay in LDS: read with a wave-uniform address where they are needed)
    const unsigned* occ = red + 1;
    bool any_occ = false;
    if constexpr (MASKED) {
        unsigned any = 0u;
#pragma unroll
        for (int rb = 0; rb < LG_NRB; ++rb) any |= occ[rb];
        any_occ = __builtin_amdgcn_readfirstlane((int)any) != 0;
    }
    // heads by rounding, tails exact differences: head + tail carries 22 bits
#pragma unroll 9
    for (int k = 0; k < LG_PER_THREAD; ++k) {
        const int idx = tid + 256 * k;
        const int r = idx / LG_R, c = idx - r * LG_R;
        const int ol = r * LG_P + c;
        unsigned short* uh = reinterpret_cast<unsigned short*>(xh) + ol;
        unsigned short* ul = reinterpret_cast<unsigned short*>(xl) + ol;
        const float xs = __uint_as_float(((unsigned)*uh << 16) | (unsigned)*ul) * scale;
        const _Float16 h = (_Float16)xs;
        xh[ol] = h;
        xl[ol] = (_Float16)(xs - (float)h);
    }
    __syncthreads();

    const f4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
    const int wr0 = 16 * wv;                  // first staged row of the wave's windows
    // the 16 x 16 pixel blocks of this wave that hold a produced pixel: a wave without one has nothing left to do (no barrier follows)
    unsigned cmask = 0;
    {
        const int i_lo = I0 + wr0, i_hi = min(I0 + wr0 + 15, A.row_end - 1);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int j_lo = max(J0 + 16 * c, 0), j_hi = min(J0 + 16 * c + 15, A.ns - 1);
            if (i_lo <= i_hi && j_lo <= j_hi && j_hi - i_lo >= A.out_lo && j_lo - i_hi <= A.out_hi) cmask |= 1u << c;
        }
    }
    if (cmask == 0u) return;
    constexpr int NCB = 4 + 2 * (NP - 1);     // 16-column steps at which a wave's A blocks (16 rows x 32 columns) start
    const bool any_mask = MASKED && any_occ;

    // ---- box sums.  Horizontal pass per 16-row block rb of the wave's 15 + km input rows (all-ones Toeplitz operands
    //      B_p[k][n] = 1 for 0 <= 32 p + k - n < kn); its accumulators (lane (n, g): rows 16 rb + 4 g + v of column n) go straight
    //      back in as the B operand of the vertical pass, slots e = 0 .. 3 of k = 8 g + e labelled as row 16 rb + 4 g + e:
    //      A[m][8 g + e] = 1 for 0 <= 16 rb + 4 g + e - m < km
    f4 S1[4], S2[4], NM[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) S1[c] = S2[c] = NM[c] = zero4;
    const int n_rb = (km + 30) / 16;
    for (int rb = 0; rb < n_rb; ++rb) {
        f4 a1[4], a2[4], am_[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) a1[c] = a2[c] = am_[c] = zero4;
        const int rowoff = (wr0 + 16 * rb + n) * LG_P + 8 * g;
        const unsigned ro = MASKED ? (unsigned)__builtin_amdgcn_readfirstlane((int)occ[min((wr0 >> 4) + rb, LG_NRB - 1)]) : 0u;
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) {
            const h8 ah = *reinterpret_cast<const h8*>(xh + rowoff + 16 * cb);
            const h8 al = *reinterpret_cast<const h8*>(xl + rowoff + 16 * cb);
            // squares as float16 pairs in packed float16 arithmetic (cs_corr_wide.hip): x^2 / 32 = (xh^2 + 2 xh xl) / 32 up to
            // xl^2 (2^-22 of it)
            const h8 ts = ah * (_Float16)0.03125f;
            const h8 qh = ts * ah;
            h8 ql = __builtin_elementwise_fma(ts, ah, -qh);
            ql = __builtin_elementwise_fma(ts + ts, al, ql);
            h8 am;
            const bool mblk = MASKED && any_mask && (ro & (3u << cb));
            if (mblk) am = *reinterpret_cast<const h8*>(xm + rowoff + 16 * cb);
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const int c = cb - 2 * p;
                if (c < 0 || c > 3) continue;
                h8 ones_b;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int t0 = 32 * p + 8 * g + e - n;
                    ones_b[e] = (t0 >= 0 && t0 < kn) ? (_Float16)1.0f : (_Float16)0.0f;
                }
                a1[c] = mfma16(ah, ones_b, a1[c]);
                a1[c] = mfma16(al, ones_b, a1[c]);
                a2[c] = mfma16(qh, ones_b, a2[c]);
                a2[c] = mfma16(ql, ones_b, a2[c]);
                if (mblk) am_[c] = mfma16(am, ones_b, am_[c]);
            }
        }
        h8 ones_a;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int d = 16 * rb + 4 * g + e - n;
            ones_a[e] = (e < 4 && d >= 0 && d < km) ? (_Float16)1.0f : (_Float16)0.0f;
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            h8 bh, bl;
            split_low(a1[c], bh, bl);
            S1[c] = mfma16(ones_a, bh, S1[c]);
            S1[c] = mfma16(ones_a, bl, S1[c]);
            split_low(a2[c], bh, bl);
            S2[c] = mfma16(ones_a, bh, S2[c]);
            S2[c] = mfma16(ones_a, bl, S2[c]);
            if (MASKED && any_mask) {
                split_low(am_[c], bh, bl);          // (counts of up to 81: exact in the head)
                NM[c] = mfma16(ones_a, bh, NM[c]);
            }
        }
    }

    // ---- cross term: per template row the wave's NCB head and tail blocks against the row's NP Toeplitz fragment pairs,
    //      loaded from the image in global memory one row ahead
    f4 accM[4], accC[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) accM[c] = accC[c] = zero4;
    {
        const uint4* F = E.frag + lane;                   // [set 0][s][pass][head | tail][lane]
        uint4 nf[2 * NP];
#pragma unroll
        for (int q = 0; q < 2 * NP; ++q) nf[q] = F[q * 64];
        for (int s = 0; s < km; ++s) {
            uint4 cf[2 * NP];
#pragma unroll
            for (int q = 0; q < 2 * NP; ++q) cf[q] = nf[q];
            {
                const uint4* Fn = F + (size_t)min(s + 1, km - 1) * (2 * NP * 64);
#pragma unroll
                for (int q = 0; q < 2 * NP; ++q) nf[q] = Fn[q * 64];
            }
            const int rowoff = (wr0 + s + n) * LG_P + 8 * g;
            h8 ah[NCB], al[NCB];
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) {
                ah[cb] = *reinterpret_cast<const h8*>(xh + rowoff + 16 * cb);
                al[cb] = *reinterpret_cast<const h8*>(xl + rowoff + 16 * cb);
            }
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const h8 bh = as_h8(cf[2 * p]), bl = as_h8(cf[2 * p + 1]);
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    accM[c] = mfma16(ah[c + 2 * p], bh, accM[c]);
                    accC[c] = mfma16(ah[c + 2 * p], bl, accC[c]);
                    accC[c] = mfma16(al[c + 2 * p], bh, accC[c]);
                }
            }
        }
    }

    // ---- mask-weighted template sums: the plane against the Wa and the Wb fragments (the plane is exact in float16: two
    //      MFMAs per block, pass and set); blocks whose 16 x 16 sub-blocks hold no flagged pixel are skipped
    f4 KA[4], KB[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) KA[c] = KB[c] = zero4;
    if constexpr (MASKED) {
        if (any_mask) {
#pragma unroll
            for (int set = 1; set <= 2; ++set) {
                const uint4* F = E.frag + (size_t)set * km * (2 * NP * 64) + lane;
                for (int s = 0; s < km; ++s) {
                    // occupied 16-column blocks among the (one or two) 16-row blocks the rows wr0 + s .. wr0 + s + 15 touch
                    const int r0 = wr0 + s;
                    const unsigned ro = (unsigned)__builtin_amdgcn_readfirstlane((int)(occ[r0 >> 4] | occ[min((r0 + 15) >> 4, LG_NRB - 1)]));
                    if (ro == 0u) continue;
                    const uint4* Fs = F + (size_t)s * (2 * NP * 64);
                    uint4 cf[2 * NP];
#pragma unroll
                    for (int q = 0; q < 2 * NP; ++q) cf[q] = Fs[q * 64];
                    const int rowoff = (r0 + n) * LG_P + 8 * g;
#pragma unroll
                    for (int cb = 0; cb < NCB; ++cb) {
                        if (!(ro & (3u << cb))) continue;        // (block cb covers the 16-column blocks cb and cb + 1)
                        const h8 am = *reinterpret_cast<const h8*>(xm + rowoff + 16 * cb);
#pragma unroll
                        for (int p = 0; p < NP; ++p) {
                            const int c = cb - 2 * p;
                            if (c < 0 || c > 3) continue;
                            const h8 wh = as_h8(cf[2 * p]), wl = as_h8(cf[2 * p + 1]);
                            if (set == 1) {
                                KA[c] = mfma16(am, wh, KA[c]);
                                KA[c] = mfma16(am, wl, KA[c]);
                            } else {
                                KB[c] = mfma16(am, wh, KB[c]);
                                KB[c] = mfma16(am, wl, KB[c]);
                            }
                        }
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                KA[c] *= E.unscale[1];
                KB[c] *= E.unscale[2];
            }
        }
    }

    // ---- epilogue: lane = column n of tile c, rows 4 g + v
    const float u_cs = unscale * E.unscale[0];
    const float u_s2 = 32.0f * unscale;
    const int kh = (km - 1) / 2, kw = (kn - 1) / 2;
    // a tile all of whose 64 x 64 pixels are produced and none forced to zero (cs_device.h pixel_forced_zero): no per-pixel
    // predicates, addresses by increments
    const int dmin_t = J0 - (I0 + LG_T - 1), dmax_t = J0 + LG_T - 1 - I0;
    const bool same_nobs = !A.nobs.ptr || (A.nobs.layout == A.out.layout && A.nobs.ld == A.out.ld && A.nobs.band_lo == A.out.band_lo &&
                                           A.nobs.band_w == A.out.band_w && A.nobs.row0 == A.out.row0);
    const bool plain = I0 + LG_T <= A.row_end && J0 >= 0 && J0 + LG_T <= A.ns && dmin_t >= A.out_lo && dmax_t <= A.out_hi && same_nobs &&
                       (A.full || (I0 >= kh && I0 + LG_T - 1 <= A.ms - km + kh && J0 >= kw && J0 + LG_T - 1 <= A.ns - kn + kw)) &&
                       (!A.sym_upper || dmin_t + (A.full ? kn - km : 0) >= 0) &&
                       (!band_out || (dmin_t >= A.out.band_lo && dmax_t < A.out.band_lo + A.out.band_w));
    const int i_lane = I0 + wr0 + 4 * g, j_lane = J0 + n;
    const long long o_lane = ((long long)i_lane - A.out.row0) * A.out.ld + (band_out ? j_lane - i_lane - A.out.band_lo : j_lane);
    const long long o_row = band_out ? A.out.ld - 1 : A.out.ld;
    // the window sums of pixel (c, v) -> coefficient (cs_device.h: the one-rsq form, the literal function next to a zeroing threshold)
    auto coefficient = [&](int c, int v, float& nobs) -> float {
        const float cs = (accM[c][v] + accC[c][v]) * u_cs;
        const float s1 = S1[c][v] * unscale;
        const float s2 = (S2[c][v] * u_s2) * unscale;
        nobs = A.ks.n;
        float r;
        if (A.xcorr_only) {
            r = (fabsf(cs) < A.ks.thr) ? 0.0f : cs;
        } else if constexpr (MASKED) {
            const float nm = NM[c][v];
            r = large_range_guard(pearson_masked_lean(cs, s1, s2, nm, KA[c][v], KB[c][v], A.ks), s2, unscale, A.ks);
            nobs = A.ks.n - nm;
        } else {
            r = large_range_guard(pearson_nomask_lean(cs, s1, s2, A.ks), s2, unscale, A.ks);
        }
        return r;
    };
    // candidate sink (cs_device.h CorrArgs::cand_keys): no map leaves the kernel, only the keys tag + row * ns + col of the pixels
    // that carry a candidate value (>= cand_thr: the screen's sentinel included), appended to the caller's list; the counter runs
    // on beyond the capacity so that the caller learns how much room a second call needs
    const bool sinking = A.cand_keys != nullptr;
    auto sink = [&](int i, int j, float r) {
        if (r >= A.ks.cand_thr) {
            const unsigned long long pos = atomicAdd(A.cand_count, 1ull);
            if (pos < (unsigned long long)A.cand_cap)
                A.cand_keys[pos] = A.cand_tag + (unsigned long long)i * (unsigned long long)A.ns + (unsigned long long)j;
        }
    };
    if (plain) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                float nobs;
                const float r = coefficient(c, v, nobs);
                if (sinking) {
                    sink(i_lane + v, j_lane + 16 * c, r);
                    continue;
                }
                const long long o = o_lane + v * o_row + 16 * c;
                if (A.out_is_f64) reinterpret_cast<double*>(A.out.ptr)[o] = (double)r;
                else reinterpret_cast<float*>(A.out.ptr)[o] = r;
                if (A.nobs.ptr) reinterpret_cast<float*>(A.nobs.ptr)[o] = nobs;
            }
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (!((cmask >> c) & 1u)) continue;
            const int j = J0 + 16 * c + n;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int i = I0 + wr0 + 4 * g + v;
                if (i >= A.row_end || j < 0 || j >= A.ns) continue;
                const int d = j - i;
                if (d < A.out_lo || d > A.out_hi) continue;
                float nobs;
                const float r = coefficient(c, v, nobs);
                if (sinking) {
                    if (!pixel_forced_zero(A, i, j)) sink(i, j, r);
                    continue;
                }
                store_pixel(A, i, j, pixel_forced_zero(A, i, j) ? 0.0f : r, nobs);
            }
        }
    }
}

// The 160 KB dynamic-LDS ceiling is a per-function, per-device attribute: set it the first time a kernel is
// launched on a device.
static hipError_t large_allow_big_lds(const void* fn)
{
    static std::mutex mu;
    static std::vector<std::pair<const void*, int>> done;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lock(mu);
    for (const auto& d : done)
        if (d.first == fn && d.second == dev) return hipSuccess;
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e == hipSuccess) done.emplace_back(fn, dev);
    return e;
}

bool corr_mfma_large_fits(int km, int kn) { return km >= 1 && kn >= 1 && km <= 81 && kn <= 81 && std::max(km, kn) >= 34; }

int corr_mfma_large_passes(int kn) { return kn + 15 <= 64 ? 2 : 3; }

int launch_corr_mfma_large_f32(CorrArgs<float>& A, const MfmaLargeWeights& E, hipStream_t stream)
{
    if (!corr_mfma_large_fits(A.km, A.kn)) return kLaunchNoFit;
    if (A.sig.counts || A.sig.layout == 2) return kLaunchDeclined;      // (bands of counts / lazily evaluated bands: other readers)
    if (!A.out.ptr && !(A.cand_keys && A.cand_count && A.ks.cand_cmin > 0.0f)) return kLaunchNeedMap;      // a map, or a candidate sink
    if (A.defer_args) return kLaunchNeedMap;                           // (argument tables of the multi-block launch: the 17 x 17 tile kernel only)
    if (E.passes != corr_mfma_large_passes(A.kn)) return kLaunchNoFit;
    A.tile_w = A.tile_h = LG_T;
    A.tiles_y = (A.row_end - A.row_begin + LG_T - 1) / LG_T;
    if (A.out.layout == 1) {
        A.out_lo = A.out.band_lo;
        A.out_hi = A.out.band_lo + A.out.band_w - 1;
        A.tiles_x = (A.out.band_w + LG_T - 1 + LG_T - 1) / LG_T;
    } else {
        A.out_lo = -(1 << 30);
        A.out_hi = (1 << 30);
        A.tiles_x = (A.ns + LG_T - 1) / LG_T;
    }
    if (A.cand_keys && !A.out.ptr) {
        // candidate sink: only the scanned diagonals (the map path trims in the compaction)
        A.out_lo = std::max(A.out_lo, A.cand_dlo);
        A.out_hi = std::min(A.out_hi, A.cand_dhi);
    } else {
        A.cand_keys = nullptr;                             // (a map was asked for: the kernel writes it)
    }
    // a tile list indexes the dense 64 x 64 grid of the row window (cs_candidates_tiles); other calls walk the whole grid
    if (!A.cand_keys || A.out.layout != 0) A.cand_tiles = nullptr;
    if (!A.cand_tiles) A.cand_n_tiles = 0;
    const long long blocks = A.cand_tiles ? (long long)A.cand_n_tiles : (long long)A.tiles_x * A.tiles_y;
    if (blocks <= 0) return 0;
    if (blocks > 0x7ffffff0LL) return kLaunchNoFit;
    const bool masked = A.mask_mode != 0;
    typedef void (*kern_t)(const CorrArgs<float>, const MfmaLargeWeights);
    const kern_t k = masked ? (E.passes == 3 ? corr_mfma_large_kernel<true, 3> : corr_mfma_large_kernel<true, 2>)
                            : (E.passes == 3 ? corr_mfma_large_kernel<false, 3> : corr_mfma_large_kernel<false, 2>);
    hipError_t e = large_allow_big_lds((const void*)k);
    if (e != hipSuccess) return (int)e;
    const unsigned grid = (unsigned)((blocks + 7) / 8 * 8);
    hipLaunchKernelGGL(k, dim3(grid), dim3(256), masked ? LG_SMEM_MASKED : LG_SMEM_PLAIN, stream, A, E);
    return (int)hipGetLastError();
}

}  // namespace cs
