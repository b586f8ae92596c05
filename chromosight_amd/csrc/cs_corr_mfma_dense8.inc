// cs_corr_mfma_dense8.inc -- the dense 17 x 17 tile kernel at four waves per SIMD (cs_corr_mfma.hip includes this file once, at
// namespace scope, behind the helpers of the dense instances).
//
// The unmasked dense float32 map with 16-byte transfers and a 17 x 17 template whose rows mirror -- the headline configuration --
// is bound by the instruction issue of ONE wave: corr_mfma_dense_kernel<true, false> holds 243 registers, so two waves sit on a
// SIMD and every phase of the tile loop is a latency chain with one partner to hide behind (DESIGN.md 7.5).  This instance keeps
// the workgroup's 64 x 64 tile, its LDS image and its tile order, and runs it with EIGHT waves: wave w owns rows 16 (w & 3) and
// the two column tiles at column 32 (w >> 2).  Fragments, accumulators and the deferred epilogue state halve, the heads of the
// weights move to LDS (the mirrored 9 + 9 row layout of the masked RSYM instance), the stores need no LDS scratch (see emit), and
// the kernel fits 128 registers: two workgroups per CU are four waves per SIMD.  Every pixel sees the operations of the
// 4-wave instance in the same order; the one decision taken per WAVE -- the lean or the literal form of the coefficient -- now
// covers 16 x 32 pixels instead of 16 x 64.
//
// Twice the waves repeat what a wave does per tile beside its MFMAs, so that part is kept short (DESIGN.md "The 8-wave dense
// kernel: what each wave repeats per tile"): the tile walk is carried without divisions (DenseTileWalk), no staging lane is
// masked, the wave maximum runs on bit patterns (wave_max_bits).  What a launch fixes -- plain cross-correlation or coefficient,
// float32 or float64 output -- is a template parameter, and an inner tile's transfers and stores go through a buffer descriptor
// whose base the scalar unit forms per tile, with 32-bit lane offsets formed once (Dense8Offsets).  None of it changes a value.

constexpr int MF8_ROWS_PER_THREAD = 7;          // staging: 480 threads = 40 column pairs x 12 row groups
constexpr int MF8_RED = MFD_WL + 18 * 1024;     // four planes, 9 tail + 9 head rows of weights, then the 8 wave maxima
constexpr int MF8_SMEM = MF8_RED + 64;
#ifdef CS_MF_PROFILE
constexpr int MF8_PROF = MF8_SMEM;              // 16 x 8 bytes of per-workgroup phase counters
constexpr int MF8_LAUNCH = MF8_SMEM + 128;
#else
constexpr int MF8_LAUNCH = MF8_SMEM;
#endif
static_assert(MF8_LAUNCH <= 80 * 1024, "two workgroups per CU");

// The tile sequence of one workgroup, carried from tile to tile without a division.  The order is that of the 4-wave instance
// (cs_corr_mfma_body.inc): XCD x takes the tiles [x n / 8, (x + 1) n / 8) of the row-major list and its workgroups walk that
// range side by side, `step` tiles at a time; tile row `by` is skewed by (by * skew) % tiles_x columns (dense_tile_skew).  The
// step is constant per workgroup, so its quotient and remainder by tiles_x, and what they add to the skew, are formed once.
struct DenseTileWalk {
    int tile, tile_end, step;        // position in the row-major tile list, end of the workgroup's range, tiles per step
    int by, bx, sk;                  // tile row, tile column before the skew, (by * skew) % tiles_x
    int tiles_x, d_by, d_bx;         // step = d_by * tiles_x + d_bx
    int d_sk, sk_carry;              // (d_by * skew) % tiles_x; skew % tiles_x: one more tile row when bx wraps

    __host__ __device__ void init(int tiles_x_, int n_tiles, int grid, int xcd_order, int block)
    {
        tiles_x = tiles_x_;
        if ((xcd_order & 1) && grid % 8 == 0) {
            const int x = block & 7, per = (n_tiles + 7) / 8;
            tile = x * per + (block >> 3);
            tile_end = (x + 1) * per < n_tiles ? (x + 1) * per : n_tiles;
            step = grid >> 3;
        } else {
            tile = block;
            tile_end = n_tiles;
            step = grid;
        }
        const int skew = xcd_order >> 1;
        by = tile / tiles_x;
        bx = tile - by * tiles_x;
        sk = (by * skew) % tiles_x;
        d_by = step / tiles_x;
        d_bx = step - d_by * tiles_x;
        d_sk = (d_by * skew) % tiles_x;
        sk_carry = skew % tiles_x;
    }
    __host__ __device__ bool done() const { return tile >= tile_end; }
    __host__ __device__ void advance()
    {
        tile += step;
        bx += d_bx;
        const bool wrap = bx >= tiles_x;
        bx -= wrap ? tiles_x : 0;
        by += d_by + (wrap ? 1 : 0);
        sk += d_sk + (wrap ? sk_carry : 0);          // < 3 tiles_x
        sk -= sk >= tiles_x ? tiles_x : 0;
        sk -= sk >= tiles_x ? tiles_x : 0;
    }
    __host__ __device__ void origin(int row_begin, int& I0, int& J0) const
    {
        int col = bx + sk;
        col -= col >= tiles_x ? tiles_x : 0;
        I0 = row_begin + by * MF_T;
        J0 = col * MF_T;
    }
};

// What does not change from tile to tile in the addresses of an inner tile: a lane's byte offsets from the tile's first staged
// pixel (transfers) and from its first output pixel (stores).  Per tile only a uniform 64-bit base remains, which the scalar
// unit forms; base and offset meet in a buffer descriptor (`buffer_load_dwordx4 ... offen lds`, `buffer_store_dwordx4 ... offen`:
// the form the compiler has for scalar base + 32-bit lane offset with 16-byte pieces; a global_load_lds is given a 64-bit
// lane address whatever the source says).  The offsets are 32-bit: fits() is the launcher's route condition.
struct Dense8Offsets {
    // piece k of thread t is piece p = t + 512 k of the tile's 1600 (80 rows x 20 pieces of 16 bytes): row p / 20, piece p % 20
    __host__ __device__ static unsigned fetch(int t, int k, unsigned ld_in)
    {
        const unsigned p = (unsigned)t + 512u * (unsigned)k, r = p / 20u, c = p - 20u * r;
        return (r * ld_in + 4u * c) * 4u;
    }
    // the plain store of thread t (see emit): row 16 (w & 3) + (n & 7) of the tile, columns 32 (w >> 2) + (n < 8 ? 0 : 16) + 4 g;
    // its second store lies 8 rows below
    __host__ __device__ static unsigned store(int t, unsigned ld_out, unsigned elem)
    {
        const unsigned lane = (unsigned)t & 63u, wv = (unsigned)t >> 6, n = lane & 15u, g = lane >> 4;
        return ((16u * (wv & 3u) + (n & 7u)) * ld_out + 32u * (wv >> 2) + (n < 8u ? 0u : 16u) + 4u * g) * elem;
    }
    // bytes a tile's transfers (80 rows) and plain stores (64 rows) span from their bases: the descriptors' ranges
    __host__ __device__ static unsigned fetch_span(unsigned ld_in) { return ((MF_R - 1) * ld_in + MF_R) * 4u; }
    __host__ __device__ static unsigned store_span(unsigned ld_out, unsigned elem) { return ((MF_T - 1) * ld_out + MF_T) * elem; }
    // every offset and span stays below 2^31 (80 rows of either pitch; elem: bytes of an output value)
    __host__ __device__ static bool fits(long long ld_in, long long ld_out, int elem)
    {
        const long long lim = 1LL << 31;
        return ld_in > 0 && ld_out > 0 && ld_in < lim && ld_out < lim && 80 * ld_in * 4 < lim && 80 * ld_out * elem < lim;
    }
};

// maximum over the wave of the bit patterns of non-negative floats, which order as unsigned integers; valid in lane 63.  The
// integer maximum takes its DPP operand directly: no canonicalisation and no separate move (wave_max_nonneg has both).
__device__ __forceinline__ unsigned wave_max_bits(unsigned v)
{
#define CS_DPP_UMAX(ctrl, rmask) v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, ctrl, rmask, 0xf, true))
    CS_DPP_UMAX(0x111, 0xf);      // row_shr:1
    CS_DPP_UMAX(0x112, 0xf);      // row_shr:2
    CS_DPP_UMAX(0x114, 0xf);      // row_shr:4
    CS_DPP_UMAX(0x118, 0xf);      // row_shr:8   -> lane 15 of every row holds the row's maximum
    CS_DPP_UMAX(0x142, 0xa);      // row_bcast:15 into rows 1 and 3
    CS_DPP_UMAX(0x143, 0xc);      // row_bcast:31 into rows 2 and 3
#undef CS_DPP_UMAX
    return v;
}

// XCORR: plain cross-correlation (A.xcorr_only); F64: float64 output (A.out_is_f64).  The launcher picks the instance.
template <bool XCORR, bool F64>
__global__ __launch_bounds__(512, 4) void corr_mfma_dense8_kernel(const MfmaDenseArgs A)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    typedef __attribute__((address_space(3))) char lds_char;
    char* const pl_xh = smem;
    char* const pl_xl = smem + MF_PLANE;
    char* const pl_qh = smem + 2 * MF_PLANE;
    char* const pl_ql = smem + 3 * MF_PLANE;
    float* const raw = reinterpret_cast<float*>(smem + 2 * MF_PLANE);      // next tile's pixels: aliases the squares
    unsigned* const red = reinterpret_cast<unsigned*>(smem + MF8_RED);
    const int tid = threadIdx.x;
    const int lane = tid & 63, wv = tid >> 6;
    const int n = lane & 15, g = lane >> 4;
    constexpr int K = 17, KH = 8;                // (the launcher routes 17 x 17 templates only)
#ifdef CS_MF_PROFILE
#undef MF_PROF_ADD
#define MF_PROF_ADD(k, v) (prof_lds[k] += (unsigned long long)(v))
    unsigned long long* const prof_lds = reinterpret_cast<unsigned long long*>(smem + MF8_PROF);
    unsigned long long tprev_ = 0;
    unsigned long long wall_ = __builtin_amdgcn_s_memrealtime();      // (MF_WALL: prologue, tile loop, final emit)
    if (tid == 0)
        for (int k = 0; k < 16; ++k) prof_lds[k] = 0;
#endif

    // all-ones Toeplitz operands (see cs_corr_mfma_body.inc): horizontal box sums, and the vertical ones with the contraction
    // slots in the order in which the horizontal pass leaves a column's rows in a lane
    h8 ones_b, ones_p;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int t = 8 * g + e - n;
        ones_b[e] = (t >= 0 && t < K) ? (_Float16)1.0f : (_Float16)0.0f;
        const int rho = (e < 4 ? 4 * g + e : 16 + 4 * g + (e - 4)) - n;
        ones_p[e] = (rho >= 0 && rho < K) ? (_Float16)1.0f : (_Float16)0.0f;
    }
    const f4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
    const int wr0 = 16 * (wv & 3), wc0 = 32 * (wv >> 2);      // the wave's rows and columns of the tile
    // staging: column pair, row group.  Thread t reads and splits the rows rg + 12 k.  No lane is masked: the threads 480 .. 511
    // (rg = 12) repeat rows of row group 0 -- the same pixels give the same maximum, the same four float16 values and the same
    // bytes at the same plane addresses -- and the seventh row, rg + 72, exists for whole waves or not at all: rg <= 7 in the
    // waves 0 .. 4 (threads < 320), rg >= 8 in the others.
    const int c2 = tid % 40, rg = tid / 40;
    static_assert(12 + 12 * (MF8_ROWS_PER_THREAD - 2) < MF_R && 319 / 40 + 72 == MF_R - 1 && 320 / 40 + 72 == MF_R, "staging rows");
    // input rows that windows of [row_begin, row_end) reach and that exist
    const int p_min = max(0, A.row_begin - KH), p_max = min(A.ms, A.row_end + (K - 1) - KH) - 1;

    // every staged pixel of the tile at (I0, J0) exists: its transfers are not clamped and its reader needs no masks
    auto tile_inside = [&](int I0, int J0) {
        const int P0 = I0 - KH, Q0 = J0 - KH;
        return P0 >= p_min && P0 + MF_R - 1 <= p_max && Q0 >= 0 && Q0 + MF_R <= A.ns;
    };
    // LDS-DMA of one tile's 80 x 80 pixels in 16-byte pieces (20 per row): a wave-wide transfer moves 64 consecutive pieces, wave
    // w issues the transfers w, w + 8, ...; a lane's piece advances by 512 pieces -- 25 rows and 12 pieces -- per step.
    const int wv_u = __builtin_amdgcn_readfirstlane(wv);
    // a lane's pieces of an inner tile, as byte offsets from the tile's first staged pixel (the fourth: wave 0 only)
    unsigned f_off[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) f_off[k] = Dense8Offsets::fetch(tid, k, (unsigned)A.ld_in);
    const unsigned f_span = Dense8Offsets::fetch_span((unsigned)A.ld_in);
    auto fetch = [&](int I0, int J0, bool inside) {
        const int P0 = I0 - KH, Q0 = J0 - KH;
        const lds_char* dst = (const lds_char*)(raw) + 1024 * wv_u;
        if (inside) {
            // inner tiles (nearly all): no clamp can bite, a piece's address is the tile's base -- uniform: scalar -- plus
            // the lane's offset of the prologue; the descriptor's range is the tile's 80 rows
            const float* base = A.sig + ((long long)P0 - A.row0_in) * A.ld_in + Q0;
            const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), 0, (int)f_span, 0x00020000);
#pragma unroll
            for (int k = 0; k < 3; ++k)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)(dst + 8192 * k), 16, (int)f_off[k], 0, 0, 0);
            static_assert(7 + 8 * 2 < 25 && 1 + 8 * 3 >= 25, "three transfers per wave, a fourth for wave 0");
            if (wv_u == 0)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)(dst + 8192 * 3), 16, (int)f_off[3], 0, 0, 0);
            return;
        }
        const int e0 = 64 * wv_u + lane;
        int r = e0 / 20, c = e0 - r * 20;
        // clamped addresses; the reader masks what lies outside (ns and the first staged column are multiples of 4: a piece
        // lies inside a row or outside it, never across its end)
#pragma unroll 1
        for (int i = wv_u; i < 25; i += 8) {
            const int p = min(max(P0 + r, p_min), p_max);
            const int q = min(max(Q0 + 4 * c, 0), A.ns - 4);
            const float* src = A.sig + ((long long)p - A.row0_in) * A.ld_in + q;
            __builtin_amdgcn_global_load_lds(src, (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
            dst += 8192;
            c += 12;
            r += 25;
            if (c >= 20) {
                c -= 20;
                r += 1;
            }
        }
    };

    // a lane's plain store of a tile, as a byte offset from the tile's first output pixel
    constexpr int ELEM = F64 ? 8 : 4;
    const unsigned s_off = Dense8Offsets::store(tid, (unsigned)A.ld_out, ELEM);
    const unsigned s_span = Dense8Offsets::store_span((unsigned)A.ld_out, ELEM);

    // Epilogue of one tile (lane = row n of the wave's 16, columns wc0 + 16 c + 4 g + v), run one iteration late: its stores have
    // the whole next tile to retire before the `vmcnt(0)` that awaits the DMA.  The arithmetic is the unmasked epilogue of
    // cs_corr_mfma_body.inc, statement for statement.
    auto emit = [&](int I0, int J0, float unscale, const f4 (&acc)[2], const f4 (&S1)[2], const f4 (&S2)[2]) {
        const float u_cs = unscale * A.w_unscale;
        const float u_s2 = 32.0f * unscale;
        const bool plain = I0 + MF_T <= A.row_end && J0 + MF_T <= A.ns &&
                           (A.full || (I0 >= KH && I0 + MF_T - 1 <= A.ms - K + KH && J0 >= KH && J0 + MF_T - 1 <= A.ns - K + KH)) &&
                           (!A.sym_upper || J0 - (I0 + MF_T - 1) >= 0);
        const int i = I0 + wr0 + n;
        f4 rv[2];
        bool lean = !XCORR && !(A.ks.cand_cmin > 0.0f);
        if (lean) {
            const KernelStats<float>& KS = A.ks;
            const float inv_u = __uint_as_float((254u << 23) - __float_as_uint(unscale));          // 2^ex, exact
            const float t1 = KS.thr_n * inv_u;                          // |s1|, |c| >= thr_n
            const float t2 = (t1 * inv_u) * 0.03125f;                   // s2 >= thr_n
            const float td = (KS.den2_min * inv_u) * inv_u;             // den2 >= den2_min
            const float top = (fmaxf(KS.kvar, 1.0f) * 4294967296.0f) * (unscale * unscale);
            auto normal_or_0 = [](float x) { return x == 0.0f || (x >= 1.17549435e-38f && x <= 3.40282347e38f); };
            lean = normal_or_0(t1) && normal_or_0(t2) && normal_or_0(td) && td > 0.0f && top <= 3.40282347e38f;
            if (lean) {
                const float n32 = 32.0f * KS.n, wu = A.w_unscale;
                bool normal = true;
#pragma unroll
                for (int c = 0; c < 2; ++c) {
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        const float s1 = S1[c][v], s2 = S2[c][v], cw = acc[c][v] * wu;
                        const float den2 = fmaf(s2, n32, -s1 * s1) * KS.kvar;
                        float r = cw * __builtin_amdgcn_rsqf(den2);
                        r = (den2 >= td) ? r : 0.0f;                    // denominator under eps, NaN -> 0
                        rv[c][v] = __builtin_amdgcn_fmed3f(r, -1.0f, 1.0f);
                        normal &= (int)(fabsf(s1) >= t1) & (int)(s2 >= t2) & (int)(fabsf(fmaf(KS.kmean, s1, cw)) >= t1);
                    }
                }
                lean = !__builtin_amdgcn_ballot_w64(!normal);
            }
        }
        if (!lean)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const float cs = acc[c][v] * u_cs;
                const float s1 = S1[c][v] * unscale;
                const float s2 = (S2[c][v] * u_s2) * unscale;
                if constexpr (XCORR) rv[c][v] = fabsf(cs) < A.ks.thr ? 0.0f : cs;       // detection.py:716-722
                else rv[c][v] = cand_range_guard(pearson_nomask_lean(cs, s1, s2, A.ks), s2, unscale, A.ks);
            }
        }
        if (plain) {
            // A lane holds 16 consecutive bytes of ONE row per column tile: stored as they are, an instruction would touch 16 rows
            // with 64 bytes each (4x the cost of the same bytes at consecutive addresses).  The lanes n < 8 trade their second
            // column tile for the first one of the lanes n + 8 -- one DPP row_ror:8 per dword, a DPP row being the 16 lanes of
            // one g -- and every store instruction writes 8 rows x 128 consecutive bytes, without a trip through LDS.
            const bool top8 = n < 8;
            f4 s0, s1;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const float mine = top8 ? rv[1][v] : rv[0][v];
                const float theirs = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, mine), 0x128, 0xf, 0xf, true));
                s0[v] = top8 ? rv[0][v] : theirs;          // rows 0 .. 7:  columns 4 g (own) | 16 + 4 g (of lane n - 8)
                s1[v] = top8 ? theirs : rv[1][v];          // rows 8 .. 15: columns 4 g (of lane n + 8) | 16 + 4 g (own)
            }
            // the tile's first output pixel -- uniform: scalar -- in a descriptor over the tile's 64 rows; the lane's offset is
            // that of the prologue, the 8 rows between its two stores the instruction's scalar offset
            typedef unsigned u4 __attribute__((ext_vector_type(4)));
            char* const ob = reinterpret_cast<char*>(A.out) + (((long long)I0 - A.row0_out) * A.ld_out + J0) * ELEM;
            const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(ob, 0, (int)s_span, 0x00020000);
            const int down8 = 8 * (int)A.ld_out * ELEM;
            if constexpr (F64) {
                typedef double d2 __attribute__((ext_vector_type(2)));
                d2 a, b;
                a[0] = s0[0]; a[1] = s0[1]; b[0] = s0[2]; b[1] = s0[3];
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4, a), ro, (int)s_off, 0, 0);
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4, b), ro, (int)s_off + 16, 0, 0);
                a[0] = s1[0]; a[1] = s1[1]; b[0] = s1[2]; b[1] = s1[3];
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4, a), ro, (int)s_off, down8, 0);
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4, b), ro, (int)s_off + 16, down8, 0);
            } else {
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4, s0), ro, (int)s_off, 0, 0);
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4, s1), ro, (int)s_off, down8, 0);
            }
        } else {
            // tiles on the rim of the map, of the row window, of the valid area or across the diagonal: pixel by pixel
            const long long o_idx = ((long long)i - A.row0_out) * A.ld_out + (J0 + wc0 + 4 * g);
#pragma unroll
            for (int c = 0; c < 2; ++c) {
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int j = J0 + wc0 + 16 * c + 4 * g + v;
                    bool z = false;
                    if (!A.full) z = (i < KH) | (i > A.ms - K + KH) | (j < KH) | (j > A.ns - K + KH);
                    if (A.sym_upper) z = z | ((j - i) < 0);
                    if (i < A.row_end && j < A.ns) {
                        const float val = z ? 0.0f : rv[c][v];
                        if constexpr (F64) reinterpret_cast<double*>(A.out)[o_idx + 16 * c + v] = (double)val;
                        else reinterpret_cast<float*>(A.out)[o_idx + 16 * c + v] = val;
                    }
                }
            }
        }
    };

    f4 p_acc[2], p_S1[2], p_S2[2];
    int p_I0 = 0, p_J0 = 0;
    float p_unscale = 0.0f;
    bool pending = false;
#pragma unroll
    for (int c = 0; c < 2; ++c) p_acc[c] = p_S1[c] = p_S2[c] = zero4;

    // Tile sequence of this workgroup (DenseTileWalk).  A tile's origin and its `inside` are formed once, where its transfers are
    // issued, and handed to the iteration that computes it.
    DenseTileWalk walk;
    walk.init(A.tiles_x, A.n_tiles, (int)gridDim.x, A.xcd_order, (int)blockIdx.x);
    bool have = !walk.done();
    int I0 = 0, J0 = 0;
    bool inside = false;
    if (have) {                                  // the first tile is on its way while the weights are loaded
        walk.origin(A.row_begin, I0, J0);
        inside = tile_inside(I0, J0);
        fetch(I0, J0, inside);
    }

    // ---- weights: nine rows of tails (slots 0 .. 8) and nine rows of heads (slots 9 .. 17) as ready-made fragments; row s > 8 is
    //      row 16 - s.  18 x 64 fragments of 16 bytes, up to three per thread.
    {
        const h8* frag = reinterpret_cast<const h8*>(A.frag);
        h8 wf[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int idx = min(tid + 512 * k, 18 * 64 - 1);
            const int slot = idx >> 6;
            const int row = slot < 9 ? slot : slot - 9, part = slot < 9 ? 1 : 0;
            wf[k] = frag[(2 * row + part) * 64 + (idx & 63)];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int idx = tid + 512 * k;
            if (idx < 18 * 64) reinterpret_cast<h8*>(smem + MFD_WL)[idx] = wf[k];
        }
    }
    MF_WALL(12);
    // waves whose threads stage a seventh row (see c2, rg)
    const bool row7 = wv_u < 5;
    // The waves 4 .. 7 are dispatched behind the waves 0 .. 3 and lose the arbitration by age in every phase: one static priority
    // for that half (s_setprio ignores EXEC: the condition is on a scalar).
    if (wv_u >= 4) __builtin_amdgcn_s_setprio(1);
    while (have) {
        const int P0 = I0 - KH, Q0 = J0 - KH;
#ifdef CS_MF_PROFILE
        tprev_ = __builtin_readcyclecounter();
        if (tid == 0) prof_lds[15] += 1ull;
#endif
        // ---- the tile's pixels have landed in `raw`: read this thread's 7 x 2, find the scale
        __builtin_amdgcn_s_waitcnt(0x0f70);      // vmcnt(0): this wave's DMA transfers (and long-retired stores)
        lds_barrier();                           // everyone's transfers; the previous tile's plane readers are done
        float xa[MF8_ROWS_PER_THREAD], xb[MF8_ROWS_PER_THREAD];
        float amax = 0.0f;
        xa[MF8_ROWS_PER_THREAD - 1] = xb[MF8_ROWS_PER_THREAD - 1] = 0.0f;
        if (inside) {
#pragma unroll
            for (int k = 0; k < MF8_ROWS_PER_THREAD; ++k) {
                if (k < MF8_ROWS_PER_THREAD - 1 || row7) {
                    const float2 v = *reinterpret_cast<const float2*>(raw + (rg + 12 * k) * MF_R + 2 * c2);
                    xa[k] = v.x;
                    xb[k] = v.y;
                    amax = fmaxf(amax, fmaxf(fabsf(v.x), fabsf(v.y)));
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < MF8_ROWS_PER_THREAD; ++k) {
                if (k < MF8_ROWS_PER_THREAD - 1 || row7) {
                    const int r = rg + 12 * k;
                    const float2 v = *reinterpret_cast<const float2*>(raw + r * MF_R + 2 * c2);
                    const int p = P0 + r, q = Q0 + 2 * c2;
                    const bool rok = (p >= p_min) & (p <= p_max);
                    const bool oka = rok & (q >= 0) & (q < A.ns), okb = rok & (q + 1 >= 0) & (q + 1 < A.ns);
                    xa[k] = oka ? v.x : 0.0f;
                    xb[k] = okb ? v.y : 0.0f;
                    amax = fmaxf(amax, fmaxf(fabsf(xa[k]), fabsf(xb[k])));
                }
            }
        }
        const unsigned amax_bits = wave_max_bits(__float_as_uint(amax));
        if (lane == 63) red[wv] = amax_bits;
        MF_STAMP(0);
        lds_barrier();                           // everyone has read `raw`: the squares may overwrite it
        int ex = 0;
        {
            const uint4 m4 = *reinterpret_cast<const uint4*>(red), m8 = *reinterpret_cast<const uint4*>(red + 4);
            const unsigned mx = max(max(max(m4.x, m4.y), max(m4.z, m4.w)), max(max(m8.x, m8.y), max(m8.z, m8.w)));
            const int e = (int)((mx >> 23) & 0xffu);     // (non-negative floats order as integers)
            if (e != 0 && e != 255) ex = 6 - (e - 127);
            ex = max(-100, min(100, ex));
        }
        const float scale = __uint_as_float((unsigned)(ex + 127) << 23);
        const float qscale = __uint_as_float((unsigned)(ex + 127 - 5) << 23);   // 2^-5: 17-sums of squares < 65504
        const float unscale = __uint_as_float((unsigned)(127 - ex) << 23);
        typedef __fp16 hv2 __attribute__((ext_vector_type(2)));
#pragma unroll
        for (int k = 0; k < MF8_ROWS_PER_THREAD; ++k) {
            if (k < MF8_ROWS_PER_THREAD - 1 || row7) {
                const int r = rg + 12 * k;
                // heads by truncation, tails exact differences (one v_fma_mix_f32 per value from the packed heads)
                const float a = xa[k] * scale, b = xb[k] * scale;
                const hv2 hh = __builtin_amdgcn_cvt_pkrtz(a, b);
                const float qa = (xa[k] * qscale) * a, qb = (xb[k] * qscale) * b;
                const hv2 qh = __builtin_amdgcn_cvt_pkrtz(qa, qb);
                const unsigned hu = __builtin_bit_cast(unsigned, hh), qu = __builtin_bit_cast(unsigned, qh);
                const hv2 tt = __builtin_amdgcn_cvt_pkrtz(sub_f16_lo(a, hu), sub_f16_hi(b, hu));
                const hv2 qt = __builtin_amdgcn_cvt_pkrtz(sub_f16_lo(qa, qu), sub_f16_hi(qb, qu));
                const int o = (r * MF_R + 2 * c2) * 2;
                *reinterpret_cast<hv2*>(pl_xh + o) = hh;
                *reinterpret_cast<hv2*>(pl_xl + o) = tt;
                *reinterpret_cast<hv2*>(pl_qh + o) = qh;
                *reinterpret_cast<hv2*>(pl_ql + o) = qt;
            }
        }
        MF_STAMP(1);
        // ---- the previous tile's coefficients and stores
        if (pending) emit(p_I0, p_J0, p_unscale, p_acc, p_S1, p_S2);
        MF_STAMP(6);
        lds_barrier();

        // ---- box sums: horizontal pass over the wave's 32 input rows, the partial sums split again and fed to the vertical
        //      pass as they lie (ones_p).  4 steps (2 column tiles x {x, x^2}); the fragments of step t + 1 are loaded before
        //      the conversions of step t.
        f4 S1[2], S2[2];                         // (every one of them is the result of a step below)
        if constexpr (XCORR) {
#pragma unroll
            for (int c = 0; c < 2; ++c) S1[c] = S2[c] = zero4;
        } else {
            auto hfrag = [&](int t, h8 (&f)[4]) {
                const int c = t >> 1;
                const char* ph = (t & 1) ? pl_qh : pl_xh;
                const char* pt = (t & 1) ? pl_ql : pl_xl;
#pragma unroll
                for (int rb = 0; rb < 2; ++rb) {
                    const int off = ((wr0 + 16 * rb + n) * MF_R + wc0 + 16 * c + 8 * g) * 2;
                    f[2 * rb] = *reinterpret_cast<const h8*>(ph + off);
                    f[2 * rb + 1] = *reinterpret_cast<const h8*>(pt + off);
                }
            };
            h8 cur[4];
            hfrag(0, cur);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                h8 nxt[4];
                if (t + 1 < 4) hfrag(t + 1, nxt);
                typedef unsigned u4 __attribute__((ext_vector_type(4)));
                u4 bhw, blw;
#pragma unroll
                for (int rb = 0; rb < 2; ++rb) {
                    f4 h = mfma16(cur[2 * rb], ones_b, zero4);
                    h = mfma16(cur[2 * rb + 1], ones_b, h);
#pragma unroll
                    for (int pr = 0; pr < 2; ++pr) {
                        const unsigned hp = pack_h2((_Float16)h[2 * pr], (_Float16)h[2 * pr + 1]);
                        bhw[2 * rb + pr] = hp;
                        blw[2 * rb + pr] = pack_h2((_Float16)sub_f16_lo(h[2 * pr], hp), (_Float16)sub_f16_hi(h[2 * pr + 1], hp));
                    }
                }
                const h8 bh = __builtin_bit_cast(h8, bhw), bl = __builtin_bit_cast(h8, blw);
                f4 sacc = mfma16(bh, ones_p, zero4);
                sacc = mfma16(bl, ones_p, sacc);
                if (t & 1) S2[t >> 1] = sacc;
                else S1[t >> 1] = sacc;
                if (t + 1 < 4) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) cur[q] = nxt[q];
                }
            }
        }
        MF_STAMP(2);
        lds_barrier();                           // all waves are done with the squares
        // ---- next tile's pixels -> `raw` while this tile's correlation runs
        walk.advance();
        const bool have_next = !walk.done();
        int n_I0 = 0, n_J0 = 0;
        bool n_inside = false;
        if (have_next) {
            walk.origin(A.row_begin, n_I0, n_J0);
            n_inside = tile_inside(n_I0, n_J0);
            fetch(n_I0, n_J0, n_inside);
        }

        MF_STAMP(3);
        // ---- cross term: 17 template rows x 2 column tiles, fragments of row s + 1 in flight during row s
        f4 acc[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) acc[c] = zero4;
        h8 ah[2], al[2];
        const int fo = ((wr0 + n) * MF_R + wc0 + 8 * g) * 2;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            ah[c] = *reinterpret_cast<const h8*>(pl_xh + fo + 32 * c);
            al[c] = *reinterpret_cast<const h8*>(pl_xl + fo + 32 * c);
        }
        h8 bl = reinterpret_cast<const h8*>(smem + MFD_WL)[lane];
        h8 bh = reinterpret_cast<const h8*>(smem + MFD_WL)[9 * 64 + lane];
#pragma unroll
        for (int s = 0; s < 17; ++s) {
            h8 nh[2], nl[2], nb, nbh;
            if (s + 1 < 17) {
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    nh[c] = *reinterpret_cast<const h8*>(pl_xh + fo + (s + 1) * MF_R * 2 + 32 * c);
                    nl[c] = *reinterpret_cast<const h8*>(pl_xl + fo + (s + 1) * MF_R * 2 + 32 * c);
                }
                const int sn = s + 1 > 8 ? 16 - (s + 1) : s + 1;
                nb = reinterpret_cast<const h8*>(smem + MFD_WL)[sn * 64 + lane];
                nbh = reinterpret_cast<const h8*>(smem + MFD_WL)[(9 + sn) * 64 + lane];
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int c = 0; c < 2; ++c) acc[c] = mfma16(bh, ah[c], acc[c]);     // weights as A: transposed tile
#pragma unroll
            for (int c = 0; c < 2; ++c) acc[c] = mfma16(bl, ah[c], acc[c]);
#pragma unroll
            for (int c = 0; c < 2; ++c) acc[c] = mfma16(bh, al[c], acc[c]);
            __builtin_amdgcn_sched_barrier(0);
            if (s + 1 < 17) {
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    ah[c] = nh[c];
                    al[c] = nl[c];
                }
                bl = nb;
                bh = nbh;
            }
        }
        MF_STAMP(4);
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            p_acc[c] = acc[c];
            p_S1[c] = S1[c];
            p_S2[c] = S2[c];
        }
        p_I0 = I0;
        p_J0 = J0;
        p_unscale = unscale;
        pending = true;
        I0 = n_I0;
        J0 = n_J0;
        inside = n_inside;
        have = have_next;
    }
    MF_WALL(13);
    if (pending) emit(p_I0, p_J0, p_unscale, p_acc, p_S1, p_S2);
    MF_WALL(14);
#ifdef CS_MF_PROFILE
    if (tid == 0) {
        prof_lds[5] += 1ull;
        for (int k = 0; k < 16; ++k)
            if (prof_lds[k]) atomicAdd(&cs_mf_prof[k], prof_lds[k]);
    }
#undef MF_PROF_ADD
#define MF_PROF_ADD(k, v) atomicAdd(&cs_mf_prof[k], (unsigned long long)(v))
#endif
}
