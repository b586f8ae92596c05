// Body of corr_mfma_dense_kernel and of the table instance behind corr_mfma_blocks_kernel (cs_corr_mfma.hip includes this
// file twice).  In scope: the template parameters VEC4, REG, RSYM, CAND; `A` (the argument block); constexpr bool TABLE and,
// when it is set, table_entry (address of the block's entry), table_tile, table_tile_end, table_tile_step; constexpr bool LIST
// and tile_list (LIST: the workgroups walk a list of tile indices by * tiles_x + bx, A.n_tiles long, instead of every tile); the macro
// MFD_NOMASK_KS (the statistics block as the unmasked epilogue passes it on: A.ks).  Textual
// inclusion, not a function call: the masked instances sit at 256 registers and their allocation follows the exact
// statement order (a call boundary cost 3 % on C4').

    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* const pl_xh = smem;
    char* const pl_xl = smem + MF_PLANE;
    char* const pl_qh = smem + 2 * MF_PLANE;
    char* const pl_ql = smem + 3 * MF_PLANE;
    float* const raw = reinterpret_cast<float*>(smem + 2 * MF_PLANE);      // next tile's pixels: aliases the squares
    const int tid = threadIdx.x;
    const int lane = tid & 63, wv = tid >> 6;
    const int n = lane & 15, g = lane >> 4;
    char* const scr = smem + MFD_SCR + wv * (2 * MF_SCR_PLANE);
    unsigned* const red = reinterpret_cast<unsigned*>(smem + MFD_RED);
    const int km = A.km, kn = A.kn;
    const int kh = (km - 1) / 2, kw = (kn - 1) / 2;
#ifdef CS_MF_PROFILE
#undef MF_PROF_ADD
#define MF_PROF_ADD(k, v) (prof_lds[k] += (unsigned long long)(v))
    unsigned long long* const prof_lds = reinterpret_cast<unsigned long long*>(smem + MFD_PROF);
    unsigned long long tprev_ = 0;
    unsigned long long wall_ = __builtin_amdgcn_s_memrealtime();
    if (tid == 0)
        for (int k = 0; k < 16; ++k) prof_lds[k] = 0;
    auto prof_flush = [&]() {
        if (tid == 0) prof_lds[5] += 1ull;
        if (tid == 0)
            for (int k = 0; k < 16; ++k)
                if (prof_lds[k]) atomicAdd(&cs_mf_prof[k], prof_lds[k]);
    };
#endif

    // all-ones Toeplitz operands: ones_b[k][n] = 1 for 0 <= k - n < kn (horizontal box sums); ones_p: the vertical
    // one, 1 for 0 <= row - n < km, with the contraction slot (g, e) standing for row rho(g, e) = 4 g + e (e < 4),
    // 16 + 4 g + e - 4 (e >= 4) -- the order in which the horizontal pass leaves a column's rows in a lane
    h8 ones_b, ones_p;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int t = 8 * g + e - n;
        ones_b[e] = (t >= 0 && t < kn) ? (_Float16)1.0f : (_Float16)0.0f;
        const int rho = (e < 4 ? 4 * g + e : 16 + 4 * g + (e - 4)) - n;
        ones_p[e] = (rho >= 0 && rho < km) ? (_Float16)1.0f : (_Float16)0.0f;
    }
    const f4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
    const int wr0 = 16 * wv;
    const int c2 = tid % 40, rg = tid / 40;         // staging: column pair, row group (threads >= 240 idle)
    const int c2_ = c2, rg_ = rg;
    const bool stager = tid < 240;
    // input rows that windows of [row_begin, row_end) reach and that exist
    const int p_min = max(0, A.row_begin - kh), p_max = min(A.ms, A.row_end + (km - 1) - kh) - 1;
    // REG, zero-padded band input (CS_LAYOUT_BAND_PADDED): the first staged row from which a tile is fetched without clamps
    // (see fetch); "never" for the other inputs
    int pad_row0 = 0x7fffffff;
    if constexpr (REG && VEC4) pad_row0 = A.pad_in ? max(p_min, (int)A.row0_in + 1) : 0x7fffffff;
    // REG, band of raw counts (CS_LAYOUT_BAND_COUNTS): the cap of the detrended values, from the header in front of the band
    float cnt_max = 0.0f;
    const float* cnt_wt = nullptr;
    const float* cnt_rlaw = nullptr;
    int cnt_n = 1, cnt_nd = 1;
    if constexpr (REG && VEC4) {
        if (A.cnt_in) {
            const CountsHdrPtr H = counts_header(A.sig);
            cnt_max = (float)H->max_val;
            cnt_wt = H->weight32;
            cnt_rlaw = H->rlaw32;
            cnt_n = H->n;
            cnt_nd = H->n_diags;
        }
    }

    auto tile_origin = [&](int tile, int& I0, int& J0) {
        if constexpr (LIST) tile = tile_list[tile];       // (cs_candidates_tiles: only the tiles a stored pixel reaches)
        int by = tile / A.tiles_x;
        int bx = tile - by * A.tiles_x;
        if constexpr (REG) {
            // (band outputs: the tile rows from by_cut on end at the matrix's last column -- launch_corr_mfma_f32)
            if (by >= A.by_cut) {
                int t = tile - A.by_cut * A.tiles_x;
                by = A.by_cut;
                for (;;) {
                    const int left = A.ns - (A.row_begin + by * MF_T + A.out_lo);
                    const int v = min(A.tiles_x, left <= 0 ? 0 : (left + MF_T - 1) / MF_T);
                    if (t < v) break;
                    t -= v;
                    ++by;
                }
                bx = t;
            }
        }
        I0 = A.row_begin + by * MF_T;
        if constexpr (!REG) {
            // Dense maps: tile row `by` starts `by * skew` columns further right (mod tiles_x).  Workgroups step through the
            // tile list 64 (an XCD's workgroups) or gridDim apart: when tiles_x divides that step -- 4096^2 is 64 x 64 tiles --
            // every workgroup walks straight DOWN one tile column, all 512 of them in step, and the map runs 13 % slower than
            // its neighbours 4032^2 and 4160^2 (profiles/r05_dense_sizes.txt: 103 us against 89 and 93).  The host picks the
            // skew (0 .. 3) under which a workgroup's next tiles are in other columns (dense_tile_skew).
            const int skew = A.xcd_order >> 1;
            if (skew) {
                bx += (by * skew) % A.tiles_x;
                bx -= bx >= A.tiles_x ? A.tiles_x : 0;
            }
        }
        J0 = bx * MF_T;
        if (REG && A.band_out) J0 += I0 + A.out_lo;       // the strip of tiles follows the band
    };
    // LDS-DMA of one tile's 80 x 80 pixels (clamped addresses; the reader masks what lies outside).
    // The image is row-major; a wave-wide transfer moves 64 consecutive 4-byte (VEC4: 16-byte) pieces of
    // it, wave w issues the transfers w, w + 4, ...  A lane's piece advances by 256 pieces per step.
    const int wv_u = __builtin_amdgcn_readfirstlane(wv);
    auto fetch_args = [&]() {
        if constexpr (REG) return TABLE ? args_at(table_entry) : args_here();
        else return &A;
    };
    constexpr int kPiecesPerRow = VEC4 ? MF_R / 4 : MF_R;
    constexpr int kTransfers = VEC4 ? 25 : 100;
    auto fetch = [&](int tile, int slot) {
        // (REG: the arguments of the transfers through an opaque pointer, see the epilogue)
        const auto FA = fetch_args();
        int I0, J0;
        tile_origin(tile, I0, J0);
        const int P0 = I0 - kh, Q0 = J0 - kw;
        // REG, zero-padded band (CS_LAYOUT_BAND_PADDED): a piece that reaches beyond a row's stored diagonals reads the zero slots
        // behind them (or behind the previous row's: the four slots in front of a row), so nothing is shifted and the reader
        // needs no masks -- only the tiles whose rows leave the matrix (or start at the buffer's first row) keep the clamps
        const bool pad_tile = REG && VEC4 && P0 >= pad_row0 && P0 + MF_R - 1 <= p_max;
        // The per-lane constants of the transfers are recomputed from an opaque copy of the lane index: hoisted out
        // of the tile loop they are spilled, and a reload here waits (vmcnt) for the previous tile's stores.
        int lane_f = lane;
        if constexpr (REG) asm volatile("" : "+v"(lane_f));         // (the dense instances have registers to spare)
        const int e0 = 64 * wv_u + lane_f;
        int r = e0 / kPiecesPerRow, c = e0 - r * kPiecesPerRow;
        if (REG && !MFD_DBG(16384)) {
            // column terms of the tile's 64 columns (waves 0..2) and the flags of its 80 staged columns (wave 3)
            if (wv_u < 3) {
                const float* src = FA->coltab + (size_t)wv_u * FA->ns + min(max(J0 + lane_f, 0), FA->ns - 1);
                __builtin_amdgcn_global_load_lds(src, (__attribute__((address_space(3))) void*)(
                    (__attribute__((address_space(3))) char*)(smem) + MFD_COL + (slot * 3 + wv_u) * 256), 4, 0, 0);
            } else {
                // the 80 flag bytes of columns Q0 .. Q0 + 79 as the <= 22 aligned dwords that hold them (lanes
                // beyond are harmless repeats; addresses clamped to the dwords that overlap the array)
                const long long base = (long long)(uintptr_t)FA->miss_col;
                const long long first = ((base + Q0) >> 2) << 2;
                long long addr = first + 4 * min(lane_f, 23);
                addr = min(max(addr, (base >> 2) << 2), ((base + FA->ns - 1) >> 2) << 2);
                if (lane_f < 24)
                    __builtin_amdgcn_global_load_lds(reinterpret_cast<const unsigned*>((uintptr_t)addr),
                                                     (__attribute__((address_space(3))) void*)(
                                                         (__attribute__((address_space(3))) char*)(smem) + MFD_CFB + slot * 128), 4, 0, 0);
            }
        }
        if constexpr (REG && VEC4) {
            if (FA->cnt_in) {
                // CS_LAYOUT_BAND_COUNTS: what turns the tile's counts into detrended values -- the weights of its 80 rows and 80
                // columns and 1 / law of its 160 diagonals, float32, 320 dwords in all -- lands in the first wave's store scratch
                // (free from here until the tile's epilogue: the previous epilogue is behind a barrier).  Clamped indices:
                // whatever a clamped slot delivers multiplies a count of 0.
                const float* wt = cnt_wt;
                const float* rlaw = cnt_rlaw;
                const int hn = cnt_n, hd = cnt_nd;
#pragma unroll 1
                for (int x = wv_u; x < 5; x += 4) {
                    const int e = 64 * x + lane_f;
                    // (one base and one clamped 32-bit index per lane: rows, columns, then diagonals against the law's reciprocals)
                    const bool is_w = e < 160;
                    const int idx = e < 80 ? P0 + e : e < 160 ? Q0 + (e - 80) : Q0 - P0 - (MF_R - 1) + (e - 160);
                    const float* src = (is_w ? wt : rlaw) + min(max(idx, is_w ? 0 : -1), is_w ? hn - 1 : hd);
                    __builtin_amdgcn_global_load_lds(src, (__attribute__((address_space(3))) void*)(
                                                              (__attribute__((address_space(3))) char*)(smem) + MFD_SCR + 256 * x), 4, 0, 0);
                }
            }
        }
        const __attribute__((address_space(3))) char* dst =
            (const __attribute__((address_space(3))) char*)(raw) + (VEC4 ? 1024 : 256) * wv_u;
        if constexpr (!REG && VEC4) {
            // Inner tiles of a dense map (every staged row and column exists: nearly all of them): no clamp can bite, a
            // piece's address is one base + r ld + 4 c -- the band instances' form below, without the diagonal shift.
            if (P0 >= p_min && P0 + MF_R - 1 <= p_max && Q0 >= 0 && Q0 + MF_R <= FA->ns) {
                const float* src = FA->sig + ((long long)P0 + r - FA->row0_in) * FA->ld_in + Q0 + 4 * c;
                const long long step_r = 12 * FA->ld_in + 64, wrap = FA->ld_in - 80;      // 256 pieces on: 12 rows and 16 pieces
#pragma unroll 1
                for (int i = wv_u; i < kTransfers; i += 4) {
                    __builtin_amdgcn_global_load_lds(src, (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
                    dst += 4096;
                    c += 16;
                    src += step_r;
                    if (c >= kPiecesPerRow) {
                        c -= kPiecesPerRow;
                        src += wrap;
                    }
                }
                return;
            }
        }
        if constexpr (REG && VEC4) {
            // Inner tiles of a band (every staged row exists, every staged diagonal is stored: 13 of the 18 tiles of a strip at
            // 1001 diagonals): no clamp can bite, a piece's address is one base + r (ld - 1) + 4 c -- two additions per transfer
            // instead of the ~ 20 instructions of the clamped form below.
            if (FA->band_in && P0 >= p_min && P0 + MF_R - 1 <= p_max && Q0 - (P0 + MF_R - 1) - FA->lo_in >= 0 &&
                Q0 + MF_R - 1 - P0 - FA->lo_in <= FA->bw_in - 1) {
                const float* src = FA->sig + ((long long)P0 - FA->row0_in) * FA->ld_in + (Q0 - P0 - FA->lo_in) + (long long)r * (FA->ld_in - 1) + 4 * c;
                const long long step_r = 12 * (FA->ld_in - 1) + 64, wrap = (FA->ld_in - 1) - 80;      // 256 pieces on: 12 rows and 16 pieces
#pragma unroll 1
                for (int i = wv_u; i < kTransfers; i += 4) {
                    __builtin_amdgcn_global_load_lds(src, (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
                    dst += 4096;
                    c += 16;
                    src += step_r;
                    if (c >= kPiecesPerRow) {
                        c -= kPiecesPerRow;
                        src += wrap;
                    }
                }
                return;
            }
        }
#pragma unroll 1
        for (int i = wv_u; i < kTransfers; i += 4) {
            const int p = min(max(P0 + r, p_min), p_max);
            const float* row = FA->sig + ((long long)p - FA->row0_in) * FA->ld_in;
            if constexpr (VEC4) {
                // REG: the piece's first stored index (band: diagonal index q - p - lo), clamped into the row's
                // stored range -- the reader undoes the shift (16-byte transfers need no 16-byte alignment)
                int q = Q0 + 4 * c;
                if (REG && FA->band_in) q = pad_tile ? min(max(q - p - FA->lo_in, -4), FA->bw_in) : min(max(q - p - FA->lo_in, 0), FA->bw_in - 4);
                else q = min(max(q, 0), FA->ns - 4);
                __builtin_amdgcn_global_load_lds(row + q, (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
                dst += 4096;
                c += 256 % kPiecesPerRow;
                r += 256 / kPiecesPerRow;
            } else {
                int q = min(max(Q0 + c, 0), FA->ns - 1);
                if (REG && FA->band_in) q = min(max(q - p - FA->lo_in, 0), FA->bw_in - 1);      // stored diagonal index
                __builtin_amdgcn_global_load_lds(row + q, (__attribute__((address_space(3))) void*)dst, 4, 0, 0);
                dst += 1024;
                c += 256 % kPiecesPerRow;
                r += 256 / kPiecesPerRow;
            }
            if (c >= kPiecesPerRow) {
                c -= kPiecesPerRow;
                r += 1;
            }
        }
    };

    // epilogue of one tile (lane = row n of the wave's 16, columns 16 c + 4 g + v), run one iteration late:
    // its stores then have the whole next tile to retire before the `vmcnt(0)` that awaits the DMA
    auto emit = [&](int I0, int J0, float unscale, const f4 (&acc)[4], const f4 (&S1)[4], const f4 (&S2)[4],
                    const f4& hdr, int slot) {
        const float u_cs = unscale * A.w_unscale;
        const float u_s2 = 32.0f * unscale;
        if constexpr (REG) {
            // ---- per-bin masks: the factorised mask sums of cs_mask_prep.hip (see cs_corr_stream.h MODE 2)
            //   n_missing = K nr[i] + (K - nr[i]) ncol[j],  sum_missing Wa = RA[i] + CA[j] - sum_kj c[j+kj] U_i[kj]
            // plus the precomputed corrections of the pixels whose window leaves the matrix / 0..max_dist
            // every argument the epilogue reads comes through a pointer the compiler cannot see through: the words are
            // loaded here, once per tile, instead of being held -- spilled to lanes -- across the whole tile loop
            const ArgsPtr EA = TABLE ? args_at(table_entry) : args_here();
            const int K = km;
            const int i = I0 + wr0 + n;
            KernelStats<float> KS;                                // loaded here, not held across the tile loop
            {
                const StatsPtr sp = TABLE ? stats_args_at(table_entry) : stats_args();
                KS.n = sp->n; KS.inv_n = sp->inv_n; KS.kmean = sp->kmean; KS.kstd = sp->kstd; KS.kvar = sp->kvar;
                KS.ksum = sp->ksum; KS.k2sum = sp->k2sum; KS.thr = sp->thr; KS.eps = sp->eps; KS.cut = sp->cut;
                KS.thr_n = sp->thr_n; KS.nkvar = sp->nkvar; KS.eps2 = sp->eps2; KS.den2_min = sp->den2_min;
                KS.zk_possible = sp->zk_possible; KS.snap_possible = sp->snap_possible;
                KS.cand_cmin = CAND ? sp->cand_cmin : 0.0f;
                KS.cand_thr = CAND ? sp->cand_thr : 0.0f;
            }
            const float* colb = reinterpret_cast<const float*>(smem + MFD_COL) + slot * 3 * 64;
            const float nr = hdr[0], ra = hdr[1], rb = hdr[2];
            // The cross term sum_kj c[j + kj] U_i[kj], U_i[kj] = sum over the flagged rows ki of row i's window of
            // W[ki][kj], exists only where a flagged row AND a flagged column reach the window.  On the matrix
            // cores: A = Hankel matrix of the column flags (exact in float16), B = U (head + tail), per column tile.
            const unsigned* cfm = reinterpret_cast<const unsigned*>(smem + MFD_CFL) + slot * 4;
            const unsigned m0 = __builtin_amdgcn_readfirstlane(cfm[0]), m1 = __builtin_amdgcn_readfirstlane(cfm[1]),
                           m2 = __builtin_amdgcn_readfirstlane(cfm[2]);
            const bool tile_flags = (m0 | m1 | m2) != 0;
            const unsigned row_bits = (tile_flags && !MFD_DBG(128)) ? (unsigned)hdr[3] : 0u;
            const bool cross_on = __builtin_amdgcn_ballot_w64(row_bits != 0) != 0;
            h8 ua_h, ua_t, ub_h, ub_t;
            if (cross_on) {
                float ua[8], ub[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) ua[e] = ub[e] = 0.0f;
                unsigned bits = row_bits;
                while (__builtin_amdgcn_ballot_w64(bits != 0)) {
                    if (bits) {
                        const int ki = __builtin_ctz(bits);
                        bits &= bits - 1;
                        const float* wa = EA->w + K * K + ki * K;
                        const float* wb = EA->w + 2 * K * K + ki * K;
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            const int kj = 8 * g + e;
                            const float in = kj < K ? 1.0f : 0.0f;
                            ua[e] = fmaf(wa[min(kj, K - 1)], in, ua[e]);
                            ub[e] = fmaf(wb[min(kj, K - 1)], in, ub[e]);
                        }
                    }
                }
                const float sa = __builtin_amdgcn_rcpf(EA->wa_unscale), sb = __builtin_amdgcn_rcpf(EA->wb_unscale);   // powers of two
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float a = ua[e] * sa, b = ub[e] * sb;
                    ua_h[e] = (_Float16)a;
                    ua_t[e] = (_Float16)(a - (float)ua_h[e]);
                    ub_h[e] = (_Float16)b;
                    ub_t[e] = (_Float16)(b - (float)ub_h[e]);
                }
            }
            MF_STAMP(7);      // emit: statistics block, U vectors of the cross term
            const unsigned kmask8 = (((1u << K) - 1u) >> (8 * g)) & 0xffu;      // template columns 8 g .. 8 g + 7 that exist
            const int dmin = J0 - (I0 + MF_T - 1), dmax = J0 + MF_T - 1 - I0;
            // frame records (cs_mask_prep.hip mask_frame_fix): tiles with a pixel whose window leaves the matrix; with
            // rim_in_kernel they are the only records left -- the edge diagonals are corrected from the rim tables below
            const bool on_edge_diag = EA->fix_on && ((dmin < K - 1 && dmax >= 0) | (dmax >= EA->fix_hi_d0 && dmin < EA->fix_hi_d0 + EA->fix_hi_w));
            // (band outputs, fix_on: below bot0 only the last KH rows and the last KH columns have a record -- mask_fix_record -- so
            // of the 16 tile rows under bot0 only the tiles at the matrix's last columns, and the last tile row, look any up)
            const bool right_or_bottom = !EA->fix_on | (I0 + MF_T - 1 + (K - 1) / 2 >= EA->ms) | (J0 + MF_T - 1 + (K - 1) / 2 >= EA->ns);
            const bool needs_fix = !MFD_DBG(256) && ((I0 < EA->fix_top) | ((I0 + MF_T - 1 >= EA->fix_bot0) & right_or_bottom) | (EA->fix_any_side != 0) |
                                   (on_edge_diag && !EA->rim_in_kernel));
            // (RSYM instances only: the others have no registers for it -- the host leaves them their records)
            const bool needs_rim = RSYM && !MFD_DBG(256) && on_edge_diag && EA->rim_in_kernel;
            // every pixel of the tile is produced: rows below row_end, columns inside the matrix, diagonals inside the band
            const bool plain_out = I0 + MF_T <= EA->row_end && J0 >= 0 && J0 + MF_T <= EA->ns && dmin >= EA->out_lo && dmax <= EA->out_hi;
            float* tb = reinterpret_cast<float*>(scr);
            const bool tile_forced = EA->sym_upper && dmin + (kn - km) < 0;
            // Pixels on an edge diagonal (lower: 0 .. K - 2, their windows reach below the main diagonal; upper: fix_hi_d0 ...,
            // beyond max_dist) whose window lies inside the matrix (the others have a frame record): the correction comes
            // from the rim tables of the weights.  A wave's 16 rows x 64 columns cross ONE of the two ranges (the host
            // checks that they lie more than a wave's 79 diagonals apart) in at most 16 diagonals per row, and of those 16
            // consecutive columns a lane owns exactly four -- one per v, in column tile c = fxc's v-th nibble -- so every
            // lane evaluates four pixels, whichever they are: four steps per wave-tile instead of one per pixel position.
            f4 fxn = zero4, fxa = zero4, fxb = zero4;
            unsigned fxc = 0xffffu;
            if constexpr (RSYM) if (needs_rim) {
                const FixArgsPtr F = TABLE ? fix_args_at(table_entry) : fix_args();
                const int hi_d0 = F->fix_hi_d0, hi_w = F->fix_hi_w;
                const int iw0 = I0 + wr0;
                const int wd_lo = J0 - iw0 - 15, wd_hi = J0 + MF_T - 1 - iw0;          // the wave's diagonals
                const bool low = wd_lo < K - 1 && wd_hi >= 0;
                const bool up = wd_hi >= hi_d0 && wd_lo < hi_d0 + hi_w;
                if (low | up) {
                    const float* rimtab = F->rim;
                    const int md = F->max_dist, bot0 = F->fix_bot0;
                    const int KHf = (K - 1) / 2;
                    const int d0 = low ? 0 : hi_d0, dn = low ? K - 1 : hi_w;
                    const int a = i + d0 - J0;                                    // tile column of the row's first pixel of the range
                    const unsigned rb_all = (unsigned)hdr[3];
                    const bool row_ok = (i >= KHf) & (i + KHf < EA->ms) & (i < EA->row_end);
                    fxc = 0u;
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        const int c = (a - 4 * g - v + 15) >> 4;                  // the lane's column 16 c + 4 g + v at or after a
                        const int x = 16 * c + 4 * g + v;
                        const int d = d0 + (x - a), j = J0 + x;
                        const bool framed = (i >= bot0) & ((i + KHf >= EA->ms) | (j + KHf >= EA->ns));
                        const bool on = row_ok & (c >= 0) & (c <= 3) & (x - a < dn) & !framed & (j >= KHf) & (j + KHf < EA->ns) &
                                        (d >= EA->out_lo) & (d <= EA->out_hi);
                        float fn = 0.0f, fa = 0.0f, fb = 0.0f;
                        if (on) {
                            const unsigned lo32 = x < 32 ? m0 : x < 64 ? m1 : m2;       // window = staged columns x .. x + K - 1
                            const unsigned hi32 = x < 32 ? m1 : x < 64 ? m2 : 0u;
                            const unsigned cb = (unsigned)((((unsigned long long)hi32 << 32) | lo32) >> (x & 31)) & ((1u << K) - 1u);
                            rim_correction(rimtab, K, d, md, rb_all, cb, fn, fa, fb);
                        }
                        fxn[v] = fn;
                        fxa[v] = fa;
                        fxb[v] = fb;
                        fxc |= (on ? (unsigned)c : 15u) << (4 * v);
                    }
                }
            }
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                // A wave's 16 rows x 32 columns of which no pixel is produced (the corners of the outer tiles of a band's strip:
                // 6 of the 40 half-rows of a 234-diagonal band, C3) are skipped whole -- scalar test, the epilogue is where the
                // masked instances spend half their time.
                {
                    const int iw0 = I0 + 16 * wv_u, jh0 = J0 + 32 * half;
                    if ((iw0 >= EA->row_end) | (jh0 + 31 < 0) | (jh0 >= EA->ns) | (jh0 + 31 - iw0 < EA->out_lo) | (jh0 - (iw0 + 15) > EA->out_hi))
                        continue;
                }
                f4 rv[2], nmv[2], kav[2], kbv[2];
                unsigned rare_bits = 0u;
#pragma unroll
                for (int cc = 0; cc < 2; ++cc) {
                    const int c = 2 * half + cc;
                    __builtin_amdgcn_sched_barrier(0);       // one column tile at a time: keeps the live set small
                    // cross term of this column tile
                    f4 xa = zero4, xb = zero4;
                    if (cross_on) {
                        // lane (m = n, k group g) of the Hankel operand: flags of staged columns 16 c + n + 8 g + e
                        const int sh = 16 * c + n + 8 * g;                       // 0 .. 87
                        const unsigned lo = sh < 32 ? m0 : sh < 64 ? m1 : m2;
                        const unsigned hi = sh < 32 ? m1 : sh < 64 ? m2 : 0u;
                        const unsigned w8 = (unsigned)((((unsigned long long)hi << 32) | lo) >> (sh & 31)) & kmask8;
                        typedef unsigned u4 __attribute__((ext_vector_type(4)));
                        u4 fw;
#pragma unroll
                        for (int pr = 0; pr < 4; ++pr)
                            fw[pr] = ((w8 >> (2 * pr)) & 1u) * 0x3C00u + ((w8 >> (2 * pr + 1)) & 1u) * 0x3C000000u;   // 1.0 in float16
                        const h8 ff = __builtin_bit_cast(h8, fw);
                        xa = mfma16(ff, ua_h, xa);
                        xa = mfma16(ff, ua_t, xa);
                        xb = mfma16(ff, ub_h, xb);
                        xb = mfma16(ff, ub_t, xb);
#pragma unroll
                        for (int v = 0; v < 4; ++v) {
                            xa[v] *= EA->wa_unscale;
                            xb[v] *= EA->wb_unscale;
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    const f4 ncol = *reinterpret_cast<const f4*>(colb + 16 * c + 4 * g);
                    const f4 ca = *reinterpret_cast<const f4*>(colb + 64 + 16 * c + 4 * g);
                    const f4 cb = *reinterpret_cast<const f4*>(colb + 128 + 16 * c + 4 * g);
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        nmv[cc][v] = (float)K * nr + ((float)K - nr) * ncol[v];
                        kav[cc][v] = ra + ca[v] - xa[v];
                        kbv[cc][v] = rb + cb[v] - xb[v];
                    }
                }
                MF_STAMP(8);      // emit: mask sums of the half (tables, cross term)
                if (needs_fix) {
                    // pixels whose window leaves the matrix or the diagonals 0 .. max_dist (tiles on the rim of the band)
                    const FixArgsPtr F = TABLE ? fix_args_at(table_entry) : fix_args();
                    const int iw0 = I0 + wr0;                 // the wave's 16 rows
                    const bool rows_hit = (iw0 < EA->fix_top) | ((iw0 + 15 >= EA->fix_bot0) & (!EA->fix_on | (iw0 + 15 + (K - 1) / 2 >= EA->ms) | (J0 + MF_T - 1 + (K - 1) / 2 >= EA->ns))) |
                                          (EA->fix_any_side != 0);
                    // rolled over the half's 8 pixels two at a time: two record loads in flight (one at a time, each awaited
                    // before the next lookup, made a rim tile 45 % slower than an inner one; four at a time spill)
#pragma unroll 1
                    for (int k = 0; k < 4; ++k) {
                        // the wave's pixels of this step: columns j0 + 4 g + {0, 1}, diagonals [j0 - iw0 - 15, j0 + 13 - iw0]
                        const int cc = k >> 1, v0 = 2 * (k & 1);
                        const int j0 = J0 + 16 * (2 * half + cc) + v0;
                        const int dlo = j0 - iw0 - 15, dhi = j0 + 13 - iw0;
                        const bool diag_hit = EA->fix_on && !EA->rim_in_kernel && ((dlo < K - 1 && dhi >= 0) | (dhi >= EA->fix_hi_d0 && dlo < EA->fix_hi_d0 + EA->fix_hi_w));
                        if (!(rows_hit | diag_hit)) continue;
                        const float* fa = mask_fix_record(A, F, i, j0 + 4 * g);
                        const float* fb = mask_fix_record(A, F, i, j0 + 4 * g + 1);
                        if (!__builtin_amdgcn_ballot_w64((fa != nullptr) | (fb != nullptr))) continue;
                        f4 ra = zero4, rb = zero4;
                        if (fa) ra = *reinterpret_cast<const f4*>(fa);        // 16-byte records, 16-byte aligned tables
                        if (fb) rb = *reinterpret_cast<const f4*>(fb);
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            if (e == k) {
                                nmv[e >> 1][2 * (e & 1)] += ra[0];
                                kav[e >> 1][2 * (e & 1)] += ra[1];
                                kbv[e >> 1][2 * (e & 1)] += ra[2];
                                nmv[e >> 1][2 * (e & 1) + 1] += rb[0];
                                kav[e >> 1][2 * (e & 1) + 1] += rb[1];
                                kbv[e >> 1][2 * (e & 1) + 1] += rb[2];
                            }
                        }
                    }
                }
                if constexpr (RSYM) if (needs_rim) {
                    // the lane's (at most four) pixels on an edge diagonal: corrections formed before the halves
#pragma unroll
                    for (int cc = 0; cc < 2; ++cc) {
#pragma unroll
                        for (int v = 0; v < 4; ++v) {
                            const bool hit = ((fxc >> (4 * v)) & 15u) == (unsigned)(2 * half + cc);
                            nmv[cc][v] += hit ? fxn[v] : 0.0f;
                            kav[cc][v] += hit ? fxa[v] : 0.0f;
                            kbv[cc][v] += hit ? fxb[v] : 0.0f;
                        }
                    }
                }
                MF_STAMP(9);      // emit: correction records
#pragma unroll
                for (int cc = 0; cc < 2; ++cc) {
                    const int c = 2 * half + cc;
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        const int j = J0 + 16 * c + 4 * g + v;
                        const int d = j - i;
                        const float nm = nmv[cc][v], ka = kav[cc][v], kb = kbv[cc][v];
                        const float cs = acc[c][v] * u_cs;
                        const float s1 = S1[c][v] * unscale;
                        const float s2 = (S2[c][v] * u_s2) * unscale;
                        bool rare;
                        float val = pearson_masked_core<CAND ? 1 : 0>(cs, s1, s2, nm, ka, kb, KS, rare);
                        if constexpr (CAND) val = cand_range_guard(val, s2, unscale, KS);
                        if MFD_DBG(4096) {
                            val = cs + s1 + s2 + nm + ka + kb;
                            rare = false;
                        }
                        // full mode: triu in framed coordinates (only the tiles that reach below the diagonal test for it);
                        // the exact evaluation of a near-threshold window is skipped where nothing depends on it: windows
                        // without signal (s2 is an exact sum: 0 means all-zero, the coefficient is 0 either way) and, on the
                        // rim of the band, pixels that are not produced -- the empty corners of a narrow band's outer tiles
                        // used to take the rolled loop below eight times per half
                        bool live = s2 > 0.0f;
                        if (tile_forced) {
                            const bool forced = d + (kn - km) < 0;
                            if (forced) val = 0.0f;
                            live &= !forced;
                        }
                        if (!plain_out) live &= (i < EA->row_end) & (j >= 0) & (j < EA->ns) & (d >= EA->out_lo) & (d <= EA->out_hi);
                        if (rare && live) rare_bits |= 1u << (4 * cc + v);
                        rv[cc][v] = val;
                    }
                }
                // windows whose sums fall under the 1e-4 thresholds (rare): ONE inlined copy of the exact function
                // per half instead of one per pixel (16 copies: 100 KB of code; a call pins the epilogue to the stack)
#pragma unroll 1
                for (int k = 0; k < (CAND ? 0 : 8); ++k) {      // (candidate mode: such pixels carry the sentinel)
                    if (!__builtin_amdgcn_ballot_w64((rare_bits >> k) != 0)) break;
                    if ((rare_bits >> k) & 1u) {
                        float cs = 0.0f, s1 = 0.0f, s2 = 0.0f, nm = 0.0f, ka = 0.0f, kb = 0.0f;
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            const int c = 2 * half + (e >> 2), v = e & 3;
                            if (e == k) {
                                cs = acc[c][v] * u_cs;
                                s1 = S1[c][v] * unscale;
                                s2 = (S2[c][v] * u_s2) * unscale;
                                nm = nmv[e >> 2][v];
                                ka = kav[e >> 2][v];
                                kb = kbv[e >> 2][v];
                            }
                        }
                        const float val = pearson_masked_f32(cs, s1, s2, nm, ka, kb, KS);
#pragma unroll
                        for (int e = 0; e < 8; ++e)
                            if (e == k) rv[e >> 2][e & 3] = val;
                    }
                }
                MF_STAMP(10);     // emit: coefficients
                if constexpr (CAND) {
                    // candidate mode: no map leaves the kernel, only the coordinates of the pixels that carry the
                    // sentinel (1e-4 of them), appended to the caller's list -- one atomic per wave and column that
                    // has any.  EA->out = the list (keys tag + row * ns + col), EA->nobs = its counter, EA->ld_out = its
                    // capacity, EA->row0_out = the tag (cs_api_foci.cpp find_candidates / cs_detect_foci_blocks).
                    unsigned long long* keys = reinterpret_cast<unsigned long long*>(EA->out);
                    unsigned long long* counter = reinterpret_cast<unsigned long long*>(EA->nobs);
                    // (one test for the half's 8 x 64 pixels first: 1e-4 of the pixels are candidates, so nearly every half
                    // skips the per-pixel range tests and votes)
                    float top = rv[0][0];
#pragma unroll
                    for (int e = 1; e < 8; ++e) top = fmaxf(top, rv[e >> 2][e & 3]);
                    if (!__builtin_amdgcn_ballot_w64(top >= KS.cand_thr)) continue;
#pragma unroll
                    for (int cc = 0; cc < 2; ++cc) {
#pragma unroll
                        for (int v = 0; v < 4; ++v) {
                            const int j = J0 + 16 * (2 * half + cc) + 4 * g + v;
                            const int d = j - i;
                            const bool hit = (rv[cc][v] >= KS.cand_thr) & (i < EA->row_end) & (j >= 0) & (j < EA->ns) &
                                             (d >= EA->out_lo) & (d <= EA->out_hi);
                            const unsigned long long m = __builtin_amdgcn_ballot_w64(hit);
                            if (m) {                                          // wave-uniform, rare
                                const int first = __builtin_ctzll(m);
                                unsigned long long base = 0;
                                if (lane == first) base = atomicAdd(counter, (unsigned long long)__builtin_popcountll(m));
                                const unsigned lo = __builtin_amdgcn_readlane((unsigned)base, first);
                                const unsigned hi = __builtin_amdgcn_readlane((unsigned)(base >> 32), first);
                                const unsigned long long pos = (((unsigned long long)hi << 32) | lo) +
                                                               (unsigned long long)__builtin_popcountll(m & ((1ull << lane) - 1ull));
                                if (hit && pos < (unsigned long long)EA->ld_out)
                                    keys[pos] = (unsigned long long)EA->row0_out + (unsigned long long)i * (unsigned long long)EA->ns + (unsigned long long)j;
                            }
                        }
                    }
                    continue;
                }
                // 16 rows x 32 columns through the wave's scratch (pitch 36 floats).  Tiles that are produced entirely
                // (77 % of a wide band) leave as 8 rows x 128 consecutive bytes per instruction, four floats per lane --
                // band rows are shifted against each other by one element, so these 16-byte stores are only 4-byte
                // aligned, which global memory accepts; the tiles on the rim of the band take 2 rows x 32 floats per
                // instruction under per-pixel predicates, the eight scratch reads in flight together (one read, one
                // wait, one store at a time made the stores a sixth of the kernel).
                const int pass_n = EA->nobs ? 2 : 1;
                for (int pass = 0; pass < pass_n; ++pass) {
                    wave_lds_sync();
                    f4 t0 = rv[0], t1 = rv[1];
                    if (pass) {
#pragma unroll
                        for (int v = 0; v < 4; ++v) {
                            t0[v] = KS.n - nmv[0][v];
                            t1[v] = KS.n - nmv[1][v];
                        }
                    }
                    *reinterpret_cast<f4*>(tb + n * 36 + 4 * g) = t0;
                    *reinterpret_cast<f4*>(tb + n * 36 + 16 + 4 * g) = t1;
                    wave_lds_sync();
                    if (plain_out) {
                        const int rr = lane >> 3, c4 = 4 * (lane & 7);
                        const f4 lo = *reinterpret_cast<const f4*>(tb + rr * 36 + c4);
                        const f4 hi = *reinterpret_cast<const f4*>(tb + (rr + 8) * 36 + c4);
                        const int oi = I0 + wr0 + rr, oj = J0 + 32 * half + c4;
                        const long long idx = ((long long)oi - EA->row0_out) * EA->ld_out + (EA->band_out ? oj - oi - EA->lo_out : oj);
                        const long long idx8 = idx + 8 * (long long)EA->ld_out - (EA->band_out ? 8 : 0);
                        if (pass == 1) {
                            *reinterpret_cast<f4u*>(EA->nobs + idx) = lo;
                            *reinterpret_cast<f4u*>(EA->nobs + idx8) = hi;
                        } else if (EA->out_is_f64) {
                            double* od = reinterpret_cast<double*>(EA->out);
                            d2u a, b;
                            a[0] = lo[0]; a[1] = lo[1]; b[0] = lo[2]; b[1] = lo[3];
                            *reinterpret_cast<d2u*>(od + idx) = a;
                            *reinterpret_cast<d2u*>(od + idx + 2) = b;
                            a[0] = hi[0]; a[1] = hi[1]; b[0] = hi[2]; b[1] = hi[3];
                            *reinterpret_cast<d2u*>(od + idx8) = a;
                            *reinterpret_cast<d2u*>(od + idx8 + 2) = b;
                        } else {
                            float* of = reinterpret_cast<float*>(EA->out);
                            *reinterpret_cast<f4u*>(of + idx) = lo;
                            *reinterpret_cast<f4u*>(of + idx8) = hi;
                        }
                        continue;
                    }
                    // tiles on the rim of the band (or of the matrix): the same lane -> (row, four columns) mapping as above; the
                    // produced columns of a row are ONE interval (inside the matrix, on the band's diagonals), so a lane's
                    // four are all produced (one 16-byte store, as on the inner tiles), none, or -- once per row -- some
                    // (up to four 4-byte stores).  The first version stored every pixel by itself under its own predicate: eight
                    // store instructions per wave and half for two, 4 700 cycles more per rim tile than an inner one.
                    const int rr = lane >> 3, c4 = 4 * (lane & 7);
                    const f4 lo = *reinterpret_cast<const f4*>(tb + rr * 36 + c4);
                    const f4 hi = *reinterpret_cast<const f4*>(tb + (rr + 8) * 36 + c4);
                    const int oj = J0 + 32 * half + c4;
#pragma unroll
                    for (int part = 0; part < 2; ++part) {
                        const int oi = I0 + wr0 + rr + 8 * part;
                        const f4 v4 = part ? hi : lo;
                        const int first = max(oj, max(0, oi + EA->out_lo)), last = min(oj + 3, min(EA->ns - 1, oi + EA->out_hi));
                        const bool row_ok = !MFD_DBG(1) & (oi < EA->row_end);
                        const long long idx = ((long long)oi - EA->row0_out) * EA->ld_out + (EA->band_out ? oj - oi - EA->lo_out : oj);
                        if (row_ok & (first == oj) & (last == oj + 3)) {
                            if (pass == 1) {
                                *reinterpret_cast<f4u*>(EA->nobs + idx) = v4;
                            } else if (EA->out_is_f64) {
                                double* od = reinterpret_cast<double*>(EA->out);
                                d2u a, b;
                                a[0] = v4[0]; a[1] = v4[1]; b[0] = v4[2]; b[1] = v4[3];
                                *reinterpret_cast<d2u*>(od + idx) = a;
                                *reinterpret_cast<d2u*>(od + idx + 2) = b;
                            } else {
                                *reinterpret_cast<f4u*>(reinterpret_cast<float*>(EA->out) + idx) = v4;
                            }
                        } else if (row_ok & (first <= last)) {
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                if ((oj + e >= first) & (oj + e <= last)) {
                                    if (pass == 1) EA->nobs[idx + e] = v4[e];
                                    else if (EA->out_is_f64) reinterpret_cast<double*>(EA->out)[idx + e] = (double)v4[e];
                                    else reinterpret_cast<float*>(EA->out)[idx + e] = v4[e];
                                }
                            }
                        }
                    }
                }
                MF_STAMP(11);     // emit: stores
            }
            return;
        }
        if constexpr (!TABLE) {                  // (the unmasked epilogue: never part of a table instance)
        const bool plain = I0 + MF_T <= A.row_end && J0 + MF_T <= A.ns &&
                           (A.full || (I0 >= kh && I0 + MF_T - 1 <= A.ms - km + kh && J0 >= kw && J0 + MF_T - 1 <= A.ns - kn + kw)) &&
                           (!A.sym_upper || J0 - (I0 + MF_T - 1) + (A.full ? kn - km : 0) >= 0);
        const int i = I0 + wr0 + n;
        const long long o_idx = ((long long)i - A.row0_out) * A.ld_out + (J0 + 4 * g);
        f4 rv[4];
        // Lean form on the tile-scaled sums.  unscale (2^-ex), u_s2 / unscale (32) and w_unscale are powers of two and the
        // coefficient is scale-invariant: with S1, S2' = 32 S2, cw = acc w_unscale the true sums are s1 = S1 u, s2 = S2' u^2,
        // cs = cw u (u = unscale), so A = s2 n - s1^2 = u^2 (S2 32n - S1^2) and r = cs rsq(A kvar) = cw rsq(A' kvar) -- the
        // same operations on operands scaled by powers of two (the result may still differ in the last bits: v_rsq_f32 is
        // an approximation, not promised to be invariant under 4^k).  The thresholds move to the tile's units instead (one scaling per tile): every
        // decision (eps cut, the three 1e-4 tests) falls on the same pixels as long as the scaled thresholds are normal
        // floats and no true-domain term (s1^2, s2 n, den2) can overflow; other tiles, plain xcorr2, candidate mode and any
        // wave holding a near-threshold window take the literal per-pixel form below.
        bool lean = !A.xcorr_only && !MFD_DBG(32) && !(MFD_NOMASK_KS.cand_cmin > 0.0f);
        if (lean) {
            const KernelStats<float>& KS = MFD_NOMASK_KS;
            const float inv_u = __uint_as_float((254u << 23) - __float_as_uint(unscale));          // 2^ex, exact
            const float t1 = KS.thr_n * inv_u;                          // |s1|, |c| >= thr_n
            const float t2 = (t1 * inv_u) * 0.03125f;                   // s2 >= thr_n
            const float td = (KS.den2_min * inv_u) * inv_u;             // den2 >= den2_min
            // (scaled sums: |S1| < 2^16, 32 n S2 < 2^31, so every true-domain term -- s1^2, s2 n, den2 -- is below this)
            const float top = (fmaxf(KS.kvar, 1.0f) * 4294967296.0f) * (unscale * unscale);
            auto normal_or_0 = [](float x) { return x == 0.0f || (x >= 1.17549435e-38f && x <= 3.40282347e38f); };
            lean = normal_or_0(t1) && normal_or_0(t2) && normal_or_0(td) && td > 0.0f && top <= 3.40282347e38f;
            if (lean) {
                const float n32 = 32.0f * KS.n, wu = A.w_unscale;
                bool normal = true;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
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
        for (int c = 0; c < 4; ++c) {
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const float cs = acc[c][v] * u_cs;
                const float s1 = S1[c][v] * unscale;
                const float s2 = (S2[c][v] * u_s2) * unscale;
                rv[c][v] = A.xcorr_only ? (fabsf(cs) < A.ks.thr ? 0.0f : cs)            // detection.py:716-722
                                        : MFD_DBG(32) ? cs + s1 + s2
                                                       : cand_range_guard(pearson_nomask_lean(cs, s1, s2, MFD_NOMASK_KS), s2, unscale, MFD_NOMASK_KS);
            }
        }
        if MFD_DBG(1) {
            if (rv[0][0] == 123.456f) reinterpret_cast<float*>(A.out)[o_idx] = rv[1][1] + rv[2][2] + rv[3][3];
        } else if (plain && VEC4) {
            // A lane holds 4 consecutive columns of ONE row per column tile: stored directly, every
            // instruction would touch 16 rows with 64 bytes each (measured: 4x the cost of the same bytes
            // at consecutive addresses).  Two column tiles at a time go through the wave's scratch
            // (16 rows x 32 columns, pitch 36 floats) and leave as 8 rows x 128 contiguous bytes.
            float* tb = reinterpret_cast<float*>(scr);
            const long long r_idx = ((long long)(I0 + wr0 + (lane >> 3)) - A.row0_out) * A.ld_out + J0 + 4 * (lane & 7);
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                wave_lds_sync();
                *reinterpret_cast<f4*>(tb + n * 36 + 4 * g) = rv[2 * half];
                *reinterpret_cast<f4*>(tb + n * 36 + 16 + 4 * g) = rv[2 * half + 1];
                wave_lds_sync();
                const f4 lo = *reinterpret_cast<const f4*>(tb + (lane >> 3) * 36 + 4 * (lane & 7));
                const f4 hi = *reinterpret_cast<const f4*>(tb + ((lane >> 3) + 8) * 36 + 4 * (lane & 7));
                if (A.out_is_f64) {
                    typedef double d2 __attribute__((ext_vector_type(2)));
                    double* od = reinterpret_cast<double*>(A.out) + r_idx + 32 * half;
                    d2 a, b;
                    a[0] = lo[0]; a[1] = lo[1]; b[0] = lo[2]; b[1] = lo[3];
                    *reinterpret_cast<d2*>(od) = a;
                    *reinterpret_cast<d2*>(od + 2) = b;
                    a[0] = hi[0]; a[1] = hi[1]; b[0] = hi[2]; b[1] = hi[3];
                    *reinterpret_cast<d2*>(od + 8 * A.ld_out) = a;
                    *reinterpret_cast<d2*>(od + 8 * A.ld_out + 2) = b;
                } else {
                    float* of = reinterpret_cast<float*>(A.out) + r_idx + 32 * half;
                    *reinterpret_cast<f4*>(of) = lo;
                    *reinterpret_cast<f4*>(of + 8 * A.ld_out) = hi;
                }
            }
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int j = J0 + 16 * c + 4 * g + v;
                    bool z = false;
                    if (!A.full) z = (i < kh) | (i > A.ms - km + kh) | (j < kw) | (j > A.ns - kn + kw);
                    if (A.sym_upper) z = z | ((j - i) + (A.full ? (kn - km) : 0) < 0);
                    if (i < A.row_end && j < A.ns) {
                        const float val = z ? 0.0f : rv[c][v];
                        if (A.out_is_f64) reinterpret_cast<double*>(A.out)[o_idx + 16 * c + v] = (double)val;
                        else reinterpret_cast<float*>(A.out)[o_idx + 16 * c + v] = val;
                    }
                }
            }
        }
        }
    };

    f4 p_acc[4], p_S1[4], p_S2[4], p_hdr = zero4;
    int p_I0 = 0, p_J0 = 0, p_slot = 0, slot = 0;
    float p_unscale = 0.0f;
    bool pending = false;
#pragma unroll
    for (int c = 0; c < 4; ++c) p_acc[c] = p_S1[c] = p_S2[c] = zero4;

    // Tile sequence of this workgroup.  Workgroups are dealt round-robin to the 8 XCDs (own L2 each): XCD x
    // takes the tiles [x n / 8, (x + 1) n / 8) and its workgroups walk that range side by side, so the 16
    // halo rows / columns neighbouring tiles share are re-read from the XCD's own L2.
    int tile, tile_end, tile_step;
    if constexpr (TABLE) {
        tile = table_tile;
        tile_end = table_tile_end;
        tile_step = table_tile_step;
    } else if ((A.xcd_order & 1) && gridDim.x % 8 == 0) {
        const int x = blockIdx.x & 7, per = (A.n_tiles + 7) / 8;
        tile = x * per + (blockIdx.x >> 3);
        tile_end = min(A.n_tiles, (x + 1) * per);
        tile_step = gridDim.x >> 3;
    } else {
        tile = blockIdx.x;
        tile_end = A.n_tiles;
        tile_step = gridDim.x;
    }
    if MFD_DBG(2048) return;                  // diagnostics: launch + dispatch only
    if (tile < tile_end) fetch(tile, 0);       // the first tile is on its way while the weights are loaded

    // ---- weights.  General templates: heads of all 17 template rows in registers (rows >= km are zero), tails in LDS.
    // RSYM (rows mirror, s and 16 - s alike): nine rows of tails AND nine rows of heads in LDS (slots 0..8 / 9..17) --
    // 36 registers that were live through the epilogue, which is where the masked instances ran out of them.
    constexpr int kHeads = RSYM ? 1 : 17;
    h8 wh[kHeads];
    {
        const h8* frag = reinterpret_cast<const h8*>(A.frag);
        h8 z;
#pragma unroll
        for (int e = 0; e < 8; ++e) z[e] = (_Float16)0.0f;
        if constexpr (!RSYM) {
#pragma unroll
            for (int s = 0; s < kHeads; ++s) {
                const int sc = min(s, km - 1);
                const h8 a = frag[(2 * sc + 0) * 64 + lane];
                wh[s] = s < km ? a : z;
            }
        } else {
            wh[0] = z;
        }
        constexpr int kSlots = RSYM ? 18 : 17;
        h8 tails[5];                                   // 17 (18) x 64 fragments = 4.25 (4.5) per thread: loads first
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const int idx = min(tid + 256 * k, kSlots * 64 - 1);
            const int slot = idx >> 6;
            const int row = RSYM ? (slot < 9 ? slot : slot - 9) : slot, part = RSYM ? (slot < 9 ? 1 : 0) : 1;
            tails[k] = frag[(2 * min(row, km - 1) + part) * 64 + (idx & 63)];
        }
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const int idx = tid + 256 * k;
            const int slot = idx >> 6;
            const int row = RSYM ? (slot < 9 ? slot : slot - 9) : slot;
            if (idx < kSlots * 64) reinterpret_cast<h8*>(smem + MFD_WL)[idx] = row < km ? tails[k] : z;
        }
    }
    // REG: one emit site (its epilogue is 4 K instructions) -- the loop runs one pass beyond the last tile, in which
    // only the pending tile is emitted.  The dense instances emit the last tile after the loop.
    MF_WALL(12);
    for (;; tile += tile_step) {
        const bool have = REG ? tile < tile_end : true;              // uniform over the workgroup
        if constexpr (REG) {
            if (!have && !pending) break;
        } else {
            if (tile >= tile_end) break;
        }
        int I0 = 0, J0 = 0;
        if (have) tile_origin(tile, I0, J0);
        const int P0 = I0 - kh, Q0 = J0 - kw;
        // every staged pixel exists (rows, columns and, for a banded input, stored diagonals): the transfers were not
        // clamped and the reader needs no masks
        bool inside = P0 >= p_min && P0 + MF_R - 1 <= p_max && Q0 >= 0 && Q0 + MF_R <= A.ns;
        if (REG && A.band_in) inside = inside && Q0 - (P0 + MF_R - 1) - A.lo_in >= 0 && Q0 + MF_R - 1 - P0 - A.lo_in <= A.bw_in - 1;
        if (REG && VEC4) inside = inside || (P0 >= pad_row0 && P0 + MF_R - 1 <= p_max);     // (see fetch)
        if (REG && MFD_DBG(512)) inside = true;
        if MFD_DBG(1024) {                    // diagnostics: prologue only
            if (!have) break;
            continue;
        }
        float unscale = 0.0f;
#ifdef CS_MF_PROFILE
        tprev_ = __builtin_readcyclecounter();
        if (tid == 0 && have) prof_lds[15] += 1ull;
#endif
        if (have) {

            // (CS_LAYOUT_BAND_COUNTS: the tile in `raw` holds raw counts, and the weights of its 80 rows and 80 columns and the
            // reciprocal law of its 160 diagonals have landed in the first wave's store scratch -- see fetch)
            bool cnt_tile = false;
            if constexpr (REG && VEC4) cnt_tile = A.cnt_in != 0;

            // ---- the tile's pixels have landed in `raw`: read this thread's 14 x 2, find the scale
            __builtin_amdgcn_s_waitcnt(0x0f70);      // vmcnt(0): this wave's DMA transfers (and long-retired stores)
            lds_barrier();                           // everyone's transfers; the previous tile's plane readers are done
            float xa[MFD_ROWS_PER_THREAD], xb[MFD_ROWS_PER_THREAD];
            float amax = 0.0f;
            if (inside) {
#pragma unroll
                for (int k = 0; k < MFD_ROWS_PER_THREAD; ++k) {
                    const int r = rg + 6 * k;
                    float2 v = make_float2(0.0f, 0.0f);
                    if (stager && r < MF_R) v = *reinterpret_cast<const float2*>(raw + r * MF_R + 2 * c2);
                    xa[k] = v.x;
                    xb[k] = v.y;
                    amax = fmaxf(amax, fmaxf(fabsf(v.x), fabsf(v.y)));
                }
            } else {
                int c2 = c2_, rg = rg_;               // (opaque copies: see fetch)
                if constexpr (REG) asm volatile("" : "+v"(c2), "+v"(rg));
#pragma unroll
                for (int k = 0; k < MFD_ROWS_PER_THREAD; ++k) {
                    const int r = rg + 6 * k;
                    float a = 0.0f, b = 0.0f;
                    if (REG && VEC4) {
                        if (stager && r < MF_R) {
                            // pieces of 4 whose start was clamped into the stored range of their row: element o of the
                            // piece holds stored index idx_c + o
                            const int p = P0 + r, q = Q0 + 2 * c2, cs = (2 * c2) & ~3;
                            const int w = A.band_in ? A.bw_in : A.ns;
                            const int off = A.band_in ? p + A.lo_in : 0;
                            const int idx_s = Q0 + cs - off;
                            const int idx_c = min(max(idx_s, 0), w - 4);
                            const int oa = (2 * c2 - cs) + (idx_s - idx_c), ob = oa + 1;
                            const int idx_a = q - off;
                            const bool rok = (p >= p_min) & (p <= p_max);
                            const bool oka = rok & (q >= 0) & (q < A.ns) & (idx_a >= 0) & (idx_a < w) & (oa >= 0) & (oa < 4);
                            const bool okb = rok & (q + 1 >= 0) & (q + 1 < A.ns) & (idx_a + 1 >= 0) & (idx_a + 1 < w) & (ob >= 0) & (ob < 4);
                            const float* piece = raw + r * MF_R + cs;
                            a = oka ? piece[min(max(oa, 0), 3)] : 0.0f;
                            b = okb ? piece[min(max(ob, 0), 3)] : 0.0f;
                        }
                    } else if (stager && r < MF_R) {
                        const float2 v = *reinterpret_cast<const float2*>(raw + r * MF_R + 2 * c2);
                        const int p = P0 + r, q = Q0 + 2 * c2;
                        const bool rok = (p >= p_min) & (p <= p_max);
                        bool oka = rok & (q >= 0) & (q < A.ns), okb = rok & (q + 1 >= 0) & (q + 1 < A.ns);
                        if (REG && A.band_in) {               // outside the stored diagonals: zero
                            const int dd = q - p - A.lo_in;
                            oka &= (dd >= 0) & (dd < A.bw_in);
                            okb &= (dd + 1 >= 0) & (dd + 1 < A.bw_in);
                        }
                        a = oka ? v.x : 0.0f;
                        b = okb ? v.y : 0.0f;
                    }
                    xa[k] = a;
                    xb[k] = b;
                    amax = fmaxf(amax, fmaxf(fabsf(a), fabsf(b)));
                }
            }
            if (cnt_tile) {
                // balance and detrend what was fetched (contacts_map.py:531-540, preprocessing.py:296-302): count * w_row * w_col *
                // (1 / law), NaN -> 0, >= max_val -> 1.  In float32 on float32 copies of the weights and of the reciprocals (two
                // pixels per packed instruction): within 6 units in the last place of the float64 expression rounded once -- the
                // detrended band's value -- which is 2 % of the rounding the kernel's own sums carry (n 2^-24, the error model of
                // the candidate screen, cs_device.h).  [The float64 expression itself, 5 double-precision instructions per pixel, cost
                // 10 % of the kernel.]  The cap is a DISCRETE decision: a tile with a product within 2e-6 of max_val -- where the
                // float32 and the float64 product may fall on different sides -- is converted again by the staging pass's own
                // function (stage_detrend_rcp) on the float64 tables: once in ~1e5 tiles.
                const float* cwin = reinterpret_cast<const float*>(smem + MFD_SCR);        // [0, 80) rows, [80, 160) columns, [160, 320) diagonals
                int c2 = c2_, rg = rg_;               // (opaque copies: see fetch)
                asm volatile("" : "+v"(c2), "+v"(rg));
                typedef float f2 __attribute__((ext_vector_type(2)));
                const f2 cw = *reinterpret_cast<const f2*>(cwin + 80 + 2 * c2);
                const float max_f = cnt_max > 0.0f ? cnt_max : __uint_as_float(0x7f800000u);
                float thin_min = __uint_as_float(0x7f800000u);        // smallest |product - max_val| of the thread's pixels
                float fa[MFD_ROWS_PER_THREAD], fb[MFD_ROWS_PER_THREAD];
                amax = 0.0f;
                // (one base per table and compile-time offsets: the rows 80 .. 83 of the last step of the row groups 2 .. 5 do not
                // exist -- their counts were read as 0, and what the neighbouring table delivers for them multiplies that 0)
                const float* wrow = cwin + rg;
                const float* rld = cwin + 160 + (MF_R - 1) + 2 * c2 - rg - 6 * (MFD_ROWS_PER_THREAD - 1);     // (the last step's: offsets >= 0)
#pragma unroll
                for (int k = 0; k < MFD_ROWS_PER_THREAD; ++k) {
                    const float rwk = wrow[6 * k];
                    f2 rl;
                    rl[0] = rld[6 * (MFD_ROWS_PER_THREAD - 1 - k)];
                    rl[1] = rld[6 * (MFD_ROWS_PER_THREAD - 1 - k) + 1];
                    f2 x;
                    x[0] = xa[k];
                    x[1] = xb[k];
                    f2 o = ((x * f2{rwk, rwk}) * cw) * rl;
                    const f2 t = o - f2{max_f, max_f};
                    thin_min = fminf(fminf(fabsf(t[0]), fabsf(t[1])), thin_min);          // (fminf ignores a NaN operand)
                    float a = fmaxf(o[0], 0.0f), b = fmaxf(o[1], 0.0f);      // NaN -> 0; the caller vouches that no count and no weight
                    a = a >= max_f ? 1.0f : a;                                // is negative (include/chromosight_hip.h band32_counts)
                    b = b >= max_f ? 1.0f : b;
                    fa[k] = a;
                    fb[k] = b;
                    amax = fmaxf(amax, fmaxf(a, b));
                }
                bool thin_any = __builtin_amdgcn_ballot_w64(thin_min <= max_f * 2e-6f) != 0;
                if (thin_any && cnt_max > 0.0f) {
                    const CountsHdrPtr H = counts_header(A.sig);
                    const int hn = H->n, hd = H->n_diags;
                    const double* wt = H->weight + H->row0;
                    const double* law = H->law;
                    const double* rlaw = H->rlaw;
                    const double max_val = H->max_val;
                    amax = 0.0f;
#pragma unroll 1
                    for (int k = 0; k < MFD_ROWS_PER_THREAD; ++k) {
                        const int r = rg + 6 * k;
                        const int p = P0 + r, q = Q0 + 2 * c2, d = q - p;
                        const double rwk = wt[min(max(p, 0), hn - 1)];
                        // the pixel pair's counts once more from `raw` (still whole: the barrier behind the scale comes later) --
                        // kept in registers through the float32 pass above they cost it 3 % of the kernel
                        float xk = 0.0f, yk = 0.0f;
                        if (stager && r < MF_R) {
                            if (inside) {
                                const float2 v = *reinterpret_cast<const float2*>(raw + r * MF_R + 2 * c2);
                                xk = v.x;
                                yk = v.y;
                            } else {
                                const int cs = (2 * c2) & ~3;
                                const int w = A.band_in ? A.bw_in : A.ns;
                                const int off = A.band_in ? p + A.lo_in : 0;
                                const int idx_s = Q0 + cs - off;
                                const int idx_c = min(max(idx_s, 0), w - 4);
                                const int oa = (2 * c2 - cs) + (idx_s - idx_c), ob = oa + 1;
                                const int idx_a = q - off;
                                const bool rok = (p >= p_min) & (p <= p_max);
                                const bool oka = rok & (q >= 0) & (q < A.ns) & (idx_a >= 0) & (idx_a < w) & (oa >= 0) & (oa < 4);
                                const bool okb = rok & (q + 1 >= 0) & (q + 1 < A.ns) & (idx_a + 1 >= 0) & (idx_a + 1 < w) & (ob >= 0) & (ob < 4);
                                const float* piece = raw + r * MF_R + cs;
                                xk = oka ? piece[min(max(oa, 0), 3)] : 0.0f;
                                yk = okb ? piece[min(max(ob, 0), 3)] : 0.0f;
                            }
                        }
                        const int da = min(max(d, 0), hd - 1), db = min(max(d + 1, 0), hd - 1);
                        const float a = (float)stage_detrend_rcp(((double)xk * rwk) * wt[min(max(q, 0), hn - 1)], rlaw[da], max_val, law + da);
                        const float b = (float)stage_detrend_rcp(((double)yk * rwk) * wt[min(max(q + 1, 0), hn - 1)], rlaw[db], max_val, law + db);
#pragma unroll
                        for (int e = 0; e < MFD_ROWS_PER_THREAD; ++e) {
                            fa[e] = e == k ? a : fa[e];
                            fb[e] = e == k ? b : fb[e];
                        }
                        amax = fmaxf(amax, fmaxf(fabsf(a), fabsf(b)));
                    }
                }
#pragma unroll
                for (int k = 0; k < MFD_ROWS_PER_THREAD; ++k) {
                    xa[k] = fa[k];
                    xb[k] = fb[k];
                }
            }
            amax = wave_max_nonneg(amax);
            if (lane == 63) red[wv] = __float_as_uint(amax);
            if constexpr (REG) {
                // the tile's column flags as bit masks (bit t = staged column Q0 + t), zero outside the matrix (the
                // transfer clamped its addresses)
                if (wv < 2) {
                    const int q = Q0 + tid;
                    const long long start = (long long)(uintptr_t)A.miss_col + Q0;
                    const int skew = (int)(start - ((start >> 2) << 2));           // bytes before column Q0 in the first dword
                    const uint8_t fb = reinterpret_cast<const uint8_t*>(smem + MFD_CFB)[slot * 128 + skew + min(tid, 79)];
                    const bool flagged = tid < 80 && q >= 0 && q < A.ns && fb;
                    const unsigned long long m = __builtin_amdgcn_ballot_w64(flagged);
                    unsigned* cfm = reinterpret_cast<unsigned*>(smem + MFD_CFL) + slot * 4;
                    if (lane == 0) {
                        cfm[2 * wv] = (unsigned)m;
                        if (wv == 0) cfm[1] = (unsigned)(m >> 32);
                    }
                }
            }
            MF_STAMP(0);
            lds_barrier();                           // everyone has read `raw`: the squares may overwrite it
            int ex = 0;
            {
                const uint4 m4 = *reinterpret_cast<const uint4*>(red);
                const unsigned mx = max(max(m4.x, m4.y), max(m4.z, m4.w));     // non-negative floats order as integers
                const int e = (int)((mx >> 23) & 0xffu);
                if (e != 0 && e != 255) ex = 6 - (e - 127);
                ex = max(-100, min(100, ex));
            }
            const float scale = __uint_as_float((unsigned)(ex + 127) << 23);
            const float qscale = __uint_as_float((unsigned)(ex + 127 - 5) << 23);   // 2^-5: 17-sums of squares < 65504
            unscale = __uint_as_float((unsigned)(127 - ex) << 23);
            typedef __fp16 hv2 __attribute__((ext_vector_type(2)));
#pragma unroll
            for (int k = 0; k < MFD_ROWS_PER_THREAD; ++k) {
                const int r = rg + 6 * k;
                if (stager && r < MF_R && !MFD_DBG(16)) {
                    // heads by truncation, tails exact differences: head + tail carries 21-22 bits either way
                    const float a = xa[k] * scale, b = xb[k] * scale;
                    const hv2 hh = __builtin_amdgcn_cvt_pkrtz(a, b);
                    const float qa = (xa[k] * qscale) * a, qb = (xb[k] * qscale) * b;
                    const hv2 qh = __builtin_amdgcn_cvt_pkrtz(qa, qb);
                    hv2 tt, qt;
                    if constexpr (!REG) {
                        // (the tails straight from the packed heads: one v_fma_mix_f32 per value instead of a convert and a
                        // subtraction -- the same exact differences; the masked instances keep their statement order)
                        const unsigned hu = __builtin_bit_cast(unsigned, hh), qu = __builtin_bit_cast(unsigned, qh);
                        tt = __builtin_amdgcn_cvt_pkrtz(sub_f16_lo(a, hu), sub_f16_hi(b, hu));
                        qt = __builtin_amdgcn_cvt_pkrtz(sub_f16_lo(qa, qu), sub_f16_hi(qb, qu));
                    } else {
                        tt = __builtin_amdgcn_cvt_pkrtz(a - (float)hh[0], b - (float)hh[1]);
                        qt = __builtin_amdgcn_cvt_pkrtz(qa - (float)qh[0], qb - (float)qh[1]);
                    }
                    const int o = (r * MF_R + 2 * c2) * 2;
                    *reinterpret_cast<hv2*>(pl_xh + o) = hh;
                    *reinterpret_cast<hv2*>(pl_xl + o) = tt;
                    *reinterpret_cast<hv2*>(pl_qh + o) = qh;
                    *reinterpret_cast<hv2*>(pl_ql + o) = qt;
                }
            }
            MF_STAMP(1);
        } else if (REG) {
            __builtin_amdgcn_s_waitcnt(0x0f70);
            lds_barrier();
        }
        // ---- the previous tile's coefficients and stores
        if (pending) emit(p_I0, p_J0, p_unscale, p_acc, p_S1, p_S2, p_hdr, p_slot);
        if (!have) break;
        MF_STAMP(6);
        lds_barrier();

        // ---- box sums: horizontal pass over the wave's 32 input rows (all-ones Toeplitz as B), the
        //      partial sums split again and transposed through the wave's scratch, vertical pass
        //      (all-ones Toeplitz as B again: transposed tile).  8 steps (4 column tiles x {x, x^2}); the
        //      fragments of step t + 1 are loaded before the scratch round trip of step t.
        f4 S1[4], S2[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) S1[c] = S2[c] = zero4;
        if (!MFD_DBG(4) && !A.xcorr_only) {
            auto hfrag = [&](int t, h8 (&f)[4]) {
                const int c = t >> 1;
                const char* ph = (t & 1) ? pl_qh : pl_xh;
                const char* pt = (t & 1) ? pl_ql : pl_xl;
#pragma unroll
                for (int rb = 0; rb < 2; ++rb) {
                    const int off = ((wr0 + 16 * rb + n) * MF_R + 16 * c + 8 * g) * 2;
                    f[2 * rb] = *reinterpret_cast<const h8*>(ph + off);
                    f[2 * rb + 1] = *reinterpret_cast<const h8*>(pt + off);
                }
            };
            h8 cur[4];
            hfrag(0, cur);
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                h8 nxt[4];
                if (t + 1 < 8) hfrag(t + 1, nxt);
                // horizontal sums of the wave's 32 input rows: lane (column n, group g) ends up with rows 4 g + v (rb = 0)
                // and 16 + 4 g + v (rb = 1) of its column -- eight rows of ONE column, which is what a lane of the
                // vertical pass's A operand holds.  The contraction index of an MFMA is only a label, so the rows go
                // in as they are (slot e of group g = row rho(g, e)) against the all-ones Toeplitz operand with its
                // rows permuted the same way (ones_p): no transposition through LDS.
                h8 bh, bl;
                typedef unsigned u4 __attribute__((ext_vector_type(4)));
                u4 bhw, blw;
#pragma unroll
                for (int rb = 0; rb < 2; ++rb) {
                    f4 h = mfma16(cur[2 * rb], ones_b, zero4);
                    h = mfma16(cur[2 * rb + 1], ones_b, h);
                    if constexpr (!REG) {
                        // heads rounded to nearest two at a time (v_cvt_pk_f16_f32), tails by v_fma_mix_f32 from the packed
                        // heads: the same values as the form below in half the instructions
#pragma unroll
                        for (int pr = 0; pr < 2; ++pr) {
                            const unsigned hp = pack_h2((_Float16)h[2 * pr], (_Float16)h[2 * pr + 1]);
                            bhw[2 * rb + pr] = hp;
                            blw[2 * rb + pr] = pack_h2((_Float16)sub_f16_lo(h[2 * pr], hp), (_Float16)sub_f16_hi(h[2 * pr + 1], hp));
                        }
                    } else {
#pragma unroll
                        for (int v = 0; v < 4; ++v) {
                            const _Float16 hh = (_Float16)h[v];
                            bh[4 * rb + v] = hh;
                            bl[4 * rb + v] = (_Float16)(h[v] - (float)hh);
                        }
                    }
                }
                if constexpr (!REG) {
                    bh = __builtin_bit_cast(h8, bhw);
                    bl = __builtin_bit_cast(h8, blw);
                }
                f4 sacc = mfma16(bh, ones_p, zero4);
                sacc = mfma16(bl, ones_p, sacc);
                if (t & 1) S2[t >> 1] = sacc;
                else S1[t >> 1] = sacc;
                if (t + 1 < 8) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) cur[q] = nxt[q];
                }
            }
        }
        MF_STAMP(2);
        lds_barrier();                           // all waves are done with the squares
        // ---- next tile's pixels -> `raw` while this tile's correlation runs
        if (tile + tile_step < tile_end && !MFD_DBG(2)) fetch(tile + tile_step, slot ^ 1);

        MF_STAMP(3);
        // ---- cross term: 17 template rows x 4 column tiles, fragments of row s + 1 in flight during row s
        f4 acc[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] = zero4;
        h8 ah[4], al[4], bl;
        const int fo = ((wr0 + n) * MF_R + 8 * g) * 2;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            ah[c] = *reinterpret_cast<const h8*>(pl_xh + fo + 32 * c);
            al[c] = *reinterpret_cast<const h8*>(pl_xl + fo + 32 * c);
        }
        h8 bh;
        bl = reinterpret_cast<const h8*>(smem + MFD_WL)[lane];
        if constexpr (RSYM) bh = reinterpret_cast<const h8*>(smem + MFD_WL)[9 * 64 + lane];
        else bh = wh[0];
        if (!MFD_DBG(8))
#pragma unroll
        for (int s = 0; s < 17; ++s) {
            h8 nh[4], nl[4], nb, nbh;
            if (s + 1 < 17) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    nh[c] = *reinterpret_cast<const h8*>(pl_xh + fo + (s + 1) * MF_R * 2 + 32 * c);
                    nl[c] = *reinterpret_cast<const h8*>(pl_xl + fo + (s + 1) * MF_R * 2 + 32 * c);
                }
                const int sn = RSYM && s + 1 > 8 ? 16 - (s + 1) : s + 1;
                nb = reinterpret_cast<const h8*>(smem + MFD_WL)[sn * 64 + lane];
                if constexpr (RSYM) nbh = reinterpret_cast<const h8*>(smem + MFD_WL)[(9 + sn) * 64 + lane];
                else nbh = wh[s + 1];
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[c] = mfma16(bh, ah[c], acc[c]);     // weights as A: transposed tile
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[c] = mfma16(bl, ah[c], acc[c]);
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[c] = mfma16(bh, al[c], acc[c]);
            __builtin_amdgcn_sched_barrier(0);
            if (s + 1 < 17) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    ah[c] = nh[c];
                    al[c] = nl[c];
                }
                bl = nb;
                bh = nbh;
            }
        }
        MF_STAMP(4);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            p_acc[c] = acc[c];
            p_S1[c] = S1[c];
            p_S2[c] = S2[c];
        }
        p_I0 = I0;
        p_J0 = J0;
        p_unscale = unscale;
        p_slot = slot;
        if constexpr (REG) p_hdr = *reinterpret_cast<const f4*>(A.rowtab + 4 * (size_t)min(I0 + wr0 + n, A.ms - 1));
        slot ^= 1;
        pending = true;
    }
    MF_WALL(13);
    if constexpr (!REG) {
        if (pending) emit(p_I0, p_J0, p_unscale, p_acc, p_S1, p_S2, p_hdr, p_slot);
    }
    MF_WALL(14);
#ifdef CS_MF_PROFILE
    prof_flush();
#undef MF_PROF_ADD
#define MF_PROF_ADD(k, v) atomicAdd(&cs_mf_prof[k], (unsigned long long)(v))
#endif
