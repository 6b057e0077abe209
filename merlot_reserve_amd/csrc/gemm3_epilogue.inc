// Epilogue of the 256-row bf16 GEMM kernels (gemm3.hip: eight waves of 128 x 64 | 48; gemm4.hip: four waves of 128 x 128 | 96), a TEXT
// fragment included inside the kernel's per-tile block (as a function taking the accumulators by reference the same statements
// allocate ~60 more registers in the aux / column-sum mode and spill).  A wave's 128 x (16 NJ) block of fp32 accumulators, held TRANSPOSED
// (mfma(B-frag, A-frag): the lane holds C[m = 16 i + li][n = 16 j + 4 g + r]), goes to bf16 in HBM through registers and ordinary
// loads / stores (no LDS).  MODE (fixed per launch):
//   0: bias | 1: bias + "rotary" scales | 2: bias + GELU, gelu' copy to c2 | 3: + residual | 4: x aux (+ column sums)
// (the bias is the accumulators' initial value: nothing to add here).
// The including scope provides: acc[MR_EPI_MI][NJ] (MR_EPI_MI = 16-row blocks per wave: 8, or 4 in the 128-row geometry of gemm5.hip), NJ, MODE, ga, lane, g, li, cm0 (the tile's first row), wrow0 / wcol0 (the wave block's
// first row / column), MR_EPI_ROW_FENCE(), item_m0 / item_n0 / qc / fetch_bias (the next tile's bias is fetched here, ahead of the stores: a load consumed
// behind them would wait for them, vmcnt retires in order).
// Every store is issued by every lane (rows >= M / columns >= N go to an out-of-range buffer offset, which the hardware drops), so the
// number of store instructions per tile is fixed: 8 * ceil(NJ / 2), twice that for MODE 2 -- the k-loop's first counted vmcnt wait
// behind an epilogue relies on it.
    const mr_gemm_args& pc = ga.p[0];
    const int eM = (int)pc.M, eN = (int)pc.N;
    const int e_ldc = (int)pc.ldc;
    const __bf16* const pre_src = static_cast<const __bf16*>(MODE == 3 ? pc.residual : pc.aux);
    const int64_t pre_ld = MODE == 3 ? pc.ldr : pc.ldaux;
    const float* const e_rot = pc.rot_tab;
    const int e_rot_rows = (int)pc.rot_rows, e_rot_cols = (int)pc.rot_cols;
    const int e_grp = (int)pc.out_grp, e_gstride = (int)pc.out_grp_stride, e_goff = (int)pc.out_grp_off;
    const void* const dummy = pc.A;
    float* const e_cs = static_cast<float*>(pc.colsum);
    const int64_t e_ldcs = pc.ldcs;
    auto out_row = [&](int gm) -> int { return e_grp > 0 ? (gm / e_grp) * e_gstride + e_goff + gm % e_grp : gm; };
    // output descriptors: every store is issued by every lane; rows >= M / columns >= N get an out-of-range offset
    const unsigned c_bytes = (unsigned)(((int64_t)out_row(eM - 1) * e_ldc + eN) * 2);
    const __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc(pc.C, 0, (int)c_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rc2 = __builtin_amdgcn_make_buffer_rsrc(MODE == 2 ? pc.c2 : pc.C, 0, (int)c_bytes, 0x00020000);

    if (item_m0(qc + 1) >= 0) fetch_bias(item_n0(qc + 1));
    constexpr bool HAS_X = MODE == 3 || MODE == 4;
    constexpr int LXD = 4;                                   // row blocks of the residual / aux tile in flight
    constexpr int NXV = NJ / 2 + (NJ & 1);
    u32x4 lx[HAS_X ? LXD : 1][HAS_X ? NXV : 1];
    auto lx_fetch = [&](int i, u32x4 (&dst)[HAS_X ? NXV : 1]) {
        if constexpr (HAS_X) {
            const int gm = wrow0 + i * 16 + li;
            const __bf16* rowp = pre_src + (int64_t)out_row(gm) * pre_ld;
#pragma unroll
            for (int jp = 0; jp < NJ / 2; ++jp) {       // 16 bytes per lane in the layout of the widened stores
                const int gn = wcol0 + (2 * jp + (g & 1)) * 16 + (g >> 1) * 8;
                dst[jp] = *reinterpret_cast<const u32x4*>((gm < eM && gn < eN) ? (const void*)(rowp + gn) : dummy);
            }
            if (NJ & 1) {
                const int gn = wcol0 + (NJ - 1) * 16 + g * 4;
                const u32x2 v = *reinterpret_cast<const u32x2*>((gm < eM && gn < eN) ? (const void*)(rowp + gn) : dummy);
                dst[NJ / 2] = u32x4{v[0], v[1], 0u, 0u};
            }
        }
    };
    if constexpr (HAS_X) {
#pragma unroll
        for (int i = 0; i < LXD; ++i) lx_fetch(i, lx[i]);
    }
    constexpr bool ROT = MODE == 1;
    f32x4 rotv[ROT ? 2 : 1][ROT ? NJ : 1];
    auto rot_fetch = [&](int i, f32x4 (&dst)[ROT ? NJ : 1]) {
        if constexpr (ROT) {
            const int gm = wrow0 + i * 16 + li;
            const int rr = (gm >= eM) ? 0 : (e_rot_rows >= eM) ? gm : gm % e_rot_rows;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int gn0 = wcol0 + j * 16 + g * 4;      // the lane's 4 columns lie inside one head's first or second 32 dims
                const bool on = (gn0 & 63) < 32 && gn0 < e_rot_cols;
                const f32x4 tv = *reinterpret_cast<const f32x4*>(on ? (const void*)(e_rot + (int64_t)rr * 32 + (gn0 & 63)) : (const void*)e_rot);
                dst[j] = on ? tv : f32x4{1.f, 1.f, 1.f, 1.f};
            }
        }
    };
    if constexpr (ROT) rot_fetch(0, rotv[0]);
    constexpr bool CS = MODE == 4;
    const bool f_cs = CS && e_cs != nullptr;
    f32x4 cs[CS ? NJ : 1];
    if constexpr (CS) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) cs[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    // Stores widened to 16 B: lanes l and l+16 hold columns 4g..4g+3 of adjacent 16-column blocks; one v_permlane16_swap per
    // dword leaves every lane with 8 contiguous columns (lane rows g = 0/2 own block 2jp, columns 0-7 / 8-15; g = 1/3 block 2jp+1)
    auto store_pair = [&](const __amdgpu_buffer_rsrc_t& r, unsigned rowoff, bool mok, int jp, bf16x4 va, bf16x4 vb) {
        u32x2 ua = __builtin_bit_cast(u32x2, va), ub = __builtin_bit_cast(u32x2, vb);
        const auto s0 = __builtin_amdgcn_permlane16_swap(ua[0], ub[0], false, false);
        const auto s1 = __builtin_amdgcn_permlane16_swap(ua[1], ub[1], false, false);
        const int col = wcol0 + (2 * jp + (g & 1)) * 16 + (g >> 1) * 8;
        const unsigned off = (mok && col < eN) ? rowoff + (unsigned)col * 2u : OOB;
        __builtin_amdgcn_raw_buffer_store_b128(u32x4{s0[0], s1[0], s0[1], s1[1]}, r, off, 0, 0);
    };
    // Full-line stores (round 6).  store_pair's wave instruction writes 16 rows x 64 B: half of a 128-byte line per row.  A CU's store path takes whole lines
    // 2-3 x faster (scripts/micro/store_bench.cpp: 16 CUs 24.6 against 11.2 B / clk / CU, one CU 44.7 against 14.4; all 256 at once 5.3 against 5.1 TB/s, the
    // chip's limit), and a K = 768 tile waits for its stores (vmcnt retires in issue order: the k-tile requested behind them waits for all of them).  When the
    // wave's column span is whole lines (64 columns per pair of block pairs: NJ % 4 == 0, i.e. the 256-wide tiles) the lanes of a 16-lane row trade halves
    // first -- lanes 0-7 hand their SECOND block pair to lanes 8-15 and take those lanes' FIRST one (one v_mov_dpp row_ror:8 per dword, written under a bank
    // mask) -- so that instruction 1 writes rows 0-7 and instruction 2 rows 8-15 of the row block, 128 contiguous bytes each.  Same instruction count per tile.
#ifndef MR_EPI_FULL_LINES
#define MR_EPI_FULL_LINES 1
#define MR_EPI_FULL_LINES_DEFAULTED
#endif
    constexpr bool FULL_LINES = MR_EPI_FULL_LINES != 0 && (NJ % 4) == 0;
#ifdef MR_EPI_FULL_LINES_DEFAULTED
#undef MR_EPI_FULL_LINES
#undef MR_EPI_FULL_LINES_DEFAULTED
#endif
    auto store_quad = [&](const __amdgpu_buffer_rsrc_t& r, int i_, int jq, bf16x4 a0, bf16x4 b0, bf16x4 a1, bf16x4 b1) {
        auto widen = [&](bf16x4 va, bf16x4 vb) -> u32x4 {
            const u32x2 ua = __builtin_bit_cast(u32x2, va), ub = __builtin_bit_cast(u32x2, vb);
            const auto s0 = __builtin_amdgcn_permlane16_swap(ua[0], ub[0], false, false);
            const auto s1 = __builtin_amdgcn_permlane16_swap(ua[1], ub[1], false, false);
            return u32x4{s0[0], s1[0], s0[1], s1[1]};
        };
        const u32x4 X = widen(a0, b0), Y = widen(a1, b1);          // the lane's 16 bytes of (row li, block pair 2 jq) and (row li, block pair 2 jq + 1)
        u32x4 T1, T2;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            T1[d] = (unsigned)__builtin_amdgcn_update_dpp((int)X[d], (int)Y[d], 0x128, 0xF, 0xC, false);     // lanes 8-15: lane - 8's second pair
            T2[d] = (unsigned)__builtin_amdgcn_update_dpp((int)Y[d], (int)X[d], 0x128, 0xF, 0x3, false);     // lanes 0-7: lane + 8's first pair
        }
        const int gm1 = wrow0 + i_ * 16 + (li & 7), gm2 = gm1 + 8;
        const int col = wcol0 + (2 * (2 * jq + (li >> 3)) + (g & 1)) * 16 + (g >> 1) * 8;
        const unsigned off1 = (gm1 < eM && col < eN) ? (unsigned)out_row(gm1) * (unsigned)e_ldc * 2u + (unsigned)col * 2u : OOB;
        const unsigned off2 = (gm2 < eM && col < eN) ? (unsigned)out_row(gm2) * (unsigned)e_ldc * 2u + (unsigned)col * 2u : OOB;
        __builtin_amdgcn_raw_buffer_store_b128(T1, r, off1, 0, 0);
        __builtin_amdgcn_raw_buffer_store_b128(T2, r, off2, 0, 0);
    };
#pragma unroll
    for (int i = 0; i < MR_EPI_MI; ++i) {
        const int gm = wrow0 + i * 16 + li;
        const bool mok = gm < eM;
        const unsigned rowoff = (unsigned)out_row(gm) * (unsigned)e_ldc * 2u;
        bf16x4 oc[NJ], od[NJ], xs[NJ];
        if constexpr (ROT) { if (i < MR_EPI_MI - 1) rot_fetch(i + 1, rotv[(i + 1) & 1]); }
        if constexpr (HAS_X) {       // undo the 16-byte load layout
#pragma unroll
            for (int jp = 0; jp < NJ / 2; ++jp) {
                const u32x4 v4 = lx[i % LXD][jp];
                const auto s0 = __builtin_amdgcn_permlane16_swap(v4[0], v4[2], false, false);
                const auto s1 = __builtin_amdgcn_permlane16_swap(v4[1], v4[3], false, false);
                xs[2 * jp] = __builtin_bit_cast(bf16x4, u32x2{s0[0], s1[0]});
                xs[2 * jp + 1] = __builtin_bit_cast(bf16x4, u32x2{s0[1], s1[1]});
            }
            if (NJ & 1) xs[NJ - 1] = __builtin_bit_cast(bf16x4, u32x2{lx[i % LXD][NJ / 2][0], lx[i % LXD][NJ / 2][1]});
            if (i + LXD < MR_EPI_MI) lx_fetch(i + LXD, lx[i % LXD]);
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            f32x4 v = acc[i][j];
            if constexpr (ROT) v *= rotv[i & 1][j];
            bf16x4 o;
#pragma unroll
            for (int r = 0; r < 4; ++r) o[r] = (__bf16)v[r];
            od[j] = o;
            if constexpr (MODE == 2) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float sg = sigmoid1702(v[r]);
                    o[r] = (__bf16)(v[r] * sg);
                    od[j][r] = (__bf16)(sg + 1.702f * v[r] * sg * (1.0f - sg));
                }
            }
            if constexpr (HAS_X) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    o[r] = (MODE == 3) ? (__bf16)((float)o[r] + (float)xs[j][r]) : (__bf16)((float)o[r] * (float)xs[j][r]);
            }
            oc[j] = o;
            if constexpr (CS) {
                if (f_cs && mok) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) cs[j][r] += (float)o[r];
                }
            }
        }
        if constexpr (FULL_LINES) {
#pragma unroll
            for (int jq = 0; jq < NJ / 4; ++jq) {
                if constexpr (MODE == 2) store_quad(rc2, i, jq, od[4 * jq], od[4 * jq + 1], od[4 * jq + 2], od[4 * jq + 3]);
                store_quad(rc, i, jq, oc[4 * jq], oc[4 * jq + 1], oc[4 * jq + 2], oc[4 * jq + 3]);
            }
        } else {
#pragma unroll
            for (int jp = 0; jp < NJ / 2; ++jp) {
                if constexpr (MODE == 2) store_pair(rc2, rowoff, mok, jp, od[2 * jp], od[2 * jp + 1]);
                store_pair(rc, rowoff, mok, jp, oc[2 * jp], oc[2 * jp + 1]);
            }
        }
        if (NJ & 1) {                                          // BN = 192: the odd block keeps 8-byte stores
            const int col = wcol0 + (NJ - 1) * 16 + g * 4;
            const unsigned off = (mok && col < eN) ? rowoff + (unsigned)col * 2u : OOB;
            if constexpr (MODE == 2) __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, od[NJ - 1]), rc2, off, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, oc[NJ - 1]), rc, off, 0, 0);
        }
        if constexpr (CS) {
            // column sums of the stored tile per 64-row band (mr_gemm_args.colsum: partial row 4 * (m / 256) + (m % 256) / 64):
            // 4 row blocks summed in registers, the 16 rows of a block across the DPP row
            if ((i & 3) == 3 && f_cs) {
                float* const prow = e_cs + (int64_t)(wrow0 / 64 + (i >> 2)) * e_ldcs;          // (wrow0 is a multiple of 64)
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) cs[j][r] = row16_sum(cs[j][r]);
                    const int col = wcol0 + j * 16 + g * 4;
                    if (li == 0 && col < eN) *reinterpret_cast<f32x4*>(prow + col) = cs[j];
                    cs[j] = f32x4{0.f, 0.f, 0.f, 0.f};
                    // 128-row tiles: the partial rows come in fours per 256 rows (mr_gemm_colsum_rows); a last row tile without a partner
                    // writes the missing two bands as zeros (they are summed by the caller's reduction like every other partial row)
                    if (MR_EPI_MI == 4 && ((cm0 >> 7) & 1) == 0 && cm0 + 128 >= eM && li == 0 && col < eN)
                        *reinterpret_cast<f32x4*>(prow + 2 * e_ldcs + col) = f32x4{0.f, 0.f, 0.f, 0.f};
                }
            }
        }
        MR_EPI_ROW_FENCE();     // gemm4: a scheduling barrier per row block (keeps the AGPR -> VGPR copies of later blocks from being hoisted)
    }
