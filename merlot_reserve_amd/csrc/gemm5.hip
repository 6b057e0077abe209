// Fifth-generation bf16 MFMA GEMM for gfx950, "NT" operands:  C[M,N] = A[M,K] . B[N,K]^T, both K-contiguous.  Same interface, epilogue
// text (gemm3_epilogue.inc) and tile-list decode as the ping-pong (gemm3.hip) and one-wave-per-SIMD (gemm4.hip) kernels; what
// changes is who shares a CU:
//
// TWO independent workgroups per CU.  A workgroup is FOUR waves (one per SIMD) as 2 (M) x 2 (N) on a 256 x 128 tile: a wave owns
// 128 x 64 = 8 x 4 accumulators of v_mfma_f32_16x16x32_bf16 -- the ping-pong kernel's wave tile -- and at most 256 registers, so
// two workgroups are resident per CU and every SIMD hosts one wave of each.  They share nothing but the CU: each has its own
// barrier, its own 72-KiB LDS ring and its own tile list, so one workgroup's epilogue -- 8 k cycles of GELU + gelu' on the vector
// ALU, the bf16 conversions, the ~3.5 k-cycle drain of its stores (vmcnt retires in order) -- runs UNDER the other's k-loop instead
// of idling the matrix pipe of the whole CU, which is what bounds the K = 768 problems in the one-workgroup-per-CU kernels (a tile's
// fixed cost there is 6.6-9.2 us of a 23-26 us tile: DESIGN.md section 3).  Persistent workgroups with equal tile lists would run in
// lockstep (both in their k-loops, then both in their epilogues), and the phase between two residents is neutrally stable, so it is
// SET at the start: the workgroup in the second wave slot of its SIMDs sleeps for about one k-loop first (a speed knob only --
// nothing depends on which workgroups share a CU).
//
// k-loop: BK = 32 steps (64-byte LDS rows), a 3-stage ring of (256 + 128) x 32 operand images = 24 KiB per stage, filled by LDS-DMA
// three steps ahead: step t multiplies the fragments of stage t from registers (read during step t-1), reads the fragments of stage
// t+1 from LDS and requests stage t+3 into the buffer stage t was read from; it ends with
//     s_waitcnt vmcnt(6) (own pieces of stage t+2 landed: all but the 6 just requested) . lgkmcnt(0) (own reads of stage t+1 done) . s_barrier
// behind which stage t+2 is visible to every wave and stage t+1's buffer is free for the requests of step t+1: safe by construction.
// Per step and wave: 32 MFMAs, 12 ds_read_b128, 6 LDS-DMA requests (4 A + 2 B pieces of 1 KiB), each behind a pair of MFMAs in
// source order pinned by scheduling barriers (as in gemm4.hip).  The requests are unconditional (a cursor without an item requests
// from an empty descriptor: zero fill into a stage nobody reads), the cursor runs across output tiles, and so do the fragment reads.
// TM = 128 (round 4, option "gemm5" = 3 / the few-tile policy): the same kernel on 128 x 128 tiles -- four waves as 2 x 2 of 64 x 64 (4 x 4
// accumulators, 16 MFMAs per step and wave), an EIGHT-stage ring (128 KiB, one workgroup per CU) -- for problems whose 256-row tile grids
// leave most of the chip empty (M = 2308 / 3072 rows, N = 768 / 1024: the VCR ViT, the span tower): twice the tiles, half the k-loop per tile,
// at 1.33 x the operand bytes per FLOP of the 256 x 128 tile (LDS-bound: 48 KiB through the LDS per 256 MFMA cycles; 550 TF/s at best).
// Measured (gemm3_test g5time, us; ping-pong / one-barrier kernels | this geometry): 2308 x 1024 x 4096 46-52 | 35, x 3072 46 | 30, x 1024 20 | 13;
// 3072 x 768 x 3072 38-48 | 30, x 768 17.5 | 11.7.  (A three-stage ring with three workgroups per CU was 10 % slower on the long-K shapes, a
// six-stage ring on 256 x 128 tiles never faster than two workgroups per CU: both removed.)
// 64-byte rows: a 16-row fragment block is one 1-KiB LDS-DMA piece (lane l -> row l >> 2, 16-byte slot l & 3); slot = chunk ^
// ((0 - (row >> 2)) & 3) on the SOURCE address and on the ds_read_b128 address makes the reads conflict-free over the hardware's
// four 16-lane groups (checked by enumeration: every group covers 16 distinct 16-byte columns of the 256-byte bank row).
#include <stdlib.h>
#include <string.h>
#include <type_traits>
#include "gemm256_sched.h"

namespace g5 {

using namespace g256;

constexpr int BN5 = 128;
// NW = 4 waves.  (An eight-wave workgroup on 256 x 256 tiles under this k-loop -- the ping-pong kernel's geometry and operand traffic, BK = 32
// steps, no wave-group phases -- was slower than the ping-pong kernel on every shape: commit 502fd27, removed.)
// NS = ring stages.  3: a request has ONE step to land (it is waited for at the end of the step after the one that issued it) -- fine beside a
// second resident workgroup.  The 128-row geometry (one workgroup per CU: its problems have fewer tiles than the chip has CUs) requests NS = 8
// steps ahead and waits for the stage two steps ahead, leaving six steps for the L2 round trip.
template <int NW, int TM = 256, int NS = 3> struct Geo5 {
    static_assert(NW == 4 && (TM == 256 || TM == 128), "geometries");
    static constexpr int NSTG = NS;
    static constexpr int BN = 128;
    static constexpr int MI = TM / 32;                                             // 16-row blocks per wave (two wave rows)
    static constexpr int STG_A = TM * 64, STG_B = BN * 64, STG = STG_A + STG_B, LDS = NSTG * STG;
    static constexpr int PA = (TM / 16) / NW, PB = (BN / 16) / NW, ND = PA + PB;   // 1-KiB pieces per wave and step: A, B, both
    static constexpr int OCC = NS > 3 ? 1 : TM == 128 ? 3 : 2;                     // workgroups per CU
};
static_assert(Geo5<4>::LDS == 72 * 1024 && 2 * Geo5<4>::LDS <= 160 * 1024, "LDS budgets");
static_assert(Geo5<4, 128, 8>::LDS == 128 * 1024, "LDS budget of the 128 x 128 geometry");

__device__ __forceinline__ int swz5(int row) { return (0 - ((row >> 2) & 3)) & 3; }

template <int MODE, int NW, int TM = 256, int NS = 3>
__global__ __launch_bounds__(NW * 64, (Geo5<NW, TM, NS>::OCC)) void gemm5_kernel(const G256Args ga, const int stagger_mode, const int stagger_units) {
    constexpr int NJ = 4, WCOLS = 64;
    using GEO = Geo5<NW, TM, NS>;
    constexpr int NSTG = NS;
    constexpr int STG = GEO::STG, STG_A = GEO::STG_A, PA = GEO::PA, PB = GEO::PB, ND = GEO::ND, BNT = GEO::BN, MI = GEO::MI;
    // store instructions a wave issues per tile (all unconditional, see gemm3_epilogue.inc): the first step behind an epilogue may
    // leave them -- and its own 6 requests -- outstanding while it waits for the stage requested AHEAD of the epilogue
    constexpr int NST = MI * (NJ / 2) * (MODE == 2 ? 2 : 1);
    constexpr int WAIT_RING = (NSTG - 2) * ND;        // requests that may stay in flight at a step's end: the stages three and more steps ahead
    constexpr int WAIT_FIRST = WAIT_RING + NST;
    static_assert(WAIT_FIRST <= 63, "vmcnt is a 6-bit counter");
    __shared__ __attribute__((aligned(16))) char smem[GEO::LDS];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int g = lane >> 4, li = lane & 15;

    const int G = gridDim.x;
    const int xcd = blockIdx.x & 7, qd = G >> 3, rm = G & 7;
    const int bperm = (xcd < rm ? xcd * (qd + 1) : rm * (qd + 1) + (xcd - rm) * qd) + (blockIdx.x >> 3);
    int m0v, n0v;
    item_pp(ga, bperm, lane, G, BNT, m0v, n0v, TM);
    auto item_m0 = [&](int q) -> int { const int r = __builtin_amdgcn_readlane(m0v, q & 63); return q < 64 ? r : -1; };
    auto item_n0 = [&](int q) -> int { return __builtin_amdgcn_readlane(n0v, q & 63); };
    if (item_m0(0) < 0) return;
    const mr_gemm_args& p0 = ga.p[0];
    const int nks = (int)(p0.K >> 5);
    const unsigned lda2 = (unsigned)p0.lda * 2u, ldb2 = (unsigned)p0.ldb * 2u;
    const char* const Aptr = static_cast<const char*>(p0.A);
    const char* const Bptr = static_cast<const char*>(p0.B);
    const int a_extent = (int)(((p0.M - 1) * p0.lda + p0.K) * 2), b_extent = (int)(((p0.N - 1) * p0.ldb + p0.K) * 2);
    auto rel = [&](int piece, unsigned ld2) -> unsigned {      // byte offset of this lane's chunk of 1-KiB piece `piece` in an item at row 0
        const int row = piece * 16 + (lane >> 2);
        return (unsigned)row * ld2 + (unsigned)(((lane & 3) ^ swz5(row)) * 16);
    };
    // one per-lane offset per operand: a wave's pieces are 16 rows apart, a wave-uniform stride that rides in the scalar offset
    const unsigned pao = rel(wave * PA, lda2), pbo = rel(wave * PB, ldb2);
    const unsigned pstep_a = 16u * lda2, pstep_b = 16u * ldb2;
    // fragment reads: lane (g, li) of a 16-row block reads k-chunk g of row li
    const int fo = li * 64 + ((g ^ swz5(li)) << 4);
    const int fa = wr * (TM * 32) + fo, fb = STG_A + wc * 4096 + fo;

    // The phase between the two workgroups of a CU (see the header): the one whose waves sit in the odd wave slots waits ~ one k-loop.
    if (stagger_mode != 0) {
        bool late;
        if (stagger_mode == 1) late = (__builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 4) & 1) != 0;          // HW_REG_HW_ID.WAVE_ID bit 0
        else if (stagger_mode == 2) late = (int)blockIdx.x >= (G >> 1);
        else late = ((blockIdx.x >> 3) & 1) != 0;
        if (late)
            for (int n = 0; n < stagger_units; ++n) __builtin_amdgcn_s_sleep(32);        // 2048 cycles each
    }

    // ---- ONE issue cursor for both operands, three steps ahead of the compute cursor, across item boundaries ----
    int ik = 0, qi = 0, ist = 0;
    __amdgpu_buffer_rsrc_t ra_c, rb_c;
    auto set_item = [&](int q_) {
        const int mi = item_m0(q_), ni = item_n0(q_);
        const int aoff = (mi >= 0 ? mi : 0) * (int)lda2, boff = (mi >= 0 ? ni : 0) * (int)ldb2;
        ra_c = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(Aptr) + aoff, 0, mi >= 0 ? a_extent - aoff : 0, 0x00020000);
        rb_c = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(Bptr) + boff, 0, mi >= 0 ? b_extent - boff : 0, 0x00020000);
    };
    set_item(0);
#define G5_ISSUE_ALL()                                                                                                  \
    do {                                                                                                                \
        char* st_ = smem + ist * STG;                                                                                   \
        const unsigned so_ = (unsigned)ik * 64u;                                                                        \
        _Pragma("unroll") for (int j_ = 0; j_ < PA; ++j_) MR_DMA(ra_c, MR_LDS_PTR(void, st_ + wave * (PA * 1024) + j_ * 1024), 16, pao, so_ + j_ * pstep_a, 0, 0); \
        _Pragma("unroll") for (int j_ = 0; j_ < PB; ++j_) MR_DMA(rb_c, MR_LDS_PTR(void, st_ + STG_A + wave * (PB * 1024) + j_ * 1024), 16, pbo, so_ + j_ * pstep_b, 0, 0); \
    } while (0)
#define G5_ADVANCE()                                                                                                    \
    do {                                                                                                                \
        ist = (ist == NSTG - 1) ? 0 : ist + 1;                                                                          \
        if (++ik == nks) {                                                                                              \
            ik = 0;                                                                                                     \
            set_item(++qi);                                                                                             \
        }                                                                                                               \
    } while (0)
#define G5_SB() __builtin_amdgcn_sched_barrier(0)
    int qc = 0, rs = 0;                 // rs: the stage the NEXT fragments are read from
    int cm0 = item_m0(0), cn0 = item_n0(0);
    bool have_stores = false;
    constexpr bool BIAS = MODE <= 2;
    f32x4 binit[NJ];
    auto fetch_bias = [&](int n0_) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) binit[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        if constexpr (BIAS) {
            const __bf16* const bp = static_cast<const __bf16*>(p0.bias);
            if (bp != nullptr) {
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    const int gn = n0_ + wc * WCOLS + j * 16 + g * 4;
                    if (gn < (int)p0.N) {
                        const bf16x4 b4 = *reinterpret_cast<const bf16x4*>(bp + gn);
#pragma unroll
                        for (int r = 0; r < 4; ++r) binit[j][r] = (float)b4[r];
                    }
                }
            }
        }
    };
    fetch_bias(cn0);

    // prologue: the first NSTG stages requested; stage 0 has landed when only the later ones are in flight
#pragma unroll
    for (int s_ = 0; s_ < NSTG; ++s_) { G5_ISSUE_ALL(); G5_ADVANCE(); }
    wait_vmcnt<(NSTG - 1) * ND>();
    G5_SB();
    __builtin_amdgcn_s_barrier();
    G5_SB();
    // Fragment registers: the B fragments and the last two A row blocks are double buffered (parity = step & 1: K % 64 == 0, so a
    // tile's first step has parity 0); A row blocks 0-5 are replaced IN PLACE behind their own MFMAs (72 registers instead of 96:
    // beside the 128 accumulators the rotary / GELU / column-sum epilogues spill with 96).  The in-place read of row block 5 is the
    // step's last: it has the 8 MFMAs of row blocks 6 and 7 to land before the step's closing wait.
    // (TM = 128: four row blocks -- 0, 1 in place, 2, 3 double buffered; "a67" = the last two row blocks of either geometry)
    constexpr int MIP = MI - 2;                       // row blocks replaced in place
    bf16x8 a[MIP], a67[2][2], b[NJ][2];
    auto read_frags0 = [&](const char* st) {          // all fragments of a stage into parity 0 (prologue, tile switch)
#pragma unroll
        for (int j = 0; j < NJ; ++j) b[j][0] = *reinterpret_cast<const bf16x8*>(st + fb + j * 1024);
#pragma unroll
        for (int i = 0; i < MIP; ++i) a[i] = *reinterpret_cast<const bf16x8*>(st + fa + i * 1024);
        a67[0][0] = *reinterpret_cast<const bf16x8*>(st + fa + MIP * 1024);
        a67[1][0] = *reinterpret_cast<const bf16x8*>(st + fa + (MIP + 1) * 1024);
    };
    read_frags0(smem);
    wait_vmcnt<WAIT_RING>();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    G5_SB();
    __builtin_amdgcn_s_barrier();
    G5_SB();
    rs = 1;

    while (cm0 >= 0) {
        // accumulators TRANSPOSED (mfma(B-frag, A-frag)): the lane holds C[m = .. + li][n = .. + 4 g + r]; bias modes start from the bias
        f32x4 acc[MI][NJ];
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j) acc[i][j] = binit[j];

        // one k-step: multiply the fragments of parity CUR, read the next step's into parity 1 - CUR, request three steps ahead
        auto step = [&](auto cur_c, auto first_c, auto last_c) {
            constexpr int CUR = decltype(cur_c)::value, NXT = 1 - CUR;
            constexpr bool FIRST = decltype(first_c)::value;        // the tile's first step: the previous tile's stores may be in flight
            constexpr bool LAST = decltype(last_c)::value;          // the tile's last step reads no fragments: the next tile's first ones are read behind the epilogue (registers)
            const char* const rd = smem + rs * STG;
            char* const st_ = smem + ist * STG;
            const unsigned so_ = (unsigned)ik * 64u;
#pragma unroll
            for (int r = 0; r < MI; ++r) {
                const bf16x8 ar = r < MIP ? a[r < MIP ? r : 0] : a67[r - MIP < 0 ? 0 : r - MIP][CUR];
                acc[r][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[0][CUR], ar, acc[r][0], 0, 0, 0);
                acc[r][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[1][CUR], ar, acc[r][1], 0, 0, 0);
                G5_SB();
                if constexpr (!LAST) {               // the double-buffered fragments first: b0..b3, then (eight row blocks) row blocks 6, 7
                    if (r < 4) b[r][NXT] = *reinterpret_cast<const bf16x8*>(rd + fb + r * 1024);
                    else if (r < 6) a67[r - 4][NXT] = *reinterpret_cast<const bf16x8*>(rd + fa + (r + 2) * 1024);
                }
                if (r < PA) MR_DMA(ra_c, MR_LDS_PTR(void, st_ + wave * (PA * 1024) + r * 1024), 16, pao, so_ + r * pstep_a, 0, 0);
                else if (r < ND) MR_DMA(rb_c, MR_LDS_PTR(void, st_ + STG_A + wave * (PB * 1024) + (r - PA) * 1024), 16, pbo, so_ + (r - PA) * pstep_b, 0, 0);
                G5_SB();
                acc[r][2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[2][CUR], ar, acc[r][2], 0, 0, 0);
                acc[r][3] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[3][CUR], ar, acc[r][3], 0, 0, 0);
                G5_SB();
                if constexpr (!LAST) {
                    if (r < MIP) a[r < MIP ? r : 0] = *reinterpret_cast<const bf16x8*>(rd + fa + r * 1024);       // in place: this row block's MFMAs are issued
                    else if (MI == 4) a67[(r - MIP) & 1][NXT] = *reinterpret_cast<const bf16x8*>(rd + fa + r * 1024);   // four row blocks: the double-buffered pair rides in these slots
                }
                G5_SB();
            }
            if (FIRST && have_stores) wait_vmcnt<WAIT_FIRST>();
            else wait_vmcnt<WAIT_RING>();
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            G5_SB();
            __builtin_amdgcn_s_barrier();
            G5_SB();
            if constexpr (!LAST) rs = (rs == NSTG - 1) ? 0 : rs + 1;
            G5_ADVANCE();
        };
        step(std::integral_constant<int, 0>{}, std::true_type{}, std::false_type{});
        for (int t = 1; t + 2 < nks; t += 2) {
            step(std::integral_constant<int, 1>{}, std::false_type{}, std::false_type{});
            step(std::integral_constant<int, 0>{}, std::false_type{}, std::false_type{});
        }
        step(std::integral_constant<int, 1>{}, std::false_type{}, std::true_type{});          // (K % 64 == 0: an even number of steps >= 4)

        // ---------------- epilogue (bf16 output; registers + ordinary loads, no LDS) ----------------
        {
            const int wrow0 = cm0 + wr * (TM / 2), wcol0 = cn0 + wc * WCOLS;
            constexpr int MR_EPI_MI = MI;
#define MR_EPI_ROW_FENCE() do {} while (0)
#define MR_EPI_FULL_LINES 0      // (full-line stores: the trade of halves costs this kernel spilled registers at its allocation limit; gemm3.hip only)
#include "gemm3_epilogue.inc"
#undef MR_EPI_FULL_LINES
#undef MR_EPI_ROW_FENCE
            have_stores = true;
        }
        ++qc;
        cm0 = item_m0(qc);
        cn0 = item_n0(qc);
        // the next tile's first fragments (stage `rs`: landed and visible since the barrier of the last step but one); the barrier keeps
        // the requests of the next step, which refill this stage's buffer, behind every wave's reads
        if (cm0 >= 0) {
            read_frags0(smem + rs * STG);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            G5_SB();
            __builtin_amdgcn_s_barrier();
            G5_SB();
            rs = (rs == NSTG - 1) ? 0 : rs + 1;
        }
    }
    // the ring's last requests (zero fill) and the stores retire before the LDS is released
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
}

}  // namespace g5


void mr_gemm5_launch(const g256::G256Args& ga, bool r128, int mode, int st_mode, int st_units, int64_t grid_size, hipStream_t s) {
    dim3 grid((unsigned)grid_size), block(256);
#define G5_LAUNCH(MODE)                                                                                       \
    do {                                                                                                      \
        if (r128) hipLaunchKernelGGL((g5::gemm5_kernel<MODE, 4, 128, 8>), grid, block, 0, s, ga, st_mode, st_units); \
        else hipLaunchKernelGGL((g5::gemm5_kernel<MODE, 4>), grid, block, 0, s, ga, st_mode, st_units);       \
    } while (0)
    switch (mode) {
        case 0: G5_LAUNCH(0); break;
        case 1: G5_LAUNCH(1); break;
        case 2: G5_LAUNCH(2); break;
        case 3: G5_LAUNCH(3); break;
        case 4: G5_LAUNCH(4); break;
        default: G5_LAUNCH(5); break;
    }
#undef G5_LAUNCH
}
