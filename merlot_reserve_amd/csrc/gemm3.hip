// Third-generation bf16 MFMA GEMM for gfx950, "NT" operands only:  C[M,N] = A[M,K] . B[N,K]^T, both K-contiguous
// (activations x dgrad weights as flax stores them; forward weights through their transposed bf16 working copy).
//
// 256 x {256,192} x 64 tiles, 8 waves as 2 (M) x 4 (N): a wave owns 128 x {64,48} of the tile = 8 x {4,3} accumulators of
// v_mfma_f32_16x16x32_bf16, computed per k-tile in FOUR quadrants of 64 x {32,32|16} (16 | 8 MFMAs each).
//
// Two wave groups, PING-PONG.  Waves 0-3 and 4-7 are the two waves of each SIMD.  Every quadrant is a phase
//     [ LDS fragment reads of the phase | LDS-DMA issue ]  s_barrier  [ MFMAs ]  s_barrier
// and group 1 runs one barrier behind group 0, so that between any two barriers one wave of a SIMD issues MFMAs while its
// partner issues LDS reads and DMA: the matrix pipe never waits for fragment reads of its own wave, which is what bounds
// the one-barrier-per-k-tile kernel of gemm256.hip (k-loop decomposition).
//
// Schedules (template parameter PH, chosen per problem by mr_gemm3_launch):
// PH = 1, the default: ONE phase per k-tile and wave.  Memory section: B (8 | 6 ds_read_b128) + A0 (8) + 8 | 6 DMA pieces; MFMA
// section: A0 x B row block by row block, each block's A1 fragments requested into the registers its last A0 MFMA has just read
// (fragment registers stay at 64), then A1 x B: 64 | 48 MFMAs between two barriers.  The groups split the operands: group 0 issues
// every B piece (k-tile t+1, waited for at the END of its MFMA section: both groups read it after the closing barrier), group 1
// every A piece (k-tile t+2, counted wait in its next memory section).
// PH = 2: per k-tile and wave TWO phases: phase 0 reads B (8 | 6 ds_read_b128) + A0 (8) and multiplies A0 x B (32 | 24 MFMAs),
// phase 1 reads A1 (8) and multiplies A1 x B; A0 / A1 = the wave's two 64-row halves.
// Operand rings, filled by LDS-DMA (buffer_load ... lds, 1 KiB per wave instruction, zero fill beyond the extents):
//     A: 3 stages x 32 KiB, two k-tiles ahead (issued in phase 0);
//     B: 2 stages x {32,24} KiB: k-tile t+2 overwrites k-tile t's stage in phase 1, after the B reads of k-tile t
//        (phase 0) have been retired by a counted lgkmcnt AHEAD of that phase's barrier.  Every LDS read that a later
//        DMA overwrites is retired ahead of a barrier the issuing wave passes before it issues: safe by construction.
//   = 160 KiB (BN = 256) | 144 KiB (BN = 192).  One counted s_waitcnt vmcnt per k-tile (never 0 inside a tile's loop), in
// phase 3 ahead of the barrier that precedes the first read of k-tile t+1.  The issue cursors run across output tiles
// (persistent workgroups), so a tile's first two k-tiles land under the previous tile's epilogue.
// The swizzle (chunk ^= (row >> 1) & 7) lives on the DMA's per-lane SOURCE address and is undone by the fragment reads.
#include <stdlib.h>
#include <string.h>
#include <type_traits>
#include "gemm256_sched.h"

namespace g3 {

using namespace g256;

template <int BN> struct Geo3 {
    static_assert(BN == 256 || BN == 192, "tile widths of the ping-pong kernel");
    static constexpr int WCOLS = BN / 4, NJ = WCOLS / 16, JB0 = 2, JB1 = NJ - 2;
    static constexpr int STAGE_A = 256 * 128, NSTAGE_A = 3;
    static constexpr int STAGE_B = BN * 128, NSTAGE_B = 2;
    static constexpr int OFF_B = NSTAGE_A * STAGE_A;
    static constexpr int LDS_BYTES = OFF_B + NSTAGE_B * STAGE_B;
    static constexpr int NBP_HI = (BN == 256) ? 2 : 1;      // B pieces per wave for rows 128.. of the B tile
    static constexpr int WAITN = 4 + 2 + NBP_HI;            // DMA pieces a wave issues per k-tile
};
static_assert(Geo3<256>::LDS_BYTES == 160 * 1024 && Geo3<192>::LDS_BYTES == 144 * 1024, "LDS budget");


// MODE (the epilogue, fixed per launch: one problem per launch):
//   0: bias | 1: bias + "rotary" scales | 2: bias + GELU, gelu' copy to c2 | 3: + residual | 4: x aux (+ column sums)
// PH = phases per k-tile.  2: [B + A0 reads | 4 A pieces] [32 MFMAs] / [A1 reads | 4 B pieces] [32 MFMAs], both groups issue both operands.
// 1: ONE phase of 64 | 48 MFMAs -- half the barriers per MFMA: the memory section reads B + A0 and issues 8 pieces, the A1 fragments
// replace the A0 fragments in place INSIDE the MFMA section (two ds_read_b128 behind each row block's last A0 MFMA, 24+ MFMAs ahead
// of their use), and the groups split the operands: group 0 issues every B piece (one k-tile ahead), group 1 every A piece (two ahead).
template <int BN, int MODE, int PH>
__global__ __launch_bounds__(512, 2) void gemm3_kernel(const G256Args ga) {
    using GEO = Geo3<BN>;
    constexpr int WCOLS = GEO::WCOLS, NJ = GEO::NJ, JB1 = GEO::JB1;
    constexpr int STAGE_A = GEO::STAGE_A, STAGE_B = GEO::STAGE_B, OFF_B = GEO::OFF_B;
    constexpr int NSTAGE_A = GEO::NSTAGE_A, NSTAGE_B = GEO::NSTAGE_B, NBP_HI = GEO::NBP_HI, WAITN = GEO::WAITN;
    // store instructions a wave issues per tile, ALL unconditional (masked lanes store to an out-of-range buffer offset, which the
    // hardware drops): vmcnt retires in order, so the first k-tile behind an epilogue may leave exactly these -- and its own DMA
    // pieces -- in flight while waiting for the k-tile issued AHEAD of the epilogue; the stores then drain under two k-tiles of
    // MFMAs instead of stalling the wave at its first counted wait.  (The column-sum stores of MODE 4 are not counted: fewer
    // outstanding operations than allowed only makes the wait conservative.)
    constexpr int NST = 8 * (NJ / 2 + (NJ & 1)) * (MODE == 2 ? 2 : 1);
    static_assert(WAITN + NST <= 63, "vmcnt is a 6-bit counter");
    __shared__ __attribute__((aligned(16))) char smem[GEO::LDS_BYTES];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 2, wc = wave & 3;             // wr = the wave GROUP (and the tile's row half), wc = column quarter
    const int g = lane >> 4, li = lane & 15;

    const int G = gridDim.x;
    const int xcd = blockIdx.x & 7, qd = G >> 3, rm = G & 7;
    const int bperm = (xcd < rm ? xcd * (qd + 1) : rm * (qd + 1) + (xcd - rm) * qd) + (blockIdx.x >> 3);
    // The workgroup's items (output tiles), decoded ONCE: lane q holds item q (m0 < 0 = none), fetched with v_readlane.  Decoding
    // an item at every cursor switch -- integer divisions and kernel-argument loads inside a phase that all eight waves wait
    // for -- cost ~4 000 cycles per tile (in-kernel stamps).  <= 64 items per workgroup (host check).
    int m0v, n0v;
    item_pp(ga, bperm, lane, G, BN, m0v, n0v);
    auto item_m0 = [&](int q) -> int { return q < 64 ? __builtin_amdgcn_readlane(m0v, q) : -1; };
    auto item_n0 = [&](int q) -> int { return __builtin_amdgcn_readlane(n0v, q & 63); };
    if (item_m0(0) < 0) return;
    const mr_gemm_args& p0 = ga.p[0];
    const int nkt = (int)(p0.K >> 6);
    const unsigned lda2 = (unsigned)p0.lda * 2u, ldb2 = (unsigned)p0.ldb * 2u;
    // operand descriptors: rows >= M (A) / >= N (B) lie beyond num_records and read as zeros -- the per-lane offsets carry the
    // item's first row, so no predicate per piece: offset(item) = offset(row 0 item) + m0 * lda2
    const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p0.A), 0, (int)(((p0.M - 1) * p0.lda + p0.K) * 2), 0x00020000);
    const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p0.B), 0, (int)(((p0.N - 1) * p0.ldb + p0.K) * 2), 0x00020000);
    auto rel = [&](int piece, unsigned ld2) -> unsigned {      // byte offset of this lane's chunk of 1-KiB piece `piece` in an item at row 0
        const int row = piece * 8 + (lane >> 3);
        return (unsigned)row * ld2 + (unsigned)(((lane & 7) ^ swz_kc(row)) * 16);
    };
    const unsigned ar0 = rel(wave * 2, lda2), ar1 = rel(wave * 2 + 1, lda2), ar2 = rel(16 + wave * 2, lda2), ar3 = rel(16 + wave * 2 + 1, lda2);
    const unsigned br0 = rel(wave * 2, ldb2), br1 = rel(wave * 2 + 1, ldb2);
    const unsigned br2 = rel(NBP_HI == 2 ? 16 + wave * 2 : 16 + wave, ldb2), br3 = rel(16 + wave * 2 + 1, ldb2);

    // PH == 1: the wave's 8 (6: B of a 192-wide tile) pieces of ITS operand -- group 0: B, group 1: A
    constexpr int PB1 = (BN == 256) ? 8 : 6;
    unsigned po[8];
    if constexpr (PH == 1) {
#pragma unroll
        for (int j = 0; j < 8; ++j) po[j] = (wr == 0) ? rel((wave & 3) * PB1 + (j < PB1 ? j : 0), ldb2) : rel((wave & 3) * 8 + j, lda2);
    }
    // ---- issue cursors (one per operand), two k-tiles ahead of the compute cursor, across item boundaries ----
    int qa = 0, ika = 0, ista = 0, qb = 0, ikb = 0, istb = 0;
    bool va = true, vb = true, issued = false;
    unsigned abase = (unsigned)item_m0(0) * lda2, bbase = (unsigned)item_n0(0) * ldb2;
    // the issue slots of a k-tile: A rows 0-127, A rows 128-255 (+ advance), B rows 0-127, B rows 128.. (+ advance)
#define G3_ISSUE_A_PIECE(ar_, off_)                                                                                     \
    do {                                                                                                                \
        if (va) MR_DMA(ra, MR_LDS_PTR(void, smem + ista * STAGE_A + (off_) + wave * 2048), 16, abase + (ar_), (unsigned)ika * 128u, 0, 0); \
    } while (0)
#define G3_ADVANCE_A()                                                                                                  \
    do {                                                                                                                \
        if (va) {                                                                                                       \
            ista = (ista == NSTAGE_A - 1) ? 0 : ista + 1;                                                               \
            if (++ika == nkt) {                                                                                         \
                ika = 0;                                                                                                \
                const int m_ = item_m0(++qa);                                                                           \
                va = m_ >= 0;                                                                                           \
                abase = (unsigned)m_ * lda2;                                                                            \
            }                                                                                                           \
        }                                                                                                               \
    } while (0)
    // the wave's four A pieces of a k-tile (rows 0-127: two, rows 128-255: two)
#define G3_ISSUE_A_LO()                                                                                                 \
    do {                                                                                                                \
        issued = va;                                                                                                    \
        G3_ISSUE_A_PIECE(ar0, 0);                                                                                       \
        G3_ISSUE_A_PIECE(ar1, 1024);                                                                                    \
    } while (0)
#define G3_ISSUE_A_HI()                                                                                                 \
    do {                                                                                                                \
        G3_ISSUE_A_PIECE(ar2, 16384);                                                                                   \
        G3_ISSUE_A_PIECE(ar3, 16384 + 1024);                                                                            \
        G3_ADVANCE_A();                                                                                                 \
    } while (0)
#define G3_ISSUE_B_LO()                                                                                                 \
    do {                                                                                                                \
        if (vb) {                                                                                                       \
            char* sb_ = smem + OFF_B + istb * STAGE_B + wave * 2048;                                                    \
            const unsigned sb = (unsigned)ikb * 128u;                                                                   \
            MR_DMA(rb, MR_LDS_PTR(void, sb_), 16, bbase + br0, sb, 0, 0);                                               \
            MR_DMA(rb, MR_LDS_PTR(void, sb_ + 1024), 16, bbase + br1, sb, 0, 0);                                        \
        }                                                                                                               \
    } while (0)
#define G3_ISSUE_B_HI()                                                                                                 \
    do {                                                                                                                \
        if (vb) {                                                                                                       \
            char* sb_ = smem + OFF_B + istb * STAGE_B + 16384 + wave * (NBP_HI * 1024);                                 \
            const unsigned sb = (unsigned)ikb * 128u;                                                                   \
            MR_DMA(rb, MR_LDS_PTR(void, sb_), 16, bbase + br2, sb, 0, 0);                                               \
            if (NBP_HI == 2) MR_DMA(rb, MR_LDS_PTR(void, sb_ + 1024), 16, bbase + br3, sb, 0, 0);                       \
            istb = (istb == NSTAGE_B - 1) ? 0 : istb + 1;                                                               \
            if (++ikb == nkt) {                                                                                         \
                ikb = 0;                                                                                                \
                vb = item_m0(++qb) >= 0;                                                                                \
                bbase = (unsigned)item_n0(qb) * ldb2;                                                                   \
            }                                                                                                           \
        }                                                                                                               \
    } while (0)
#define G3_RING_WAIT()                                                                                                  \
    do {                                                                                                                \
        if (issued) wait_vmcnt<WAITN>();                                                                                \
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                                           \
    } while (0)
#define G3_BARRIER()                                                                                                    \
    do {                                                                                                                \
        __builtin_amdgcn_sched_barrier(0);                                                                              \
        __builtin_amdgcn_s_barrier();                                                                                   \
        __builtin_amdgcn_sched_barrier(0);                                                                              \
    } while (0)
#define G3_LGKM(n)                                                                                                      \
    do {                                                                                                                \
        asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(n) : "memory");                                                      \
        __builtin_amdgcn_sched_barrier(0);                                                                              \
    } while (0)

    // PH == 1: all 8 A pieces of the A cursor's k-tile (group 1) / all PB1 B pieces of the B cursor's k-tile (group 0)
#define G3_ISSUE_A8()                                                                                                   \
    do {                                                                                                                \
        issued = va;                                                                                                    \
        if (va) {                                                                                                       \
            char* st_ = smem + ista * STAGE_A + (wave & 3) * 8192;                                                      \
            const unsigned sa = (unsigned)ika * 128u;                                                                   \
            _Pragma("unroll") for (int j_ = 0; j_ < 8; ++j_) MR_DMA(ra, MR_LDS_PTR(void, st_ + j_ * 1024), 16, abase + po[j_], sa, 0, 0); \
        }                                                                                                               \
        G3_ADVANCE_A();                                                                                                 \
    } while (0)
#define G3_ISSUE_B8()                                                                                                   \
    do {                                                                                                                \
        issued = vb;                                                                                                    \
        if (vb) {                                                                                                       \
            char* sb_ = smem + OFF_B + istb * STAGE_B + (wave & 3) * (PB1 * 1024);                                      \
            const unsigned sb = (unsigned)ikb * 128u;                                                                   \
            _Pragma("unroll") for (int j_ = 0; j_ < PB1; ++j_) MR_DMA(rb, MR_LDS_PTR(void, sb_ + j_ * 1024), 16, bbase + po[j_], sb, 0, 0); \
            istb = (istb == NSTAGE_B - 1) ? 0 : istb + 1;                                                               \
            if (++ikb == nkt) {                                                                                         \
                ikb = 0;                                                                                                \
                vb = item_m0(++qb) >= 0;                                                                                \
                bbase = (unsigned)item_n0(qb) * ldb2;                                                                   \
            }                                                                                                           \
        }                                                                                                               \
    } while (0)
    if constexpr (PH == 1) {
        // prologue: group 1 issues A of k-tiles 0 and 1 (k-tile 0 landed when only the second one's pieces are in flight), group 0 B of k-tile 0
        if (wr == 1) { G3_ISSUE_A8(); G3_ISSUE_A8(); if (issued) wait_vmcnt<8>(); else asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
        else { G3_ISSUE_B8(); asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
    } else {
    // prologue: k-tiles 0 and 1 of the sequence; k-tile 0 has landed when all but the second one's pieces have
    G3_ISSUE_A_LO(); G3_ISSUE_A_HI(); G3_ISSUE_B_LO(); G3_ISSUE_B_HI();
    G3_ISSUE_A_LO(); G3_ISSUE_A_HI(); G3_ISSUE_B_LO(); G3_ISSUE_B_HI();
    G3_RING_WAIT();
    }
    G3_BARRIER();
    if (wr == 1) G3_BARRIER();          // group 1 runs one barrier behind group 0 from here on

    int qc = 0, csa = 0, csb = 0;
    int cm0 = item_m0(0), cn0 = item_n0(0);
    bool have_stores = false;          // an epilogue's stores may be in flight (never before the workgroup's first tile)
    // The bias is the accumulators' INITIAL value (no add per element in the epilogue).  A tile's bias is fetched and widened in
    // the PREVIOUS tile's epilogue, ahead of its stores (a load consumed behind them would wait for them: vmcnt retires in order).
    constexpr bool BIAS = MODE <= 2;             // residual / aux problems carry no bias (host check)
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
    while (cm0 >= 0) {
        // accumulators TRANSPOSED (mfma(B-frag, A-frag)): the lane holds C[m = .. + li][n = .. + 4 g + r]
        f32x4 acc[8][NJ];
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j) acc[i][j] = binit[j];

        auto ktile = [&](auto first_c) {
            constexpr bool FIRST = decltype(first_c)::value;       // the tile's first k-tile: the previous tile's stores are in flight
            const char* As = smem + csa * STAGE_A;
            const char* Bs = smem + OFF_B + csb * STAGE_B;
            bf16x8 a[4][2], b[NJ][2];
            auto read_b = [&](int j0, int j1) {
#pragma unroll
                for (int j = j0; j < j1; ++j)
#pragma unroll
                    for (int kk = 0; kk < 2; ++kk) b[j][kk] = frag<false, 256, 64>(Bs, wc * WCOLS + j * 16, kk, lane);
            };
            auto read_a = [&](int half) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int kk = 0; kk < 2; ++kk) a[i][kk] = frag<false, 256, 64>(As, wr * 128 + half * 64 + i * 16, kk, lane);
            };
            auto mfmas = [&](int half, int j0, int j1) {
                __builtin_amdgcn_s_setprio(1);
#pragma unroll
                for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int j = j0; j < j1; ++j)
                            acc[half * 4 + i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[j][kk], a[i][kk], acc[half * 4 + i][j], 0, 0, 0);
                __builtin_amdgcn_s_setprio(0);
            };
            auto tile_wait = [&]() {        // k-tile t+1 has landed behind the next barrier
                if (FIRST && issued && have_stores) wait_vmcnt<WAITN + NST>();
                else G3_RING_WAIT();
            };
            if constexpr (PH == 1) {
                // ---------------- memory section: B + A0 fragments, this group's 8 pieces ----------------
                read_b(0, NJ);
                __builtin_amdgcn_sched_barrier(0);      // B before A: the counted wait below relies on the issue order
                read_a(0);
                __builtin_amdgcn_sched_barrier(0);
                if (wr == 0) {
                    G3_ISSUE_B8();                       // k-tile t+1 into the stage k-tile t-1 was read from (its reads were retired ahead of a barrier)
                    G3_LGKM(8);
                } else {
                    G3_ISSUE_A8();                       // k-tile t+2
                    G3_LGKM(8);
                    // A of k-tile t+1 (issued one k-tile ago) has landed behind the coming barrier: group 0 reads it right after it
                    if (FIRST && issued && have_stores) wait_vmcnt<8 + NST>();
                    else if (issued) wait_vmcnt<8>();
                    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                }
                G3_BARRIER();
                G3_LGKM(0);
                // ---------------- MFMA section: A0 x B row block by row block, each block's A1 fragments requested into the registers
                // its last A0 MFMA has just read; then A1 x B ----------------
                __builtin_amdgcn_s_setprio(1);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
#pragma unroll
                    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                        for (int j = 0; j < NJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[j][kk], a[i][kk], acc[i][j], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int kk = 0; kk < 2; ++kk) a[i][kk] = frag<false, 256, 64>(As, wr * 128 + 64 + i * 16, kk, lane);
                    __builtin_amdgcn_sched_barrier(0);
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
#pragma unroll
                    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                        for (int j = 0; j < NJ; ++j) acc[4 + i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[j][kk], a[i][kk], acc[4 + i][j], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
                __builtin_amdgcn_s_setprio(0);
                if (wr == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // B of k-tile t+1 has landed behind the closing barrier
                G3_BARRIER();
            } else {
                // ---------------- phase 0: A0 x B.  The B reads are retired AHEAD of the barrier (phase 1 restages B) ----------------
                read_b(0, NJ);
                __builtin_amdgcn_sched_barrier(0);      // B before A: the counted wait below relies on the issue order
                read_a(0);
                __builtin_amdgcn_sched_barrier(0);
                G3_ISSUE_A_LO();
                G3_ISSUE_A_HI();
                G3_LGKM(8);
                G3_BARRIER();
                G3_LGKM(0);
                mfmas(0, 0, NJ);
                G3_BARRIER();
                // ---------------- phase 1: A1 x B.  The A reads are retired ahead of the barrier (the next phase 0 restages A) ----------------
                read_a(1);
                __builtin_amdgcn_sched_barrier(0);
                G3_ISSUE_B_LO();
                G3_ISSUE_B_HI();
                G3_LGKM(0);
                tile_wait();
                G3_BARRIER();
                mfmas(1, 0, NJ);
                G3_BARRIER();
            }
            csa = (csa == NSTAGE_A - 1) ? 0 : csa + 1;
            csb = (csb == NSTAGE_B - 1) ? 0 : csb + 1;
        };
        ktile(std::integral_constant<bool, true>{});
        for (int t = 1; t < nkt; ++t) ktile(std::integral_constant<bool, false>{});

        // ---------------- epilogue (bf16 output; registers + ordinary loads, no LDS) ----------------
        // The two groups' epilogues run side by side (group 0 waits for group 1's last MFMAs, group 1 waits behind its epilogue
        // for group 0's, which restores the one-barrier offset).
        if (wr == 0) G3_BARRIER();
        {
            const int wrow0 = cm0 + wr * 128, wcol0 = cn0 + wc * WCOLS;
            constexpr int MR_EPI_MI = 8;
#define MR_EPI_ROW_FENCE() do {} while (0)
#include "gemm3_epilogue.inc"
#undef MR_EPI_ROW_FENCE
            have_stores = true;
        }
        if (wr == 1) G3_BARRIER();
        ++qc;
        cm0 = item_m0(qc);
        cn0 = item_n0(qc);
    }
    if (wr == 0) G3_BARRIER();          // pairs with group 1's last barrier
}


// ---------------------------------------------------------------------------------------------------------------------------
// "TN" variant for the weight gradients:  C[M,N] = A^T . B with A stored [K, M] and B stored [K, N] (activations x upstream
// gradients, the contraction index = tokens is the ROW index of both).  Same two-group ping-pong k-loop; the operand tiles are
// [64 k][256] images read with ds_read_b64_tr_b16 (two per MFMA operand).  One 256 x 256 output tile per workgroup, no
// persistence (K = tokens is long: 93-241 k-tiles, the prologue and the plain bf16 epilogue are < 2 % of a tile), up to 20
// problems per launch: the weight gradients of TWO transformer layers fill the chip without split-K (216 tiles for the base
// model) where one layer's four are 108; FOUR layers of the large model are 768 tiles = three full rounds where one layer's 192
// leave a quarter of the CUs idle.  (TNArgs: gemm_plan.h)
//
// The k-tile's schedule (profiles/tn_kloop_before.txt, profiles/tn_kloop.txt).  A wave needs 48 ds_read_b64_tr_b16 and issues
// 8 DMA pieces per k-tile, and in-kernel stamps showed its two memory sections (32 reads + 4 pieces, 16 reads + 4 pieces, each drained with
// lgkmcnt(0)) at 870-960 and 670-680 clocks beside the partner group's 512-clock MFMA blocks: the sections, not the matrix pipe, set the k-tile.
// So the sections carry only what nothing else can:
//     phase 0 memory  B (16 reads) + the kk = 0 halves of A0 (8)  | A pieces 0-1 of k-tile t+2 | lgkmcnt(8): the B reads are back   s_barrier
//     phase 0 MFMA    the kk = 1 halves of A0 (8 reads) | 16 MFMAs kk = 0 | A1 kk = 0 in place (8) | 16 MFMAs kk = 1 | A1 kk = 1 in place (8)  s_barrier
//     phase 1 memory  A pieces 2-3 and the four B pieces of k-tile t+2 | lgkmcnt(0) | the counted vmcnt: k-tile t+1 has landed           s_barrier
//     phase 1 MFMA    32 MFMAs A1 x B                                                                                                   s_barrier
// 24 of the 48 reads land under the wave's own MFMAs behind counted waits (LDS data returns in issue order).  Every accumulator still receives
// kk = 0 before kk = 1 of every k-tile, so the outputs are those of the two-drain schedule bit for bit.
// Ring safety, by construction as before: every LDS read that a later DMA overwrites is retired ahead of a barrier its wave passes before any wave
// issues that DMA.  B (2 stages: k-tile t+2 overwrites k-tile t in phase 1): all B reads sit in phase 0's memory section and are retired by its
// lgkmcnt(8) ahead of the barrier (the B reads are issued first; 8 later reads may be outstanding).  A (3 stages: k-tile t+3 overwrites k-tile t in
// the phase 0 / phase 1 memory sections of k-tile t+1): the last reads of k-tile t, A1 in phase 0's MFMA section, are retired by phase 1's lgkmcnt(0)
// ahead of its barrier -- the barrier behind which the OTHER group enters its next phase 0.

// -DMR_TN_STAMPS: a DIAGNOSTIC build (scripts/tn_kloop_stamps.py).  Every wave reads the shader clock at the section boundaries of a k-tile and adds
// the differences into scalar sums; lane 0 of wave 0 (group 0) and of wave 4 (group 1) of the first 256 workgroups store them behind the k-loop into a
// buffer of their own, which the launcher prints.  The stamp's lgkmcnt(0) drains the fragment reads a section leaves in flight: read the SHARES of such
// a build, never its run time.  Segments: 0 memory section 0 | 1 barrier | 2 MFMA block 0 | 3 barrier | 4 memory section 1 | 5 ring wait | 6 barrier |
// 7 MFMA block 1 | 8 barrier.
#ifdef MR_TN_STAMPS
#include <stdio.h>
constexpr int TN_NSEG = 9;
__device__ unsigned long long tn_stamp_sums[256][2][TN_NSEG];
#define TN_STAMP_NOW(v_)                                                                                                \
    do {                                                                                                                \
        __builtin_amdgcn_sched_barrier(0);                                                                              \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v_)::"memory");                                      \
        __builtin_amdgcn_sched_barrier(0);                                                                              \
    } while (0)
#define TN_STAMP_INIT()                                                                                                 \
    unsigned long long st_prev, st_sum[TN_NSEG] = {};                                                                   \
    TN_STAMP_NOW(st_prev)
#define TN_STAMP(seg_)                                                                                                  \
    do {                                                                                                                \
        unsigned long long now_;                                                                                        \
        TN_STAMP_NOW(now_);                                                                                             \
        st_sum[seg_] += now_ - st_prev;                                                                                 \
        st_prev = now_;                                                                                                 \
    } while (0)
#define TN_STAMP_STORE()                                                                                                \
    do {                                                                                                                \
        if (blockIdx.x < 256 && (wave & 3) == 0 && lane == 0)                                                           \
            for (int k_ = 0; k_ < TN_NSEG; ++k_) tn_stamp_sums[blockIdx.x][wr][k_] = st_sum[k_];                        \
    } while (0)
#else
#define TN_STAMP_INIT() do {} while (0)
#define TN_STAMP(seg_) do {} while (0)
#define TN_STAMP_STORE() do {} while (0)
#endif

__global__ __launch_bounds__(512, 2) void gemm3_tn_kernel(const TNArgs ta) {
    constexpr int NJ = 4, STAGE = 64 * 512, NSTAGE_A = 3, NSTAGE_B = 2, OFF_B = NSTAGE_A * STAGE, WAITN = 8;
    __shared__ __attribute__((aligned(16))) char smem[(NSTAGE_A + NSTAGE_B) * STAGE];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 2, wc = wave & 3;
    const int g = lane >> 4, li = lane & 15;
    const int G = gridDim.x;
    const int xcd = blockIdx.x & 7, qd = G >> 3, rm = G & 7;
    const int tile = (xcd < rm ? xcd * (qd + 1) : rm * (qd + 1) + (xcd - rm) * qd) + (blockIdx.x >> 3);
    int pi = 0;
#pragma unroll
    for (int k = 1; k < TN_MAXG; ++k) pi += (k < ta.count && tile >= ta.tile_start[k]) ? 1 : 0;
    const TNProb& pr = ta.p[pi];
    const int lt = tile - ta.tile_start[pi], tn = ta.tiles_n[pi];
    const int m0 = (lt / tn) * 256, n0 = (lt % tn) * 256;
    const int M = pr.M, N = pr.N, K = ta.K;
    const int nkt = (K + 63) >> 6;
    const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(pr.A), 0, (int)(((int64_t)(K - 1) * pr.lda + M) * 2), 0x00020000);
    const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(pr.B), 0, (int)(((int64_t)(K - 1) * pr.ldb + N) * 2), 0x00020000);
    const unsigned a_step = 64u * (unsigned)pr.lda * 2u, b_step = 64u * (unsigned)pr.ldb * 2u;
    unsigned ao[4], bo[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        ao[j] = piece_src<true, 256, 64>(wave * 4 + j, lane, pr.lda, m0, M);
        bo[j] = piece_src<true, 256, 64>(wave * 4 + j, lane, pr.ldb, n0, N);
    }
    int ik = 0, ista = 0, istb = 0;
    bool issued = false;
#define TN_ISSUE_A_LO()                                                                                                 \
    do {                                                                                                                \
        issued = ik < nkt;                                                                                              \
        if (issued) {                                                                                                   \
            char* st_ = smem + ista * STAGE + wave * 4096;                                                              \
            const unsigned sa = (unsigned)ik * a_step;                                                                  \
            MR_DMA(ra, MR_LDS_PTR(void, st_), 16, ao[0], sa, 0, 0);                                                     \
            MR_DMA(ra, MR_LDS_PTR(void, st_ + 1024), 16, ao[1], sa, 0, 0);                                              \
        }                                                                                                               \
    } while (0)
#define TN_ISSUE_A_HI()                                                                                                 \
    do {                                                                                                                \
        if (issued) {                                                                                                   \
            char* st_ = smem + ista * STAGE + wave * 4096;                                                              \
            const unsigned sa = (unsigned)ik * a_step;                                                                  \
            MR_DMA(ra, MR_LDS_PTR(void, st_ + 2048), 16, ao[2], sa, 0, 0);                                              \
            MR_DMA(ra, MR_LDS_PTR(void, st_ + 3072), 16, ao[3], sa, 0, 0);                                              \
            ista = (ista == NSTAGE_A - 1) ? 0 : ista + 1;                                                               \
        }                                                                                                               \
    } while (0)
#define TN_ISSUE_A()                                                                                                    \
    do {                                                                                                                \
        TN_ISSUE_A_LO();                                                                                                \
        TN_ISSUE_A_HI();                                                                                                \
    } while (0)
#define TN_ISSUE_B()                                                                                                    \
    do {                                                                                                                \
        if (ik < nkt) {                                                                                                 \
            char* sb_ = smem + OFF_B + istb * STAGE + wave * 4096;                                                      \
            const unsigned sb = (unsigned)ik * b_step;                                                                  \
            MR_DMA(rb, MR_LDS_PTR(void, sb_), 16, bo[0], sb, 0, 0);                                                     \
            MR_DMA(rb, MR_LDS_PTR(void, sb_ + 1024), 16, bo[1], sb, 0, 0);                                              \
            MR_DMA(rb, MR_LDS_PTR(void, sb_ + 2048), 16, bo[2], sb, 0, 0);                                              \
            MR_DMA(rb, MR_LDS_PTR(void, sb_ + 3072), 16, bo[3], sb, 0, 0);                                              \
            istb = (istb == NSTAGE_B - 1) ? 0 : istb + 1;                                                               \
            ++ik;                                                                                                       \
        }                                                                                                               \
    } while (0)
    TN_ISSUE_A(); TN_ISSUE_B();
    TN_ISSUE_A(); TN_ISSUE_B();
    if (issued) wait_vmcnt<WAITN>(); else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    G3_BARRIER();
    if (wr == 1) G3_BARRIER();

    f32x4 acc[8][NJ];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    int csa = 0, csb = 0;
    TN_STAMP_INIT();
    for (int t = 0; t < nkt; ++t) {
        const char* As = smem + csa * STAGE;
        const char* Bs = smem + OFF_B + csb * STAGE;
        bf16x8 a[4][2], b[NJ][2];
        // ---------------- phase 0, memory section: B (16 reads), the kk = 0 halves of A0 (8 reads), two A pieces of k-tile t+2 ----------------
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) b[j][kk] = frag<true, 256, 64>(Bs, wc * 64 + j * 16, kk, lane);
        __builtin_amdgcn_sched_barrier(0);      // B before A: the counted waits below rely on the issue order
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i][0] = frag<true, 256, 64>(As, wr * 128 + i * 16, 0, lane);
        __builtin_amdgcn_sched_barrier(0);
        TN_ISSUE_A_LO();
        G3_LGKM(8);                             // every B read is back AHEAD of the barrier (phase 1 restages B); the 8 A0 reads may still fly
        TN_STAMP(0);
        G3_BARRIER();
        TN_STAMP(1);
        // ---------------- phase 0, MFMA section: A0 x B, kk = 0 then kk = 1 (each accumulator's k order is that of the two-drain schedule).
        // Reads land under the wave's own MFMAs: the kk = 1 halves of A0 are requested first and waited for 16 MFMAs later; the A1
        // fragments replace the A0 fragments IN PLACE, each half requested behind the last MFMA that read its registers.  LDS data returns
        // in issue order, and behind the fragments a wait is for exactly 8 reads are outstanding. ----------------
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i][1] = frag<true, 256, 64>(As, wr * 128 + i * 16, 1, lane);
        __builtin_amdgcn_sched_barrier(0);
        G3_LGKM(8);                             // A0, kk = 0
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[j][0], a[i][0], acc[i][j], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i][0] = frag<true, 256, 64>(As, wr * 128 + 64 + i * 16, 0, lane);
        __builtin_amdgcn_sched_barrier(0);
        G3_LGKM(8);                             // A0, kk = 1
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[j][1], a[i][1], acc[i][j], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i][1] = frag<true, 256, 64>(As, wr * 128 + 64 + i * 16, 1, lane);
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(0);
        TN_STAMP(2);
        G3_BARRIER();
        TN_STAMP(3);
        // ---------------- phase 1, memory section: no fragment reads of its own -- the other two A pieces and the four B pieces of k-tile t+2.
        // The A1 reads are retired ahead of the barrier (behind it the other group's next phase 0 restages A) ----------------
        TN_ISSUE_A_HI();
        TN_ISSUE_B();
        G3_LGKM(0);
        TN_STAMP(4);
        if (issued) wait_vmcnt<WAITN>(); else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        TN_STAMP(5);
        G3_BARRIER();
        TN_STAMP(6);
        // ---------------- phase 1, MFMA section: A1 x B ----------------
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < NJ; ++j) acc[4 + i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[j][kk], a[i][kk], acc[4 + i][j], 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
        TN_STAMP(7);
        G3_BARRIER();
        TN_STAMP(8);
        csa = (csa == NSTAGE_A - 1) ? 0 : csa + 1;
        csb = (csb == NSTAGE_B - 1) ? 0 : csb + 1;
    }
    TN_STAMP_STORE();
    if (wr == 0) G3_BARRIER();          // pairs with group 1's last barrier

    // epilogue: bf16 stores, widened to 16 B (see the NT kernel's store_pair)
    const unsigned c_bytes = (unsigned)(((int64_t)(M - 1) * pr.ldc + N) * 2);
    const __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc(pr.C, 0, (int)c_bytes, 0x00020000);
    const int wrow0 = m0 + wr * 128, wcol0 = n0 + wc * 64;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int gm = wrow0 + i * 16 + li;
        const unsigned rowoff = (unsigned)gm * (unsigned)pr.ldc * 2u;
#pragma unroll
        for (int jp = 0; jp < NJ / 2; ++jp) {
            bf16x4 va, vb;
#pragma unroll
            for (int r = 0; r < 4; ++r) { va[r] = (__bf16)acc[i][2 * jp][r]; vb[r] = (__bf16)acc[i][2 * jp + 1][r]; }
            u32x2 ua = __builtin_bit_cast(u32x2, va), ub = __builtin_bit_cast(u32x2, vb);
            const auto s0 = __builtin_amdgcn_permlane16_swap(ua[0], ub[0], false, false);
            const auto s1 = __builtin_amdgcn_permlane16_swap(ua[1], ub[1], false, false);
            const int col = wcol0 + (2 * jp + (g & 1)) * 16 + (g >> 1) * 8;
            const unsigned off = (gm < M && col < N) ? rowoff + (unsigned)col * 2u : OOB;
            __builtin_amdgcn_raw_buffer_store_b128(u32x4{s0[0], s1[0], s0[1], s1[1]}, rc, off, 0, 0);
        }
    }
}

}  // namespace g3

void mr_gemm3_launch(const g256::G256Args& ga, int bn, int mode, int ph, int64_t grid_size, hipStream_t s) {
    dim3 grid((unsigned)grid_size), block(512);
#define G3_LAUNCH(MODE)                                                                               \
    do {                                                                                              \
        if (ph == 1) {                                                                                \
            if (bn == 256) hipLaunchKernelGGL((g3::gemm3_kernel<256, MODE, (MODE == 4 ? 2 : 1)>), grid, block, 0, s, ga);   \
            else hipLaunchKernelGGL((g3::gemm3_kernel<192, MODE, 1>), grid, block, 0, s, ga);             \
        } else {                                                                                      \
            if (bn == 256) hipLaunchKernelGGL((g3::gemm3_kernel<256, MODE, 2>), grid, block, 0, s, ga);   \
            else hipLaunchKernelGGL((g3::gemm3_kernel<192, MODE, 2>), grid, block, 0, s, ga);             \
        }                                                                                             \
    } while (0)
    switch (mode) {
        case 0: G3_LAUNCH(0); break;
        case 1: G3_LAUNCH(1); break;
        case 2: G3_LAUNCH(2); break;
        case 3: G3_LAUNCH(3); break;
        default: G3_LAUNCH(4); break;
    }
#undef G3_LAUNCH
}

void mr_gemm3_tn_launch(const g3::TNArgs& ta, int64_t tiles, hipStream_t s) {
    hipLaunchKernelGGL(g3::gemm3_tn_kernel, dim3((unsigned)tiles), dim3(512), 0, s, ta);
#ifdef MR_TN_STAMPS
    // diagnostic build: one line per stamped wave and launch on stderr -- workgroup, group, k-tiles, the nine segment sums in shader clocks
    static unsigned long long host_sums[256][2][g3::TN_NSEG];
    if (hipStreamSynchronize(s) != hipSuccess || hipMemcpyFromSymbol(host_sums, HIP_SYMBOL(g3::tn_stamp_sums), sizeof(host_sums)) != hipSuccess) return;
    for (int w = 0; w < (tiles < 256 ? (int)tiles : 256); ++w)
        for (int g = 0; g < 2; ++g) {
            fprintf(stderr, "TNSTAMP %d %d %d", w, g, (ta.K + 63) >> 6);
            for (int k = 0; k < g3::TN_NSEG; ++k) fprintf(stderr, " %llu", host_sums[w][g][k]);
            fprintf(stderr, "\n");
        }
#endif
}
