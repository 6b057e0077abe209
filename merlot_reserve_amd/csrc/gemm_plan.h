// Launch plans of the GEMM kernels: the argument structs the router (gemm_route.cpp) fills and the one launcher per kernel family
// that turns a plan into a template instance.  The launchers live beside their kernels and hold no policy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/mreserve_hip.h"

namespace g256 {

constexpr int BM = 256, BK = 64;
constexpr int MAXG = 4;
// One launch = up to MAXG independent problems (same layouts and tile width) sharing the persistent grid: the four
// weight gradients of a transformer layer fill the 256 CUs together, with no split-K traffic.
struct G256Args {
    int count, nwork, splits, kt_per_split;
    // XCD-blocked tile order (xmode = 1; single problem, no split-K, grid = 256): the 8 XCDs own the cells of a px x py
    // partition of the tile grid and walk their cell in panels of XPANEL tile columns, so that the 32 workgroups of an
    // XCD -- which move through K in lockstep -- ask their L2 for few distinct operand strips at a time, and a cell's
    // slice of B stays L2-resident while its A strips stream through.  (With the plain row-major order every XCD swept
    // all of B once per round of 256 tiles: rocprofv3 FETCH_SIZE showed 6x the operand bytes leaving L2 per launch.)
    int xmode, px, py, tm, tn;
    int xpanel;            // tile columns per panel of a cell's walk (0 = XPANEL)
    int tiles_n[MAXG], tile_start[MAXG + 1];
    mr_gemm_args p[MAXG];
};

}  // namespace g256

namespace g3 {

// the grouped TN weight-gradient kernel: one 256 x 256 output tile per workgroup, up to TN_MAXG problems with one K
struct TNProb { const void* A; const void* B; void* C; int M, N, lda, ldb, ldc, pad; };
constexpr int TN_MAXG = 20;
struct TNArgs { int count, K; int tile_start[TN_MAXG + 1]; int tiles_n[TN_MAXG]; TNProb p[TN_MAXG]; };

}  // namespace g3

// gemm.hip: 128 x 128 x 64 tiles
constexpr int SMALL_TILE = 128, SMALL_BK = 64;
constexpr int SMALL_MAXG = 8;          // problems of one grouped small-tile launch

// gemm.hip: `tiles` output tiles (tiles_n per row) x `splits` K ranges of kt_per_split k-tiles; the split-K reduction (+ bias);
// several small problems of one operand layout over `tiles` tiles in one launch
void mr_gemm_small_launch(const mr_gemm_args* a, int64_t tiles, int64_t tiles_n, int64_t splits, int64_t kt_per_split, hipStream_t s);
void mr_gemm_splitk_reduce(const mr_gemm_args* a, int64_t splits, hipStream_t s);
void mr_gemm_small_grouped_launch(const mr_gemm_args* list, int count, int64_t tiles, hipStream_t s);
// gemm256.hip: the one-barrier kernel, tile width bn (96, 128, 192, 256), `grid` persistent workgroups
void mr_gemm256_launch(const g256::G256Args& ga, int bn, int64_t grid, hipStream_t s);
// gemm3.hip: the ping-pong kernel (epilogue mode 0-4, ph phases per k-tile) and the grouped TN kernel (one workgroup per tile)
void mr_gemm3_launch(const g256::G256Args& ga, int bn, int mode, int ph, int64_t grid, hipStream_t s);
void mr_gemm3_tn_launch(const g3::TNArgs& ta, int64_t tiles, hipStream_t s);
// gemm4.hip: the one-wave-per-SIMD kernel on the ping-pong kernel's plan (epilogue mode 0, 3 or 5)
int mr_gemm4_launch(const g256::G256Args& ga, int bn, int mode, int64_t grid, hipStream_t s);
// gemm5.hip: the two-per-CU kernel (256 x 128 tiles) or its 128 x 128 geometry; epilogue mode 0-5, start stagger of the second resident
void mr_gemm5_launch(const g256::G256Args& ga, bool rows128, int mode, int stagger_mode, int stagger_units, int64_t grid, hipStream_t s);
