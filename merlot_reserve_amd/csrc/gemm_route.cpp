// The GEMM router: every decision of mr_gemm / mr_gemm_grouped -- which kernel family takes a problem, its tile width, epilogue
// instance, schedule, grid and tile order -- in one place.  The kernel files keep their kernels and one launcher each (gemm_plan.h).
// One problem goes to the first family that takes it:
//   gemm5 (two workgroups per CU, gemm5.hip)  ->  the ping-pong kernel (gemm3.hip; or its one-wave-per-SIMD twin, gemm4.hip)
//   ->  the one-barrier kernel (gemm256.hip)  ->  the 128 x 128 small-tile kernel with split-K (gemm.hip).
// Host code only.
#include <string.h>
#include "gemm_plan.h"
#include "mr_common.h"
#include "mr_options.h"

namespace {

constexpr int64_t NUM_CU = 256;    // MI355X

// Persistent workgroups a launch may fill (option "gemm_cus": 256, or fewer -- a multiple of 8 -- while a collective kernel holds CUs: a
// 256-workgroup grid would then run its last workgroups as a second round behind the others).  gemm5 has two per CU; the one-barrier
// kernel always fills 256.
int64_t persistent_cus() {
    const int c = mr_opts().gemm_cus;
    return (c >= 64 && c < NUM_CU) ? (c & ~7) : NUM_CU;
}

// The epilogue of a problem: 0 bias | 1 bias + "rotary" scales | 2 bias + GELU, gelu' copy to c2 | 3 + residual | 4 x aux (+ column sums) |
// 5 plain product.  gemm3 runs 5 as 0 (its bias modes start from a null bias as zeros); gemm4 takes 0, 3 and 5.
int epi_mode(const mr_gemm_args* a) {
    if (a->c2) return 2;
    if (a->rot_tab) return 1;
    if (a->residual) return 3;
    if (a->aux) return 4;
    return a->bias ? 0 : 5;
}

bool plain(const mr_gemm_args* a) { return !a->rot_tab && !a->c2 && a->act == MR_ACT_NONE && !a->residual && !a->aux && a->out_grp == 0; }

// What the fused-epilogue NT kernels (gemm3, gemm4, gemm5) can take: A [M,K], B [N,K], K % 64 == 0, bf16 output, 32-bit buffer offsets,
// at most one extra operand, c2 exactly with GELU, column sums only with aux, no bias with a residual / aux (the bias rides in the
// accumulators of the bias modes only).
bool nt_fusable(const mr_gemm_args* a) {
    if (a->transA || !a->transB || a->c_dtype != MR_DT_BF16 || a->K % 64 != 0) return false;
    if (a->M * a->lda * 2 >= (1LL << 31) || a->N * a->ldb * 2 >= (1LL << 31)) return false;
    const int64_t last = a->out_grp > 0 ? ((a->M - 1) / a->out_grp) * a->out_grp_stride + a->out_grp_off + (a->M - 1) % a->out_grp : a->M - 1;
    if ((last * a->ldc + a->N) * 2 >= (1LL << 31)) return false;
    const int n_extra = (a->rot_tab != nullptr) + (a->residual != nullptr) + (a->aux != nullptr) + (a->c2 != nullptr);
    if (n_extra > 1) return false;
    if ((a->c2 != nullptr) != (a->act == MR_ACT_GELU1702)) return false;
    if (a->colsum && !a->aux) return false;
    return !(a->bias && (a->residual || a->aux));
}

// ---- gemm5 ----
// Tile height: 128 x 128 tiles (deep ring, one workgroup per CU) where even the 128-row grid has no more tiles than the chip has CUs, or
// on request (option "gemm5" = 3); 256 x 128 (two workgroups per CU) otherwise.
bool gemm5_rows128(const mr_gemm_args* a) {
    const int v = mr_opts().gemm5;
    if (v == 3) return true;
    if (v == 1) return false;
    return ((a->M + 127) / 128) * ((a->N + 127) / 128) <= 256;
}

// Which problems go to gemm5: option "gemm5" 1 / 3 = every one it can take (tests, A/B), 0 = none, -1 = the policy below.
bool gemm5_wanted(const mr_gemm_args* a) {
    const int v = mr_opts().gemm5;
    if (v == 0 || (a->colsum != nullptr && !a->aux)) return false;
    if (!nt_fusable(a) || a->K < 128) return false;
    if (((a->M + 127) / 128) * ((a->N + 127) / 128) > 64 * 2 * persistent_cus()) return false;     // <= 64 items per workgroup (either tile height)
    if (v == 1 || v == 3) return true;
    // Default policy (measured, scripts/micro/gemm3_test g5time): the few-tile short-K problems -- at most one 256 x 128 tile per CU, K <= 1024:
    // the audio / span towers' 768-wide projections, the span and VCR-ViT QKV -- run 8-13 % faster here than on the one-barrier kernel's
    // 96-wide tiles (16.3 vs 18.0, 20.6 vs 23.4, 15.3 vs 17.4, 24.5 vs 26.9 us); everything with more tiles or a longer K is slower
    // (the 256 x 128 tile pair of a CU writes 1.5 x the operand bytes into LDS: DESIGN.md section 3).
    // Round 4, 128 x 128 tiles: problems with at most one such tile per CU (M = 2308 / 3072, N = 768 / 1024, any K) run 25-40 % faster there than
    // on either of the above (gemm5.hip's header); with more tiles the 256-row geometries win (audio tower, M = 5952: 36-38 vs 52 us at K = 3072).
    if (a->colsum != nullptr || a->M < 1024 || a->N < 256) return false;
    if (gemm5_rows128(a)) return true;
    const int64_t tiles = ((a->M + 255) / 256) * ((a->N + 127) / 128);
    return tiles <= 256 && a->K <= 1024;
}

// ---- the ping-pong kernel (gemm3) and its hand-off to gemm4 ----
// Takes: the NT epilogue combinations above and at least one full round of 256-row tiles' worth of work.  Option "gemm3": 0 = never,
// 256 / 192 = any shape it can take, on tiles that wide (tests).
bool gemm3_eligible(const mr_gemm_args* a) {
    const int v = mr_opts().gemm3;
    if (!v || !nt_fusable(a)) return false;
    const bool forced = v == 256 || v == 192;
    if (!forced && (a->K < 128 || a->N < 192 || a->M < 1024)) return false;
    // enough tiles to fill the chip (short-K problems with few tiles go to the split-K path of the one-barrier kernel)
    constexpr int64_t MIN_TILES = 128;
    const int64_t tm = (a->M + 255) / 256;
    if (tm * ((a->N + 191) / 192) > 64 * persistent_cus()) return false;     // <= 64 items per workgroup (the kernel keeps them one per lane)
    if (!forced && tm * ((a->N + 255) / 256) < MIN_TILES) return false;
    return true;
}

// gemm4 (one wave per SIMD, the ping-pong kernel's tile plan) has the bias / residual / plain epilogues, but not the 256-wide bias mode:
// 256 accumulators + the bias rows overflow the wave's 512 registers (183 spilled, reloads inside the k-loop, 299 vs 91 us), so that
// combination stays on the ping-pong kernel.  Option "gemm4" = 0 keeps everything there.
bool gemm4_takes(const mr_gemm_args* a, int bn) {
    return mr_opts().gemm4 != 0 && !a->c2 && !a->rot_tab && !a->aux && !(bn == 256 && a->bias && !a->residual);
}

// ---- the one-barrier kernel (gemm256) ----
bool gemm256_eligible(const mr_gemm_args* a) {
    if (a->M < 512 || a->N < 96) return false;
    if (a->residual && a->aux) return false;              // the epilogue prefetches ONE bf16 operand
    if (!a->transA && a->K % 64 != 0) return false;       // K-contiguous operands are fetched in whole 128-B rows
    if (a->transB && a->K % 64 != 0) return false;
    const int64_t a_rows = a->transA ? a->K : a->M, b_rows = a->transB ? a->N : a->K;
    if (a_rows * a->lda * 2 >= (1LL << 31) || b_rows * a->ldb * 2 >= (1LL << 31)) return false;   // 32-bit buffer offsets
    return true;
}

// Tile width: the one that wastes the fewest CU-rounds (256 workgroups per round, one per CU); option "gemm_tile_n" forces one.
int gemm256_tile_n(const mr_gemm_args* a, int64_t tm) {
    // measured: a 96-wide tile costs ~0.91 of a 128-wide one (the A side and the LDS-DMA issue do not shrink); a 256-wide one ~1.9
    // (twice the FLOPs for 4/3 of the LDS-DMA bytes, but its 2-stage ring drains behind every k-tile)
    constexpr int64_t C96 = 91, C128 = 100, C192 = 150, C256 = 180;
    const bool can256 = a->N >= 256, can192 = a->N >= 192;
    int bn = 128;
    const int64_t t128 = tm * ((a->N + 127) / 128), t96 = tm * ((a->N + 95) / 96), t256 = tm * ((a->N + 255) / 256);
    const int64_t c128 = ((t128 + 255) / 256) * C128, c96 = ((t96 + 255) / 256) * C96, c256 = ((t256 + 255) / 256) * C256;
    int64_t best = c128;
    if (c96 < best && !a->rot_tab) { bn = 96; best = c96; }       // the prefetched "rotary" scales assume whole heads per wave
    if (can256 && c256 < best) { bn = 256; best = c256; }
    const int64_t t192 = tm * ((a->N + 191) / 192), c192 = ((t192 + 255) / 256) * C192;
    if (can192 && c192 < best) bn = 192;
    const int f = mr_opts().tile_n;
    if (f == 96 || f == 128 || (f == 256 && can256) || (f == 192 && can192)) bn = f;
    if (a->rot_tab && bn == 96) bn = 128;
    if (a->colsum && bn == 256 && can192) bn = 192;     // the column-sum accumulators beside a 256-wide tile's 128 accumulators spill (measured: +22 us)
    return bn;
}

// ---- shared plan pieces ----
// Split-K for problems with few output tiles and a long contraction (every wgrad; they cannot fill 256 CUs otherwise): about `target` work
// items, fewer than `max_tiles` tiles, at least `min_kt` k-tiles per split, at most `cap` splits and what the workspace holds; plain
// products only (the reduction adds the bias).  Returns the number of splits and their k-tiles.
int64_t splitk(const mr_gemm_args* a, int64_t tiles, int64_t nk, int64_t max_tiles, int64_t target, int64_t min_kt, int64_t cap, int64_t* kt_per_split) {
    int64_t splits = 1;
    if (a->workspace && plain(a) && a->N % 4 == 0 && tiles < max_tiles && nk >= 16) {
        splits = (target + tiles - 1) / tiles;
        if (splits > nk / min_kt) splits = nk / min_kt;
        if (splits > cap) splits = cap;
        const int64_t fit = a->workspace_bytes / (a->M * a->N * (int64_t)sizeof(float));
        if (splits > fit) splits = fit;
        if (splits < 2) splits = 1;
    }
    *kt_per_split = (nk + splits - 1) / splits;
    return (nk + *kt_per_split - 1) / *kt_per_split;
}

// One problem's G256Args: row-major tile order until xcd_partition says otherwise.
g256::G256Args single_args(const mr_gemm_args* a, int64_t nwork, int64_t splits, int64_t kt_per_split, int64_t tn) {
    g256::G256Args ga;
    memset(&ga, 0, sizeof(ga));
    ga.count = 1; ga.nwork = (int)nwork; ga.splits = (int)splits; ga.kt_per_split = (int)kt_per_split;
    ga.tiles_n[0] = (int)tn;
    for (int k = 1; k <= g256::MAXG; ++k) ga.tile_start[k] = 0x7fffffff;
    ga.p[0] = *a;
    return ga;
}

// XCD partition of a single problem's tm x tn tile grid (G256Args.xmode) when a full grid of `slots` persistent workgroups has at least two
// rounds of tiles: fewest rounds first (the slowest XCD sets the time), then least traffic out of L2.
void xcd_partition(g256::G256Args& ga, const mr_gemm_args* a, int64_t tm, int64_t tn, int64_t slots, int64_t grid) {
    if (grid != slots || tm * tn < 2 * slots) return;
    const double a_bytes = 2.0 * a->M * a->K, b_bytes = 2.0 * a->N * a->K;
    double best = 1e300;
    for (int px = 1; px <= 8; px *= 2) {
        const int py = 8 / px;
        if (px > tm || py > tn) continue;
        int64_t rounds = 0;
        for (int xi = 0; xi < px; ++xi)
            for (int xj = 0; xj < py; ++xj) {
                const int64_t hm = (xi + 1) * tm / px - xi * tm / px, hn = (xj + 1) * tn / py - xj * tn / py;
                const int64_t r = (hm * hn + slots / 8 - 1) / (slots / 8);
                if (r > rounds) rounds = r;
            }
        const bool b_fits = b_bytes / py < 2.5e6;         // a cell's B slice stays in the XCD's 4-MiB L2
        const double traffic = a_bytes * py + b_bytes * px * (b_fits ? 1.0 : (double)rounds);
        const double cost = (double)rounds * 1e12 + traffic;
        if (cost < best) { best = cost; ga.px = px; ga.py = py; }
    }
    if (best < 1e300) { ga.xmode = 1; ga.tm = (int)tm; ga.tn = (int)tn; }
}

// ---- single-problem routes ----
int route_gemm5(const mr_gemm_args* a, hipStream_t s) {
    const int64_t ncu = persistent_cus();
    const bool r128 = gemm5_rows128(a);                 // 128 x 128 tiles, deep ring, one workgroup per CU
    const int64_t slots = r128 ? ncu : 2 * ncu;         // workgroups of a full grid
    const int64_t tm = (a->M + (r128 ? 127 : 255)) / (r128 ? 128 : 256), tn = (a->N + 127) / 128, nwork = tm * tn;
    const int64_t gsz = nwork < slots ? nwork : slots;
    g256::G256Args ga = single_args(a, nwork, 1, a->K / 32, tn);
    xcd_partition(ga, a, tm, tn, slots, gsz);
    const int mode = epi_mode(a);
    // the second resident workgroup of a CU starts ~ one k-loop late: K / 32 steps of ~600 cycles, in units of 2048 cycles; one workgroup
    // per CU has nobody to be out of phase with (three per CU: no phase is set)
    const int st_mode = (gsz <= ncu || r128) ? 0 : 1;
    const int st_units = (int)((a->K / 32) * 600 / 2048);
    mr_gemm5_launch(ga, r128, mode, st_mode, st_units, gsz, s);
    mr_note_route(r128 ? "g5::gemm5_kernel<%d,4,128,8>" : "g5::gemm5_kernel<%d,4>", mode);
    MR_CHECK_LAUNCH("mr_gemm (gemm5)");
    return MR_OK;
}

int route_pingpong(const mr_gemm_args* a, hipStream_t s) {
    const int64_t tm = (a->M + 255) / 256, ncu = persistent_cus();
    // tile width: fewest CU-rounds, a 192-wide tile costing 0.78 of a 256-wide one
    const int64_t t256 = tm * ((a->N + 255) / 256), t192 = tm * ((a->N + 191) / 192);
    const int64_t c256 = ((t256 + ncu - 1) / ncu) * 100, c192 = ((t192 + ncu - 1) / ncu) * 78;
    int bn = (c192 < c256) ? 192 : 256;
    if (mr_opts().gemm3 == 256 || mr_opts().gemm3 == 192) bn = mr_opts().gemm3;
    const int64_t tn = (a->N + bn - 1) / bn, nwork = tm * tn;
    const int64_t gsz = nwork < ncu ? nwork : ncu;
    g256::G256Args ga = single_args(a, nwork, 1, a->K / 64, tn);
    xcd_partition(ga, a, tm, tn, ncu, gsz);
    const int mode = epi_mode(a);
    if (gemm4_takes(a, bn)) {
        const int rc = mr_gemm4_launch(ga, bn, mode, gsz, s);
        if (rc != MR_OK) return rc;
        mr_note_route("g4::gemm4_kernel<%d,%d>", bn, mode);
        MR_CHECK_LAUNCH("mr_gemm (gemm4)");
        return MR_OK;
    }
    const int m3 = mode == 5 ? 0 : mode;
    // one phase per k-tile (half the barriers: 2-7 % faster at K <= 4096) except where it measured slower: the 256-wide aux / column-sum
    // epilogue (its prefetch registers + the one-phase schedule's spill: 94 vs 86 us on the fc1 dgrad) and very long k-loops, where B
    // requested one phase ahead by ONE group lands later than the two-phase schedule's (8192^3: 745 vs 729 us)
    const int ph_auto = ((m3 == 4 && bn == 256) || a->K >= 8192) ? 2 : 1;
    int ph = mr_opts().gemm3_ph ? mr_opts().gemm3_ph : ph_auto;
    if (m3 == 4 && bn == 256) ph = 2;      // <256,4,1> is not built: 20 spilled registers with a reload inside the k-loop's MFMA block
    mr_gemm3_launch(ga, bn, m3, ph, gsz, s);
    mr_note_route("g3::gemm3_kernel<%d,%d,%d>", bn, m3, ph);
    MR_CHECK_LAUNCH("mr_gemm (ping-pong kernel)");
    return MR_OK;
}

int route_one_barrier(const mr_gemm_args* a, hipStream_t s) {
    const int64_t tm = (a->M + g256::BM - 1) / g256::BM;
    const int bn = gemm256_tile_n(a, tm);
    const int64_t tn = (a->N + bn - 1) / bn, nk = (a->K + g256::BK - 1) / g256::BK;
    int64_t kps;
    const int64_t splits = splitk(a, tm * tn, nk, 192, 512, 6, 64, &kps);
    const int64_t nwork = tm * tn * splits;
    const int64_t gsz = nwork < NUM_CU ? nwork : NUM_CU;        // persistent: one workgroup per CU
    g256::G256Args ga = single_args(a, nwork, splits, kps, tn);
    if (splits == 1) xcd_partition(ga, a, tm, tn, NUM_CU, gsz);
    mr_gemm256_launch(ga, bn, gsz, s);
    if (splits > 1) mr_gemm_splitk_reduce(a, splits, s);
    mr_note_route("g256::gemm256_kernel<%d,%d,%d>%s", bn, (int)a->transA, (int)a->transB, splits > 1 ? " + splitk_reduce" : "");
    MR_CHECK_LAUNCH("mr_gemm (256-row kernel)");
    return MR_OK;
}

int route_small(const mr_gemm_args* a, hipStream_t s) {
    const int64_t tm = (a->M + SMALL_TILE - 1) / SMALL_TILE, tn = (a->N + SMALL_TILE - 1) / SMALL_TILE;
    MR_CHECK_ARG(tm * tn < (1LL << 30), "mr_gemm: grid too large");
    int64_t kps;
    const int64_t splits = splitk(a, tm * tn, (a->K + SMALL_BK - 1) / SMALL_BK, 384, 768, 8, 32, &kps);
    mr_gemm_small_launch(a, tm * tn, tn, splits, kps, s);
    if (splits > 1) mr_gemm_splitk_reduce(a, splits, s);
    mr_note_route("gemm_bf16_kernel<%d,%d>%s", (int)a->transA, (int)a->transB, splits > 1 ? " + splitk_reduce" : "");
    MR_CHECK_LAUNCH("mr_gemm");
    return MR_OK;
}

// ---- grouped routes ----
// Weight gradients on the TN ping-pong kernel: <= TN_MAXG problems, all transA = 1 / transB = 0 with one K, bf16 outputs, no epilogue,
// worth it when the tiles fill most of the chip (one tile per workgroup, one workgroup per CU) and K is long.  Fills `ta` when it takes them.
bool tn_group(const mr_gemm_args* list, int count, g3::TNArgs& ta, int64_t* tiles_out) {
    if (!mr_opts().gemm3 || count < 1 || count > g3::TN_MAXG) return false;
    if (mr_opts().group_tile_n != 0) return false;   // an explicitly requested tile width of the one-barrier kernel
    memset(&ta, 0, sizeof(ta));
    int64_t tiles = 0;
    for (int k = 0; k < count; ++k) {
        const mr_gemm_args* a = &list[k];
        if (!a->transA || a->transB || a->c_dtype != MR_DT_BF16 || a->K != list[0].K) return false;
        if (a->bias || a->rot_tab || a->c2 || a->act != MR_ACT_NONE || a->residual || a->aux || a->out_grp != 0 || a->colsum) return false;
        if (a->M % 8 || a->N % 8 || a->lda % 8 || a->ldb % 8 || a->ldc % 8) return false;
        if (a->K * a->lda * 2 >= (1LL << 31) || a->K * a->ldb * 2 >= (1LL << 31) || a->M * a->ldc * 2 >= (1LL << 31)) return false;
        const int64_t tm = (a->M + 255) / 256, tn = (a->N + 255) / 256;
        ta.tile_start[k] = (int)tiles;
        ta.tiles_n[k] = (int)tn;
        tiles += tm * tn;
        ta.p[k] = g3::TNProb{a->A, a->B, a->C, (int)a->M, (int)a->N, (int)a->lda, (int)a->ldb, (int)a->ldc, 0};
    }
    ta.tile_start[count] = (int)tiles;
    ta.count = count;
    ta.K = (int)list[0].K;
    *tiles_out = tiles;
    const bool forced = mr_opts().gemm3 == 256;
    return forced || !(tiles < 160 || tiles > 4 * NUM_CU || list[0].K < 2048);
}

// A member of a grouped small-tile launch: the first problem's layout, none of the bigger kernels would take it, and it passes the
// checks mr_gemm makes beyond mr_gemm_grouped's.
bool small_group_member(const mr_gemm_args* a, const mr_gemm_args& first) {
    if (a->transA != first.transA || a->transB != first.transB || gemm5_wanted(a) || gemm3_eligible(a) || gemm256_eligible(a)) return false;
    if (((a->transA ? a->M : a->K) + 7) / 8 * 8 > a->lda || ((a->transB ? a->K : a->N) + 7) / 8 * 8 > a->ldb) return false;
    if (!(a->c_dtype == MR_DT_BF16 || (a->c_dtype == MR_DT_F32 && !a->residual && !a->aux && !a->c2 && a->act == MR_ACT_NONE && a->out_grp == 0))) return false;
    if (a->colsum || (a->rot_tab && a->rot_rows <= 0)) return false;
    return a->c_dtype != MR_DT_BF16 || ((!a->residual || a->ldr % 8 == 0) && (!a->aux || a->ldaux % 8 == 0));
}

// The one-barrier kernel over <= MAXG problems with identical transA / transB, each eligible for it, epilogue limited to bias; no split-K.
// Returns false if the group does not qualify (the caller falls back).
bool route_one_barrier_group(const mr_gemm_args* list, int count, hipStream_t s) {
    if (count < 1 || count > g256::MAXG) return false;
    for (int k = 0; k < count; ++k) {
        const mr_gemm_args* a = &list[k];
        if (!gemm256_eligible(a) || a->transA != list[0].transA || a->transB != list[0].transB) return false;
        if (a->rot_tab || a->c2 || a->act != MR_ACT_NONE || a->residual || a->aux || a->out_grp != 0) return false;
    }
    // tile width for the whole group: fewest CU-rounds, a 256-wide tile costing ~1.8 of a 128-wide one (the large model's four weight
    // gradients are 384 tiles of 128 = 1.5 rounds -> 2, but 192 tiles of 256 = one round); option "gemm_group_tile_n" forces one
    constexpr int64_t C256 = 180;
    int64_t t128 = 0, t256 = 0;
    bool can256 = true;
    for (int k = 0; k < count; ++k) {
        const int64_t tm = (list[k].M + g256::BM - 1) / g256::BM;
        t128 += tm * ((list[k].N + 127) / 128);
        t256 += tm * ((list[k].N + 255) / 256);
        can256 = can256 && list[k].N % 256 == 0;
    }
    int bn = (can256 && ((t256 + NUM_CU - 1) / NUM_CU) * C256 < ((t128 + NUM_CU - 1) / NUM_CU) * 100) ? 256 : 128;
    const int f = mr_opts().group_tile_n;
    if (f == 128 || (f == 256 && can256)) bn = f;
    g256::G256Args ga;
    memset(&ga, 0, sizeof(ga));
    int64_t tiles = 0, nk_max = 0;
    for (int k = 0; k <= g256::MAXG; ++k) ga.tile_start[k] = 0x7fffffff;
    for (int k = 0; k < count; ++k) {
        const mr_gemm_args* a = &list[k];
        const int64_t tm = (a->M + g256::BM - 1) / g256::BM, tn = (a->N + bn - 1) / bn;
        ga.tiles_n[k] = (int)tn;
        ga.tile_start[k] = (int)tiles;
        tiles += tm * tn;
        ga.p[k] = *a;
        const int64_t nk = (a->K + g256::BK - 1) / g256::BK;
        if (nk > nk_max) nk_max = nk;
    }
    ga.count = count; ga.nwork = (int)tiles; ga.splits = 1; ga.kt_per_split = (int)nk_max;
    mr_gemm256_launch(ga, bn, tiles < NUM_CU ? tiles : NUM_CU, s);
    mr_note_route("g256::gemm256_kernel<%d,%d,%d> grouped x%d", bn, (int)list[0].transA, (int)list[0].transB, count);
    return true;
}

}  // namespace

extern "C" int64_t mr_gemm_colsum_rows(int64_t M) { return 4 * ((M + g256::BM - 1) / g256::BM); }
extern "C" int32_t mr_gemm_colsum_supported(const mr_gemm_args* a) {
    return a && gemm256_eligible(a) && a->c_dtype == MR_DT_BF16 && a->aux && !a->residual && !a->c2 && a->act == MR_ACT_NONE &&
           !a->rot_tab && a->out_grp == 0 && a->N % 4 == 0;
}

extern "C" int mr_gemm(const mr_gemm_args* a, void* stream) {
    MR_CHECK_ARG(a != nullptr, "mr_gemm: null args");
    MR_CHECK_ARG(a->M > 0 && a->N > 0 && a->K > 0, "mr_gemm: empty problem M=%ld N=%ld K=%ld", (long)a->M, (long)a->N, (long)a->K);
    MR_CHECK_ARG(a->A && a->B && a->C, "mr_gemm: null operand");
    MR_CHECK_ARG(a->lda % 8 == 0 && a->ldb % 8 == 0, "mr_gemm: lda/ldb must be multiples of 8 (got %ld, %ld)", (long)a->lda, (long)a->ldb);
    // the contiguous dimension of each operand is consumed in 16-byte chunks: a ragged extent is allowed when the
    // row is padded (with zeros, by the caller) up to the next multiple of 8 inside the leading dimension
    MR_CHECK_ARG(((a->transA ? a->M : a->K) + 7) / 8 * 8 <= a->lda, "mr_gemm: A rows must be padded to a multiple of 8 elements");
    MR_CHECK_ARG(((a->transB ? a->K : a->N) + 7) / 8 * 8 <= a->ldb, "mr_gemm: B rows must be padded to a multiple of 8 elements");
    MR_CHECK_ARG(((uintptr_t)a->A % 16) == 0 && ((uintptr_t)a->B % 16) == 0 && ((uintptr_t)a->C % 16) == 0,
                 "mr_gemm: operands must be 16-byte aligned");
    if (a->c_dtype == MR_DT_BF16) {
        MR_CHECK_ARG(a->N % 8 == 0 && a->ldc % 8 == 0, "mr_gemm: bf16 output needs N, ldc multiples of 8");
        MR_CHECK_ARG(!a->residual || a->ldr % 8 == 0, "mr_gemm: ldr must be a multiple of 8");
        MR_CHECK_ARG(!a->aux || a->ldaux % 8 == 0, "mr_gemm: ldaux must be a multiple of 8");
    } else {
        MR_CHECK_ARG(a->c_dtype == MR_DT_F32, "mr_gemm: bad c_dtype %d", a->c_dtype);
        MR_CHECK_ARG(!a->residual && !a->aux && !a->c2 && a->act == MR_ACT_NONE && a->out_grp == 0,
                     "mr_gemm: fp32 output supports bias only");
    }
    MR_CHECK_ARG(!a->rot_tab || a->rot_rows > 0, "mr_gemm: rot_rows must be > 0");
    MR_CHECK_ARG(!a->colsum || (mr_gemm_colsum_supported(a) && a->ldcs >= a->N && ((uintptr_t)a->colsum % 16) == 0 && a->ldcs % 4 == 0),
                 "mr_gemm: colsum is only produced by the 256-row kernel with the aux epilogue (ask mr_gemm_colsum_supported)");
    mr_gemm_args with_ws;                    // the current handle's split-K workspace when the caller brings none
    if (a->workspace == nullptr && mr_current_handle() != nullptr && mr_current_handle()->ws != nullptr) {
        int dev_now = -1;                    // the workspace lives on the handle's device: never hand it to a launch on another one
        (void)hipGetDevice(&dev_now);
        MR_CHECK_ARG(dev_now == mr_current_handle()->device, "mr_gemm: the current handle was created for device %d, this thread launches on device %d",
                     mr_current_handle()->device, dev_now);
        with_ws = *a;
        with_ws.workspace = mr_current_handle()->ws;
        with_ws.workspace_bytes = mr_current_handle()->ws_bytes;
        a = &with_ws;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (gemm5_wanted(a)) return route_gemm5(a, s);
    if (gemm3_eligible(a)) return route_pingpong(a, s);
    if (gemm256_eligible(a)) return route_one_barrier(a, s);
    return route_small(a, s);
}

extern "C" int mr_gemm_grouped(const mr_gemm_args* list, int32_t count, void* stream) {
    MR_CHECK_ARG(list != nullptr && count >= 1, "mr_gemm_grouped: empty list");
    for (int k = 0; k < count; ++k) {          // the same operand checks mr_gemm makes, BEFORE any kernel sees the list (16-byte LDS-DMA loads / b128 stores)
        const mr_gemm_args* a = &list[k];
        MR_CHECK_ARG(a->M > 0 && a->N > 0 && a->K > 0, "mr_gemm_grouped: problem %d is empty (M=%ld N=%ld K=%ld)", k, (long)a->M, (long)a->N, (long)a->K);
        MR_CHECK_ARG(a->A && a->B && a->C, "mr_gemm_grouped: problem %d has a null operand", k);
        MR_CHECK_ARG(a->lda % 8 == 0 && a->ldb % 8 == 0, "mr_gemm_grouped: problem %d: lda / ldb must be multiples of 8", k);
        MR_CHECK_ARG(((uintptr_t)a->A % 16) == 0 && ((uintptr_t)a->B % 16) == 0 && ((uintptr_t)a->C % 16) == 0,
                     "mr_gemm_grouped: problem %d: operands must be 16-byte aligned", k);
        MR_CHECK_ARG(a->c_dtype != MR_DT_BF16 || (a->N % 8 == 0 && a->ldc % 8 == 0), "mr_gemm_grouped: problem %d: bf16 output needs N, ldc multiples of 8", k);
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    {
        g3::TNArgs ta;
        int64_t tiles = 0;
        if (tn_group(list, count, ta, &tiles)) {
            mr_gemm3_tn_launch(ta, tiles, s);
            mr_note_route("g3::gemm3_tn_kernel grouped x%d", count);
            MR_CHECK_LAUNCH("mr_gemm_grouped (ping-pong kernel)");
            return MR_OK;
        }
    }
    // small problems of one layout (none of which the big kernels would take): ONE launch of the 128 x 128 kernel over all their tiles
    if (count > 1 && count <= SMALL_MAXG) {
        bool small = true;
        int64_t tiles = 0;
        for (int k = 0; small && k < count; ++k) {
            const mr_gemm_args* a = &list[k];
            small = small_group_member(a, list[0]);
            tiles += ((a->M + SMALL_TILE - 1) / SMALL_TILE) * ((a->N + SMALL_TILE - 1) / SMALL_TILE);
        }
        if (small && tiles <= 4096) {
            mr_gemm_small_grouped_launch(list, count, tiles, s);
            mr_note_route("gemm_bf16_grouped_kernel<%d,%d> x%d", (int)list[0].transA, (int)list[0].transB, count);
            MR_CHECK_LAUNCH("mr_gemm_grouped (small problems)");
            return MR_OK;
        }
    }
    if (count > 4) {        // the one-barrier kernel groups <= 4 problems per launch
        for (int k = 0; k < count; k += 4) {
            const int rc = mr_gemm_grouped(list + k, count - k < 4 ? count - k : 4, stream);
            if (rc != MR_OK) return rc;
        }
        return MR_OK;
    }
    bool all_big = count > 1;
    for (int k = 0; all_big && k < count; ++k) all_big = list[k].M > 0 && list[k].N % 128 == 0;     // (256-wide tiles: N % 256, checked inside)
    if (all_big && route_one_barrier_group(list, count, s)) {
        MR_CHECK_LAUNCH("mr_gemm_grouped");
        return MR_OK;
    }
    for (int k = 0; k < count; ++k) {          // not groupable: one launch per problem (identical results)
        const int rc = mr_gemm(&list[k], stream);
        if (rc != MR_OK) return rc;
    }
    return MR_OK;
}
