// libmreserve_zeroshot.so (include/mreserve_zeroshot.h): the zero-shot head for gfx950 -- scale * queries @ labels^T, log-sum-exp, top-k and the
// group marginal in two launches, without the [Q, L] logits ever reaching HBM unless the caller asks for them.
//
//   score_slice_kernel  One workgroup = 16 queries x one slice of MRZ_SLICE = 512 labels, 4 waves.  The product runs on v_mfma_f32_16x16x4_f32
//                       (exact fp32, bf16 operands widened on the way in, never the other way round), output-stationary: a wave owns 8 blocks of
//                       16 labels, and a lane reads 4 consecutive h of its query row and of its 8 label rows per step (16-byte loads; which 4 h
//                       share an MFMA is a permutation of the sum both operands agree on).  The 16 x 512 scaled logits go to LDS.  Then a wave
//                       per query: the slice's (max, sum-exp) pair, and the slice's k best by k rounds of a wave-wide max over the 64-bit key
//                           (order-preserving bits of the logit << 32) | (0xFFFFFFFF - label index)
//                       -- value descending, then lower index, in one integer compare; the keys of a row are distinct, so a round removes exactly
//                       one.  Group maxima are integer atomic maxima of the same key into the workspace: order-independent, hence deterministic.
//   merge_kernel        One wave per query: the k best of the slices' lists (the same selection, streamed 448 keys at a time beside the running
//                       list), the (max, sum-exp) pairs combined in slice order, and the k best groups out of the G group keys.
// With one slice the first kernel writes the results itself; without groups the second launch is skipped.  Nothing depends on Q or on the
// number of CUs: a row's bits are the same in any batch.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/mreserve_zeroshot.h"

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef unsigned long long u64;

static thread_local char g_err[512] = "";

static void mrz_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

#define MRZ_CHECK_ARG(cond, ...)           \
    do {                                   \
        if (!(cond)) {                     \
            mrz_set_error(__VA_ARGS__);    \
            return MRZ_EINVAL;             \
        }                                  \
    } while (0)

namespace {

constexpr int SLICE = MRZ_SLICE;             // labels per workgroup
constexpr int QT = 16;                       // queries per workgroup = the M of one MFMA
constexpr int BPW = SLICE / 4 / 16;          // 8 blocks of 16 labels per wave
constexpr int LDP = SLICE + 4;               // LDS row stride in floats: rows 4 g + r of the accumulator layout land 16 banks apart
constexpr int KPL = SLICE / 64;              // 8 keys per lane in a selection
constexpr int STREAM = (KPL - 1) * 64;       // 448 new keys per pass of the streamed selection (one register holds the running list)
static_assert(SLICE % 64 == 0 && BPW * 64 == SLICE && MRZ_MAX_K <= 64, "one rank per lane, whole blocks per wave");
static_assert(QT * LDP * 4 <= 65536, "static LDS");

struct bf16_t { uint16_t bits; };            // storage only: widened to fp32 by a shift

__device__ __forceinline__ f32x4 load4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ f32x4 load4(const bf16_t* p) {
    const uint2 u = *reinterpret_cast<const uint2*>(p);
    return f32x4{__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16), __uint_as_float(u.y & 0xffff0000u)};
}

// value descending, then lower index: one unsigned compare.  A key is never 0 (index < 2^24), so 0 means "nothing here"
__device__ __forceinline__ u64 make_key(float v, uint32_t index) {
    const uint32_t b = __float_as_uint(v);
    const uint32_t u = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ((u64)u << 32) | (u64)(0xFFFFFFFFu - index);
}
__device__ __forceinline__ void split_key(u64 key, float& v, int32_t& index) {
    if (key == 0) {
        v = -INFINITY;
        index = -1;
        return;
    }
    const uint32_t u = (uint32_t)(key >> 32);
    v = __uint_as_float((u & 0x80000000u) ? (u ^ 0x80000000u) : ~u);
    index = (int32_t)(0xFFFFFFFFu - (uint32_t)key);
}

// butterflies: every lane ends with the same bits (a + b == b + a), in an order that depends on nothing
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = v + __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ u64 wave_max(u64 v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const u64 t = __shfl_xor(v, o);
        v = t > v ? t : v;
    }
    return v;
}

// the k largest of the wave's 64 x KPL keys: lane r returns rank r (0 when fewer than r + 1 non-zero keys exist).  Destroys `key`.
__device__ __forceinline__ u64 wave_select(u64 (&key)[KPL], int k, int lane) {
    u64 mine = 0;
    for (int r = 0; r < k; ++r) {
        u64 best = key[0];
#pragma unroll
        for (int j = 1; j < KPL; ++j) best = key[j] > best ? key[j] : best;
        best = wave_max(best);
        if (best == 0) break;                // wave-uniform
#pragma unroll
        for (int j = 0; j < KPL; ++j) key[j] = key[j] == best ? 0 : key[j];
        mine = lane == r ? best : mine;
    }
    return mine;
}

// the k largest of src[0 .. n): the running list rides in register 0 of every pass
__device__ __forceinline__ u64 wave_select_stream(const u64* __restrict__ src, int64_t n, int k, int lane) {
    u64 run = 0;
    for (int64_t base = 0; base < n; base += STREAM) {
        u64 key[KPL];
        key[0] = run;
#pragma unroll
        for (int j = 1; j < KPL; ++j) {
            const int64_t i = base + (j - 1) * 64 + lane;
            key[j] = i < n ? src[i] : 0;
        }
        run = wave_select(key, k, lane);
    }
    return run;
}

template <typename TQ, typename TL>
__global__ __launch_bounds__(256) void score_slice_kernel(const TQ* __restrict__ queries, int64_t ldq, const TL* __restrict__ labels, int64_t ldl,
                                                          int64_t Q, int L, int H, float scale, int k, int nslices, float* __restrict__ top_val,
                                                          int32_t* __restrict__ top_idx, float* __restrict__ lse, float* __restrict__ logits,
                                                          const int32_t* __restrict__ groups, int G, u64* __restrict__ part_keys,
                                                          float2* __restrict__ part_ms, u64* __restrict__ gkeys) {
    __shared__ __attribute__((aligned(16))) float S[QT * LDP];
    const int tid = threadIdx.x, lane = tid & 63, wave_id = tid >> 6;
    const int g = lane >> 4, li = lane & 15;
    const int64_t q0 = (int64_t)blockIdx.x * QT;
    const int slice = blockIdx.y, l0 = slice * SLICE;
    // rows past the ends are clamped (their logits are never read as valid); blocks wholly past L are skipped, wave-uniformly
    const int wl0 = l0 + wave_id * (SLICE / 4);
    const int nblk = min(max((L - wl0 + 15) / 16, 0), BPW);
    const int64_t qrow = min(q0 + li, Q - 1);
    const TQ* qa = queries + qrow * ldq + 4 * g;
    const TL* lb[BPW];
#pragma unroll
    for (int b = 0; b < BPW; ++b) lb[b] = labels + (int64_t)min(wl0 + 16 * b + li, L - 1) * ldl + 4 * g;
    f32x4 acc[BPW];
#pragma unroll
    for (int b = 0; b < BPW; ++b) acc[b] = f32x4{0.f, 0.f, 0.f, 0.f};
    // step h: lane (g, li) holds h + 4 g + c, c = 0 .. 3, of its rows; MFMA c sums the four h + 4 g' + c
    for (int h = 0; h < H; h += 16) {
        const f32x4 a = load4(qa + h);
#pragma unroll
        for (int b = 0; b < BPW; ++b) {
            if (b < nblk) {
                const f32x4 bv = load4(lb[b] + h);
                acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0], bv[0], acc[b], 0, 0, 0);
                acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1], bv[1], acc[b], 0, 0, 0);
                acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[2], bv[2], acc[b], 0, 0, 0);
                acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[3], bv[3], acc[b], 0, 0, 0);
            }
        }
    }
    // accumulator layout: label 16 b + (lane & 15), queries 4 (lane >> 4) + r.  One multiply; + 0 turns -0 into +0
#pragma unroll
    for (int b = 0; b < BPW; ++b) {
        if (b < nblk) {
            const int c = wave_id * (SLICE / 4) + 16 * b + li;
            S[(4 * g + 0) * LDP + c] = scale * acc[b][0] + 0.f;
            S[(4 * g + 1) * LDP + c] = scale * acc[b][1] + 0.f;
            S[(4 * g + 2) * LDP + c] = scale * acc[b][2] + 0.f;
            S[(4 * g + 3) * LDP + c] = scale * acc[b][3] + 0.f;
        }
    }
    __syncthreads();
    if (logits) {
        for (int e = tid; e < QT * SLICE; e += 256) {
            const int qi = e / SLICE, c = e % SLICE;
            if (q0 + qi < Q && l0 + c < L) logits[(q0 + qi) * (int64_t)L + l0 + c] = S[qi * LDP + c];
        }
    }
    for (int qi = wave_id; qi < QT; qi += 4) {
        const int64_t q = q0 + qi;
        if (q >= Q) break;                   // wave-uniform
        const float* row = S + qi * LDP;
        float v[KPL];
        float m = -INFINITY;
#pragma unroll
        for (int j = 0; j < KPL; ++j) {
            const int c = lane + 64 * j;
            v[j] = l0 + c < L ? row[c] : -INFINITY;
            m = fmaxf(m, v[j]);
        }
        m = wave_max(m);
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < KPL; ++j) s += l0 + lane + 64 * j < L ? expf(v[j] - m) : 0.f;
        s = wave_sum(s);
        u64 key[KPL];
#pragma unroll
        for (int j = 0; j < KPL; ++j) {
            const int l = l0 + lane + 64 * j;
            key[j] = l < L ? make_key(v[j], (uint32_t)l) : 0;
        }
        if (groups) {
#pragma unroll
            for (int j = 0; j < KPL; ++j) {
                const int l = l0 + lane + 64 * j;
                if (l < L) {
                    const int gid = groups[l];
                    if ((unsigned)gid < (unsigned)G) atomicMax(gkeys + q * (int64_t)G + gid, key[j]);
                }
            }
        }
        const u64 mine = wave_select(key, k, lane);
        if (nslices == 1) {
            if (lane < k) {
                float tv;
                int32_t ti;
                split_key(mine, tv, ti);
                top_val[q * k + lane] = tv;
                top_idx[q * k + lane] = ti;
            }
            if (lane == 0) lse[q] = m + logf(s);
        } else {
            if (lane < k) part_keys[(q * nslices + slice) * k + lane] = mine;
            if (lane == 0) part_ms[q * nslices + slice] = make_float2(m, s);
        }
    }
}

__global__ __launch_bounds__(64) void merge_kernel(int L, int k, int nslices, float* __restrict__ top_val, int32_t* __restrict__ top_idx,
                                                   float* __restrict__ lse, const int32_t* __restrict__ groups, int G,
                                                   float* __restrict__ gtop_val, int32_t* __restrict__ gtop_group, int32_t* __restrict__ gtop_label,
                                                   const u64* __restrict__ part_keys, const float2* __restrict__ part_ms,
                                                   const u64* __restrict__ gkeys) {
    const int lane = threadIdx.x;
    const int64_t q = blockIdx.x;
    if (nslices > 1) {
        const u64 mine = wave_select_stream(part_keys + q * nslices * k, (int64_t)nslices * k, k, lane);
        if (lane < k) {
            float tv;
            int32_t ti;
            split_key(mine, tv, ti);
            top_val[q * k + lane] = tv;
            top_idx[q * k + lane] = ti;
        }
        // slices lane, lane + 64, ... per lane in slice order, then the butterfly
        const float2* ms = part_ms + q * nslices;
        float m = -INFINITY;
        for (int i = lane; i < nslices; i += 64) m = fmaxf(m, ms[i].x);
        m = wave_max(m);
        float s = 0.f;
        for (int i = lane; i < nslices; i += 64) s += ms[i].y * expf(ms[i].x - m);
        s = wave_sum(s);
        if (lane == 0) lse[q] = m + logf(s);
    }
    if (groups) {
        const u64 mine = wave_select_stream(gkeys + q * (int64_t)G, G, k, lane);
        if (lane < k) {
            float tv;
            int32_t ti;
            split_key(mine, tv, ti);
            gtop_val[q * k + lane] = tv;
            gtop_label[q * k + lane] = ti;
            gtop_group[q * k + lane] = ti >= 0 ? groups[ti] : -1;
        }
    }
}

bool sizes_ok(const char* fn, int64_t Q, int64_t L, int64_t G, int64_t k) {
    if (!(Q >= 1 && Q < (1LL << 31) - 16)) {
        mrz_set_error("%s: Q = %lld outside [1, 2^31 - 16)", fn, (long long)Q);
        return false;
    }
    if (!(L >= 1 && L < (1LL << 24))) {
        mrz_set_error("%s: L = %lld outside [1, 2^24)", fn, (long long)L);
        return false;
    }
    if (!(G >= 0 && G <= L)) {
        mrz_set_error("%s: G = %lld outside [0, L = %lld]", fn, (long long)G, (long long)L);
        return false;
    }
    if (!(k >= 1 && k <= MRZ_MAX_K)) {
        mrz_set_error("%s: k = %lld outside [1, %d]", fn, (long long)k, MRZ_MAX_K);
        return false;
    }
    return true;
}

inline int64_t round16(int64_t n) { return (n + 15) / 16 * 16; }

// the workspace: [Q, nslices, k] keys, [Q, nslices] (max, sum-exp) pairs (both only with more than one slice), [Q, G] group keys
struct Layout {
    int64_t nslices, keys, ms, gkeys, total;
};
Layout layout(int64_t Q, int64_t L, int64_t G, int64_t k) {
    Layout w;
    w.nslices = (L + SLICE - 1) / SLICE;
    const int64_t pk = w.nslices > 1 ? round16(Q * w.nslices * k * 8) : 0, pm = w.nslices > 1 ? round16(Q * w.nslices * 8) : 0;
    w.keys = 0;
    w.ms = pk;
    w.gkeys = pk + pm;
    w.total = pk + pm + (G > 0 ? round16(Q * G * 8) : 0);
    return w;
}

bool row_aligned(const void* p, int64_t ld, int32_t dtype) {
    const int64_t es = dtype == MRZ_DT_F32 ? 4 : 2;
    return (reinterpret_cast<uintptr_t>(p) % 16) == 0 && (ld * es) % 16 == 0;
}

}  // namespace

extern "C" int mrz_version(void) { return 1; }
extern "C" const char* mrz_last_error(void) { return g_err; }

extern "C" int64_t mrz_workspace_bytes(int64_t Q, int64_t L, int64_t G, int64_t k) {
    if (!sizes_ok("mrz_workspace_bytes", Q, L, G, k)) return MRZ_EINVAL;
    return layout(Q, L, G, k).total;
}

extern "C" int mrz_score_topk(const void* queries, int64_t ldq, int32_t q_dtype, const void* labels, int64_t ldl, int32_t l_dtype, int64_t Q,
                              int64_t L, int64_t H, float scale, int64_t k, float* top_val, int32_t* top_idx, float* lse, float* logits_or_null,
                              const int32_t* groups_or_null, int64_t G, float* gtop_val, int32_t* gtop_group, int32_t* gtop_label,
                              void* workspace, void* stream) {
    const char* fn = "mrz_score_topk";
    MRZ_CHECK_ARG(queries && labels && top_val && top_idx && lse, "%s: null pointer (queries, labels, top_val, top_idx and lse are required)", fn);
    MRZ_CHECK_ARG((q_dtype == MRZ_DT_F32 || q_dtype == MRZ_DT_BF16) && (l_dtype == MRZ_DT_F32 || l_dtype == MRZ_DT_BF16),
                  "%s: dtypes must be MRZ_DT_F32 or MRZ_DT_BF16, got %d / %d", fn, (int)q_dtype, (int)l_dtype);
    if (!groups_or_null) G = 0;
    if (!sizes_ok(fn, Q, L, G, k)) return MRZ_EINVAL;
    MRZ_CHECK_ARG(H >= 64 && H <= MRZ_MAX_H && H % 64 == 0, "%s: H = %lld must be a multiple of 64 in [64, %d]", fn, (long long)H, MRZ_MAX_H);
    MRZ_CHECK_ARG(ldq >= H && ldl >= H, "%s: row stride %lld / %lld < H = %lld", fn, (long long)ldq, (long long)ldl, (long long)H);
    MRZ_CHECK_ARG(row_aligned(queries, ldq, q_dtype) && row_aligned(labels, ldl, l_dtype), "%s: rows must be 16-byte aligned (base and stride)", fn);
    if (groups_or_null) {
        MRZ_CHECK_ARG(G >= 1, "%s: G = %lld with groups given; need 1 <= G <= L", fn, (long long)G);
        MRZ_CHECK_ARG(gtop_val && gtop_group && gtop_label, "%s: null pointer (the three group outputs are required with groups)", fn);
    }
    const Layout w = layout(Q, L, G, k);
    MRZ_CHECK_ARG(w.total == 0 || workspace, "%s: null pointer (workspace of %lld bytes required)", fn, (long long)w.total);
    MRZ_CHECK_ARG(reinterpret_cast<uintptr_t>(workspace) % 16 == 0, "%s: workspace must be 16-byte aligned", fn);
    char* ws = static_cast<char*>(workspace);
    u64* part_keys = w.nslices > 1 ? reinterpret_cast<u64*>(ws + w.keys) : nullptr;
    float2* part_ms = w.nslices > 1 ? reinterpret_cast<float2*>(ws + w.ms) : nullptr;
    u64* gkeys = G > 0 ? reinterpret_cast<u64*>(ws + w.gkeys) : nullptr;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (gkeys) {
        hipError_t e = hipMemsetAsync(gkeys, 0, (size_t)(Q * G * 8), st);
        if (e != hipSuccess) {
            mrz_set_error("%s: clearing the group keys failed: %s", fn, hipGetErrorString(e));
            return MRZ_ELAUNCH;
        }
    }
    const dim3 grid((unsigned)((Q + QT - 1) / QT), (unsigned)w.nslices);
#define MRZ_LAUNCH(TQ, TL)                                                                                                                         \
    hipLaunchKernelGGL((score_slice_kernel<TQ, TL>), grid, dim3(256), 0, st, static_cast<const TQ*>(queries), ldq, static_cast<const TL*>(labels), \
                       ldl, Q, (int)L, (int)H, scale, (int)k, (int)w.nslices, top_val, top_idx, lse, logits_or_null, groups_or_null, (int)G,       \
                       part_keys, part_ms, gkeys)
    if (q_dtype == MRZ_DT_F32 && l_dtype == MRZ_DT_F32)
        MRZ_LAUNCH(float, float);
    else if (q_dtype == MRZ_DT_F32)
        MRZ_LAUNCH(float, bf16_t);
    else if (l_dtype == MRZ_DT_F32)
        MRZ_LAUNCH(bf16_t, float);
    else
        MRZ_LAUNCH(bf16_t, bf16_t);
#undef MRZ_LAUNCH
    if (w.nslices > 1 || G > 0)
        hipLaunchKernelGGL(merge_kernel, dim3((unsigned)Q), dim3(64), 0, st, (int)L, (int)k, (int)w.nslices, top_val, top_idx, lse, groups_or_null,
                           (int)G, gtop_val, gtop_group, gtop_label, part_keys, part_ms, gkeys);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        mrz_set_error("%s: launch failed: %s", fn, hipGetErrorString(e));
        return MRZ_ELAUNCH;
    }
    return MRZ_OK;
}
