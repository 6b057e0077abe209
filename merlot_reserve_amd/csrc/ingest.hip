// libmreserve_ingest.so (include/mreserve_ingest.h): decoded media as decoders give it -> what the media front end takes, for gfx950.
//
//   resample_kernel  PCM (int16 / fp32, any channel layout through two strides) -> mono fp32 at 22050 Hz + peak.  One workgroup per block of `bo`
//                    consecutive outputs (the host picks bo <= 1024 so that the block's input span fits SPAN floats of LDS).  The span is
//                    downmixed once into LDS (zero outside [0, N)); a thread then computes outputs tid, tid + 256, ...: its phase row of the host-made
//                    tap table comes through the cache as float2 (rows are K floats, K even), the samples from LDS, one fmaf chain in ascending j --
//                    the same chain over the same values wherever the block boundaries fall.  No transcendental, no float atomic: the peak is an
//                    integer maximum of |y| bit patterns, reduced over the wave and the workgroup before its one atomic (skipped when it cannot raise the peak).
//   bounds_kernel    uint8 frames -> {first row, last row, first column, last column} holding a byte >= threshold.  A pure read: the stack is one
//                    flat byte stream, taken 16 aligned bytes per lane whatever 3 W is; four bytes are compared at once in a 32-bit word, and as
//                    row and column are monotone along a row only the first and last hit of each row segment inside a vector are turned into
//                    coordinates.  Bytes before the first / after the last aligned vector go through a byte path, as does a frame narrower than a
//                    vector.  Reduced over the wave and the workgroup, then at most four integer atomics per workgroup -- only those that can still move a bound.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/mreserve_ingest.h"

static thread_local char g_err[512] = "";

static void mri_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

#define MRI_CHECK_ARG(cond, ...)           \
    do {                                   \
        if (!(cond)) {                     \
            mri_set_error(__VA_ARGS__);    \
            return MRI_EINVAL;             \
        }                                  \
    } while (0)

#define MRI_CHECK_LAUNCH(name)                                                    \
    do {                                                                          \
        hipError_t e__ = hipGetLastError();                                       \
        if (e__ != hipSuccess) {                                                  \
            mri_set_error("%s: launch failed: %s", name, hipGetErrorString(e__)); \
            return MRI_ELAUNCH;                                                   \
        }                                                                         \
    } while (0)

namespace {

constexpr int THREADS = 256;
constexpr int SPAN = 12288;                  // floats of LDS for a block's downmixed input span (48 KB)
constexpr int MAX_BO = 1024, MIN_BO = 64;    // outputs per workgroup
constexpr int UNROLL = 4;                    // 16-byte vectors a lane of the bounds kernel has in flight

__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, o, 64));
    return v;
}
__device__ __forceinline__ int wave_min_i32(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ int wave_max_i32(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}

template <typename T>
__global__ __launch_bounds__(THREADS) void resample_kernel(const T* __restrict__ x, int C, int64_t N, int64_t ch_stride, int64_t sample_stride,
                                                           const float* __restrict__ taps, int64_t L, int64_t M, int K, int bo, int64_t n_out,
                                                           float* __restrict__ y, unsigned* __restrict__ peak) {
    __shared__ float sm[SPAN];
    __shared__ unsigned wmax[THREADS / 64];
    const int tid = threadIdx.x;
    const int half = K >> 1;
    const int64_t n0 = (int64_t)blockIdx.x * bo;
    const int cnt = (int)min((int64_t)bo, n_out - n0);                     // >= 1: the grid is ceil(n_out / bo)
    const int64_t i0 = (n0 * M) / L - half + 1;                           // first input sample of the block's span
    const int len = (int)(((n0 + cnt - 1) * M) / L + half - i0 + 1);      // <= (bo - 1) M / L + 1 + K <= SPAN (checked on the host)
    const float fc = (float)C;
    for (int s = tid; s < len; s += THREADS) {
        const int64_t i = i0 + s;
        float m = 0.f;
        if (i >= 0 && i < N) {
            const T* p = x + i * sample_stride;
            m = (float)p[0];
            for (int c = 1; c < C; ++c) m += (float)p[c * ch_stride];
            m = m / fc;
        }
        sm[s] = m;
    }
    __syncthreads();
    unsigned pk = 0;
    for (int o = tid; o < cnt; o += THREADS) {
        const int64_t n = n0 + o;
        const int64_t q = (n * M) / L;                                    // 64-bit: n M passes 2^31 within minutes of audio
        const int64_t ph = n % L;
        const float2* __restrict__ w = reinterpret_cast<const float2*>(taps + ph * K);
        const float* __restrict__ s = sm + (int)(q - half + 1 - i0);
        float acc = 0.f;
        for (int j = 0; j < half; ++j) {
            const float2 t = w[j];
            acc = fmaf(t.x, s[2 * j], acc);
            acc = fmaf(t.y, s[2 * j + 1], acc);
        }
        y[n] = acc;
        pk = max(pk, __float_as_uint(fabsf(acc)));
    }
    pk = wave_max_u32(pk);
    if ((tid & 63) == 0) wmax[tid >> 6] = pk;
    __syncthreads();
    if (tid == 0) {
        pk = max(max(wmax[0], wmax[1]), max(wmax[2], wmax[3]));
        // the maximum only grows: a workgroup that cannot raise what it reads (however stale) has nothing to add, and most cannot
        if (pk > __hip_atomic_load(peak, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(peak, pk);
    }
}

struct Box {
    int r0, r1, c0, c1;
    __device__ __forceinline__ void add(int r, int ca, int cb) {
        r0 = min(r0, r); r1 = max(r1, r); c0 = min(c0, ca); c1 = max(c1, cb);
    }
};

// bit 7 of every byte of x that is >= the threshold.  k = 0x01010101 (128 - thr) for thr <= 128: the low seven bits carry into bit 7, or bit 7 is
// set already; k = 0x01010101 (256 - thr) above: bit 7 must be set and the low seven bits must carry.  No byte's sum passes 255.
__device__ __forceinline__ unsigned ge_mask(unsigned x, unsigned k, bool low) {
    const unsigned s = (x & 0x7f7f7f7fu) + k;
    return (low ? (s | x) : (s & x)) & 0x80808080u;
}
// the four bit-7 flags of a word -> bits 0 .. 3
__device__ __forceinline__ unsigned pack4(unsigned h) { return ((h >> 7) & 1u) | ((h >> 14) & 2u) | ((h >> 21) & 4u) | ((h >> 28) & 8u); }

// one byte at flat offset f of the stack (head, tail and narrow frames)
__device__ __forceinline__ void byte_hit(Box& b, int64_t f, int fb, int rowb) {
    const int r = (int)(f % fb);
    b.add(r / rowb, (r % rowb) / 3, (r % rowb) / 3);
}

__global__ __launch_bounds__(THREADS) void bounds_kernel(const uint8_t* __restrict__ frames, int64_t total, int head, int64_t nvec, int tail,
                                                         int H, int W, int thr, int stride_mod, int* __restrict__ bounds) {
    __shared__ int red[4][THREADS / 64];
    const int tid = threadIdx.x;
    const int rowb = 3 * W, fb = H * rowb;
    const bool low = thr <= 128;
    const unsigned k = 0x01010101u * (unsigned)(low ? 128 - thr : 256 - thr);
    Box b{H, -1, W, -1};
    if (blockIdx.x == 0 && tid < 32) {                                   // the bytes outside the aligned vectors: at most 15 on either side
        const int64_t f = tid < 16 ? (int64_t)tid : (int64_t)head + 16 * nvec + (tid - 16);
        const bool in = tid < 16 ? tid < head : tid - 16 < tail;
        if (in && frames[f] >= thr) byte_hit(b, f, fb, rowb);
    }
    const uint4* __restrict__ vec = reinterpret_cast<const uint4*>(frames + head);
    const int64_t gid = (int64_t)blockIdx.x * THREADS + tid, gsz = (int64_t)gridDim.x * THREADS;
    int r = gid < nvec ? (int)((head + 16 * gid) % fb) : 0;             // offset of this lane's vector inside its frame, kept incrementally
    for (int64_t v0 = gid; v0 < nvec; v0 += UNROLL * gsz) {
        uint4 d[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {                               // independent loads in flight before the first is looked at
            const int64_t v = v0 + u * gsz;
            d[u] = v < nvec ? vec[v] : uint4{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const int64_t v = v0 + u * gsz;
            unsigned m = pack4(ge_mask(d[u].x, k, low)) | (pack4(ge_mask(d[u].y, k, low)) << 4) | (pack4(ge_mask(d[u].z, k, low)) << 8) |
                         (pack4(ge_mask(d[u].w, k, low)) << 12);
            if (v >= nvec) m = 0;
            if (m) {
                if (rowb >= 16) {
                    // at most one row boundary inside the vector (a frame boundary is one too: the next frame's row 0)
                    const int row = r / rowb, cb = r - row * rowb;
                    const int ka = min(16, rowb - cb);
                    const unsigned ma = m & ((1u << ka) - 1u), mb = m >> ka;
                    if (ma) b.add(row, (cb + __builtin_ctz(ma)) / 3, (cb + 31 - __builtin_clz(ma)) / 3);
                    if (mb) b.add(row + 1 == H ? 0 : row + 1, __builtin_ctz(mb) / 3, (31 - __builtin_clz(mb)) / 3);
                } else {
                    const int64_t f = (int64_t)head + 16 * v;
                    for (int e = 0; e < 16; ++e)
                        if (m & (1u << e)) byte_hit(b, f + e, fb, rowb);
                }
            }
            r += stride_mod;                                             // one grid stride further, modulo the frame
            if (r >= fb) r -= fb;
        }
    }
    b.r0 = wave_min_i32(b.r0); b.r1 = wave_max_i32(b.r1); b.c0 = wave_min_i32(b.c0); b.c1 = wave_max_i32(b.c1);
    if ((tid & 63) == 0) { red[0][tid >> 6] = b.r0; red[1][tid >> 6] = b.r1; red[2][tid >> 6] = b.c0; red[3][tid >> 6] = b.c1; }
    __syncthreads();
    if (tid == 0) {
        const int r0 = min(min(red[0][0], red[0][1]), min(red[0][2], red[0][3])), r1 = max(max(red[1][0], red[1][1]), max(red[1][2], red[1][3]));
        const int c0 = min(min(red[2][0], red[2][1]), min(red[2][2], red[2][3])), c1 = max(max(red[3][0], red[3][1]), max(red[3][2], red[3][3]));
        // a workgroup that saw only bars touches nothing; the others only what they can still improve -- the four values move one way, so a
        // stale read can cost an atomic but never drop one, and 8192 atomics on one cache line would otherwise be most of the kernel's time
        if (r1 >= 0) {
            if (r0 < __hip_atomic_load(bounds + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(bounds + 0, r0);
            if (r1 > __hip_atomic_load(bounds + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(bounds + 1, r1);
            if (c0 < __hip_atomic_load(bounds + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(bounds + 2, c0);
            if (c1 > __hip_atomic_load(bounds + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(bounds + 3, c1);
        }
    }
}

}  // namespace

extern "C" int mri_version(void) { return 1; }
extern "C" const char* mri_last_error(void) { return g_err; }

extern "C" int64_t mri_resample_len(int64_t N, int64_t L, int64_t M) {
    if (N < 1 || L < 1 || M < 1 || N > (1LL << 62) / L) return 0;
    return (N * L + M - 1) / M;
}

extern "C" int mri_resample_mono(const void* x, int32_t dtype, int64_t C, int64_t N, int64_t ch_stride, int64_t sample_stride, const float* taps,
                                 int64_t L, int64_t M, int64_t K, float* y, uint32_t* peak, void* stream) {
    MRI_CHECK_ARG(x && taps && y && peak, "mri_resample_mono: null pointer");
    MRI_CHECK_ARG(dtype == MRI_DT_S16 || dtype == MRI_DT_F32, "mri_resample_mono: dtype must be MRI_DT_S16 or MRI_DT_F32, got %d", (int)dtype);
    MRI_CHECK_ARG(N >= 1 && C >= 1 && C <= 65535, "mri_resample_mono: bad shape, %lld channels of %lld samples", (long long)C, (long long)N);
    MRI_CHECK_ARG(L >= 1 && M >= 1 && L < (1LL << 31) && M < (1LL << 31), "mri_resample_mono: bad ratio L / M = %lld / %lld", (long long)L, (long long)M);
    MRI_CHECK_ARG(K >= 2 && K % 2 == 0 && K <= SPAN, "mri_resample_mono: K = %lld taps per phase must be even and in [2, %d]", (long long)K, SPAN);
    MRI_CHECK_ARG(ch_stride != 0 && sample_stride != 0, "mri_resample_mono: zero stride (%lld, %lld)", (long long)ch_stride, (long long)sample_stride);
    const int64_t n_out = mri_resample_len(N, L, M);
    MRI_CHECK_ARG(n_out >= 1 && n_out < (1LL << 62) / M, "mri_resample_mono: %lld samples by %lld / %lld overflow the 64-bit index", (long long)N, (long long)L, (long long)M);
    int bo = MAX_BO;                         // the largest block whose input span fits the staging buffer
    while (bo >= MIN_BO && ((int64_t)(bo - 1) * M) / L + 1 + K > SPAN) bo >>= 1;
    MRI_CHECK_ARG(bo >= MIN_BO, "mri_resample_mono: ratio %lld / %lld with %lld taps: the span of %d outputs does not fit %d staged samples",
                  (long long)M, (long long)L, (long long)K, MIN_BO, SPAN);
    const int64_t blocks = (n_out + bo - 1) / bo;
    MRI_CHECK_ARG(blocks < (1LL << 31), "mri_resample_mono: too many output samples");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (dtype == MRI_DT_S16)
        hipLaunchKernelGGL(resample_kernel<int16_t>, dim3((unsigned)blocks), dim3(THREADS), 0, st, static_cast<const int16_t*>(x), (int)C, N, ch_stride,
                           sample_stride, taps, L, M, (int)K, bo, n_out, y, peak);
    else
        hipLaunchKernelGGL(resample_kernel<float>, dim3((unsigned)blocks), dim3(THREADS), 0, st, static_cast<const float*>(x), (int)C, N, ch_stride,
                           sample_stride, taps, L, M, (int)K, bo, n_out, y, peak);
    MRI_CHECK_LAUNCH("mri_resample_mono");
    return MRI_OK;
}

extern "C" int mri_content_bounds(const uint8_t* frames, int64_t n, int64_t H, int64_t W, int32_t threshold, int32_t* bounds, void* stream) {
    MRI_CHECK_ARG(frames && bounds, "mri_content_bounds: null pointer");
    MRI_CHECK_ARG(n >= 1 && H >= 1 && W >= 1, "mri_content_bounds: bad frame shape [%lld, %lld, %lld, 3]", (long long)n, (long long)H, (long long)W);
    MRI_CHECK_ARG(H < (1LL << 31) && W < (1LL << 31) && H * W < (1LL << 30) / 3, "mri_content_bounds: a frame of %lld x %lld x 3 bytes passes 2^30", (long long)H, (long long)W);
    MRI_CHECK_ARG(n < (1LL << 62) / (H * W * 3), "mri_content_bounds: too many frames");
    MRI_CHECK_ARG(threshold >= 0 && threshold <= 255, "mri_content_bounds: threshold %d outside 0 .. 255", (int)threshold);
    const int64_t total = n * H * W * 3, fb = H * W * 3;
    const int head = (int)std::min<int64_t>((16 - (reinterpret_cast<uintptr_t>(frames) & 15)) & 15, total);
    const int64_t nvec = (total - head) / 16;
    const int tail = (int)(total - head - 16 * nvec);
    const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>((nvec + THREADS * UNROLL - 1) / (THREADS * UNROLL), 2048));
    const int stride_mod = (int)((16 * blocks * THREADS) % fb);
    hipLaunchKernelGGL(bounds_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, static_cast<hipStream_t>(stream), frames, total, head, nvec, tail, (int)H,
                       (int)W, (int)threshold, stride_mod, bounds);
    MRI_CHECK_LAUNCH("mri_content_bounds");
    return MRI_OK;
}
