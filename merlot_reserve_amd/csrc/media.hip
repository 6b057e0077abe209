// libmreserve_media.so (include/mreserve_media.h): the media front end of the zero-shot surface for gfx950.
//
//   logmel_kernel   waveform -> [T, 65] log-mel rows.  One workgroup = 16 frames of one waveform, 4 waves.  The DFT is the matrix product
//                   frames [16, 1536] x twiddle [1536, 2 x 769] on v_mfma_f32_16x16x4_f32 (exact fp32, an fmaf chain in n order), output-stationary:
//                   the 49 blocks of 16 bins are dealt round-robin to the waves (13 per wave, re and im: 26 accumulators, more than the two the
//                   40-cycle dependent latency asks for), and the windowed frames stream through LDS 64 samples at a time -- padded (numpy
//                   'reflect'), framed and windowed on the way in, so neither the frame matrix nor the spectrum ever exists in HBM.  The B operand
//                   is a gather from the 1536-entry cos / sin tables (LDS) at the integer (n k) mod 1536, which every lane keeps incrementally
//                   (+ 4 k mod 1536 per k-step); no sinf / cosf of a growing angle.  The power spectrum goes to LDS k-major (over the twiddle and
//                   frame buffers, dead by then) and feeds the [16, 769] x [769, 64] mel product, one 16-mel block per wave; log in the epilogue.
//   patches_kernel  uint8 frames -> resized / padded / patchified rows in one pass: a thread per output pixel, host-made tap tables, each output
//                   element written once at its patch position.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/mreserve_media.h"

typedef __attribute__((ext_vector_type(4))) float f32x4;

static thread_local char g_err[512] = "";

static void mrm_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

#define MRM_CHECK_ARG(cond, ...)           \
    do {                                   \
        if (!(cond)) {                     \
            mrm_set_error(__VA_ARGS__);    \
            return MRM_EINVAL;             \
        }                                  \
    } while (0)

#define MRM_CHECK_LAUNCH(name)                                                    \
    do {                                                                          \
        hipError_t e__ = hipGetLastError();                                       \
        if (e__ != hipSuccess) {                                                  \
            mrm_set_error("%s: launch failed: %s", name, hipGetErrorString(e__)); \
            return MRM_ELAUNCH;                                                   \
        }                                                                         \
    } while (0)

namespace {

constexpr int NFFT = MRM_NFFT, HOP = MRM_HOP, NBINS = MRM_NBINS, NMELS = MRM_NMELS;
constexpr int FR = 16;                       // frames per workgroup = the M of one MFMA
constexpr int NC = 64;                       // samples per LDS chunk
constexpr int NCHUNK = NFFT / NC;            // 24
constexpr int NBLK = (NBINS + 15) / 16;      // 49 blocks of 16 bins (784: bins 769 .. 783 are computed and dropped)
constexpr int BPW = (NBLK + 3) / 4;          // 13 bin blocks per wave (block = wave + 4 j; a block >= 49 is computed and dropped)
constexpr int KPAD = NBLK * 16;              // 784
constexpr int LDS_TW = 2 * NFFT;             // floats: cos, sin
constexpr int LDS_FR = 2 * NC * FR;          // floats: two chunk buffers [n][frame]
constexpr int LDS_S = KPAD * FR;             // floats: power spectrum [bin][frame]
constexpr int LDS_FLOATS = LDS_S > LDS_TW + LDS_FR ? LDS_S : LDS_TW + LDS_FR;
static_assert(NFFT % NC == 0 && NC % 4 == 0 && NC * FR == 4 * 256, "chunk geometry: four elements per thread");
static_assert(LDS_FLOATS * 4 <= 65536, "static LDS");

template <typename T> __device__ __forceinline__ void store_out(T* p, float v);
template <> __device__ __forceinline__ void store_out<float>(float* p, float v) { *p = v; }
template <> __device__ __forceinline__ void store_out<__bf16>(__bf16* p, float v) { *p = (__bf16)v; }       // round to nearest even

// sample n of frame t of a waveform of L samples: p[588 t + n] of the reflect-padded signal.  L >= 769 keeps both reflections inside [0, L)
__device__ __forceinline__ float frame_sample(const float* __restrict__ w, int64_t L, int64_t t, int n) {
    int64_t i = t * HOP + n - NFFT / 2;
    if (i < 0) i = -i;
    if (i >= L) i = 2 * (L - 1) - i;
    return w[i];
}

template <typename T>
__global__ __launch_bounds__(256) void logmel_kernel(const float* __restrict__ wave, int64_t ldw, int64_t L, int64_t nframes,
                                                     const float* __restrict__ window, const float* __restrict__ twiddle,
                                                     const float* __restrict__ fb, float speed, float eps, T* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float smem[LDS_FLOATS];
    float* tw = smem;                        // [2][1536]
    float* fr = smem + LDS_TW;               // [2][NC][FR]
    float* Ss = smem;                        // [KPAD][FR], after the DFT
    const int tid = threadIdx.x, lane = tid & 63, wave_id = tid >> 6;
    const int g = lane >> 4, li = lane & 15;
    const int64_t t0 = (int64_t)blockIdx.x * FR;
    const float* w = wave + (int64_t)blockIdx.y * ldw;

    for (int i = tid; i < LDS_TW; i += 256) tw[i] = twiddle[i];

    // staging: element e = tid + 256 q of a chunk is (frame e >> 6, sample e & 63): coalesced reads along the waveform
    const int s_row = tid >> 6, s_n = tid & 63;          // frames s_row + 4 q
    float pre[4];
    auto load_chunk = [&](int c) {
        const int n = c * NC + s_n;
        const float wn = window[n];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t t = t0 + s_row + 4 * q;
            pre[q] = t < nframes ? frame_sample(w, L, t, n) * wn : 0.f;
        }
    };
    auto store_chunk = [&](int buf) {
#pragma unroll
        for (int q = 0; q < 4; ++q) fr[(buf * NC + s_n) * FR + s_row + 4 * q] = pre[q];
    };

    // this lane's twiddle index (n k) mod 1536 per bin block, n = 4 s + g, and its step 4 k mod 1536
    int idx[BPW], step[BPW];
#pragma unroll
    for (int j = 0; j < BPW; ++j) {
        const int k = 16 * (wave_id + 4 * j) + li;
        idx[j] = (g * k) % NFFT;
        step[j] = (4 * k) % NFFT;
    }
    f32x4 re[BPW], im[BPW];
#pragma unroll
    for (int j = 0; j < BPW; ++j) { re[j] = f32x4{0.f, 0.f, 0.f, 0.f}; im[j] = f32x4{0.f, 0.f, 0.f, 0.f}; }

    load_chunk(0);
    store_chunk(0);
    __syncthreads();
    for (int c = 0; c < NCHUNK; ++c) {
        const int buf = c & 1;
        const bool more = c + 1 < NCHUNK;
        if (more) load_chunk(c + 1);
        const float* As = fr + buf * NC * FR;
        for (int s = 0; s < NC / 4; ++s) {
            const float a = As[(4 * s + g) * FR + li];
#pragma unroll
            for (int j = 0; j < BPW; ++j) {
                const float bc = tw[idx[j]], bs = tw[NFFT + idx[j]];
                re[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bc, re[j], 0, 0, 0);
                im[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bs, im[j], 0, 0, 0);
                const int nx = idx[j] + step[j];
                idx[j] = nx >= NFFT ? nx - NFFT : nx;
            }
        }
        if (more) store_chunk(buf ^ 1);      // the other buffer was last read before the previous barrier
        __syncthreads();
    }
    // every wave is past its last twiddle / frame read (the barrier above): the power spectrum takes their place, [bin][frame].
    // accumulator layout: bin = 16 block + (lane & 15), frames 4 (lane >> 4) + r
#pragma unroll
    for (int j = 0; j < BPW; ++j) {
        const int blk = wave_id + 4 * j;
        if (blk < NBLK) {
            const int k = 16 * blk + li;
            f32x4 p = re[j] * re[j] + im[j] * im[j];
            if (k >= NBINS) p = f32x4{0.f, 0.f, 0.f, 0.f};
            *reinterpret_cast<f32x4*>(Ss + k * FR + 4 * g) = p;
        }
    }
    __syncthreads();
    // mel[frame, m] = sum_k S[frame, k] fb[m, k]: A = S (lane: frame li, k = 4 s + g), B = fb^T (lane: k = 4 s + g, mel 16 wave + li)
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const float* fbr = fb + (int64_t)(16 * wave_id + li) * NBINS;
    for (int s = 0; s < KPAD / 4; ++s) {
        const int k = 4 * s + g;
        const float b = k < NBINS ? fbr[k] : 0.f;
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(Ss[k * FR + li], b, acc, 0, 0, 0);
    }
    // the same logf evaluates both terms, so silence is exactly 0
    const float l0 = logf(eps);
    T* o = out + ((int64_t)blockIdx.y * nframes + t0) * (NMELS + 1);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int f = 4 * g + r;
        if (t0 + f < nframes) store_out(o + (int64_t)f * (NMELS + 1) + 16 * wave_id + li, logf(acc[r] + eps) - l0);
    }
    if (tid < FR && t0 + tid < nframes) store_out(o + (int64_t)tid * (NMELS + 1) + NMELS, speed);
}

template <typename T>
__global__ __launch_bounds__(256) void patches_kernel(const uint8_t* __restrict__ frames, int64_t npix, int H, int W, int dh, int dw,
                                                      const int32_t* __restrict__ yrange, const float* __restrict__ yweights, int ky,
                                                      const int32_t* __restrict__ xrange, const float* __restrict__ xweights, int kx,
                                                      T* __restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    const int x = (int)(p % dw);
    const int y = (int)((p / dw) % dh);
    const int64_t b = p / ((int64_t)dw * dh);
    const int y0 = yrange[2 * y], ny = min(yrange[2 * y + 1], ky);
    const int x0 = xrange[2 * x], nx = min(xrange[2 * x + 1], kx);
    const uint8_t* img = frames + b * (int64_t)H * W * 3;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int ty = 0; ty < ny; ++ty) {
        const int jy = min(max(y0 + ty, 0), H - 1);
        const uint8_t* row = img + (int64_t)jy * W * 3;
        float r0 = 0.f, r1 = 0.f, r2 = 0.f;
        for (int tx = 0; tx < nx; ++tx) {
            const int jx = min(max(x0 + tx, 0), W - 1);
            const float wx = xweights[x * kx + tx];
            const uint8_t* px = row + 3 * jx;
            r0 = fmaf(wx, (float)px[0], r0);
            r1 = fmaf(wx, (float)px[1], r1);
            r2 = fmaf(wx, (float)px[2], r2);
        }
        const float wy = yweights[y * ky + ty];
        a0 = fmaf(wy, r0, a0);
        a1 = fmaf(wy, r1, a1);
        a2 = fmaf(wy, r2, a2);
    }
    // patch (y / 16, x / 16), element ((y % 16) 16 + x % 16) 3 + c
    constexpr int P = MRM_PATCH;
    const int w1 = dw / P;
    T* o = out + ((b * (dh / P) + y / P) * w1 + x / P) * (int64_t)(P * P * 3) + ((y % P) * P + x % P) * 3;
    store_out(o, fminf(fmaxf(a0, 0.f), 255.f) / 255.f);
    store_out(o + 1, fminf(fmaxf(a1, 0.f), 255.f) / 255.f);
    store_out(o + 2, fminf(fmaxf(a2, 0.f), 255.f) / 255.f);
}

}  // namespace

extern "C" int mrm_version(void) { return 1; }
extern "C" const char* mrm_last_error(void) { return g_err; }

extern "C" int64_t mrm_logmel_frames(int64_t L) { return L < NBINS ? 0 : 1 + L / HOP; }

extern "C" int mrm_logmel(const float* wave, int64_t ldw, int64_t n, int64_t L, const float* window, const float* twiddle, const float* fb,
                          float playback_speed, void* out, int32_t out_dtype, void* stream) {
    MRM_CHECK_ARG(wave && window && twiddle && fb && out, "mrm_logmel: null pointer");
    MRM_CHECK_ARG(out_dtype == MRM_DT_F32 || out_dtype == MRM_DT_BF16, "mrm_logmel: out_dtype must be MRM_DT_F32 or MRM_DT_BF16, got %d", (int)out_dtype);
    MRM_CHECK_ARG(L >= NBINS, "mrm_logmel: L = %lld; reflect padding by %d needs L >= %d", (long long)L, NFFT / 2, NBINS);
    MRM_CHECK_ARG(n > 0 && n <= 65535, "mrm_logmel: n = %lld outside [1, 65535]", (long long)n);
    MRM_CHECK_ARG(ldw >= L, "mrm_logmel: row stride %lld < L = %lld", (long long)ldw, (long long)L);
    const int64_t T = 1 + L / HOP;
    MRM_CHECK_ARG((T + FR - 1) / FR < (1LL << 31), "mrm_logmel: too many frames");
    const dim3 grid((unsigned)((T + FR - 1) / FR), (unsigned)n);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (out_dtype == MRM_DT_F32)
        hipLaunchKernelGGL(logmel_kernel<float>, grid, dim3(256), 0, st, wave, ldw, L, T, window, twiddle, fb, playback_speed, 0.1f, static_cast<float*>(out));
    else
        hipLaunchKernelGGL(logmel_kernel<__bf16>, grid, dim3(256), 0, st, wave, ldw, L, T, window, twiddle, fb, playback_speed, 0.1f, static_cast<__bf16*>(out));
    MRM_CHECK_LAUNCH("mrm_logmel");
    return MRM_OK;
}

extern "C" int mrm_frames_to_patches(const uint8_t* frames, int64_t n, int64_t H, int64_t W, int64_t dh, int64_t dw, const int32_t* yrange,
                                     const float* yweights, int64_t ky, const int32_t* xrange, const float* xweights, int64_t kx, void* out,
                                     int32_t out_dtype, void* stream) {
    MRM_CHECK_ARG(frames && yrange && yweights && xrange && xweights && out, "mrm_frames_to_patches: null pointer");
    MRM_CHECK_ARG(out_dtype == MRM_DT_F32 || out_dtype == MRM_DT_BF16, "mrm_frames_to_patches: out_dtype must be MRM_DT_F32 or MRM_DT_BF16, got %d", (int)out_dtype);
    MRM_CHECK_ARG(n > 0 && H > 0 && W > 0 && H <= 65536 && W <= 65536, "mrm_frames_to_patches: bad frame shape [%lld, %lld, %lld, 3]", (long long)n, (long long)H, (long long)W);
    MRM_CHECK_ARG(dh > 0 && dw > 0 && dh % MRM_PATCH == 0 && dw % MRM_PATCH == 0 && dh <= 65536 && dw <= 65536,
                  "mrm_frames_to_patches: output %lld x %lld must be positive multiples of %d", (long long)dh, (long long)dw, MRM_PATCH);
    MRM_CHECK_ARG(ky >= 1 && kx >= 1 && ky <= 65536 && kx <= 65536, "mrm_frames_to_patches: tap table widths %lld / %lld", (long long)ky, (long long)kx);
    const int64_t npix = n * dh * dw;
    MRM_CHECK_ARG((npix + 255) / 256 < (1LL << 31), "mrm_frames_to_patches: too many output pixels");
    const dim3 grid((unsigned)((npix + 255) / 256));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (out_dtype == MRM_DT_F32)
        hipLaunchKernelGGL(patches_kernel<float>, grid, dim3(256), 0, st, frames, npix, (int)H, (int)W, (int)dh, (int)dw, yrange, yweights, (int)ky,
                           xrange, xweights, (int)kx, static_cast<float*>(out));
    else
        hipLaunchKernelGGL(patches_kernel<__bf16>, grid, dim3(256), 0, st, frames, npix, (int)H, (int)W, (int)dh, (int)dw, yrange, yweights, (int)ky,
                           xrange, xweights, (int)kx, static_cast<__bf16*>(out));
    MRM_CHECK_LAUNCH("mrm_frames_to_patches");
    return MRM_OK;
}
