/* libmreserve_media.so: the media front end of the zero-shot surface, for AMD gfx950 (MI355X).
 *
 * The two numeric transforms between decoded media and the model's inputs (mreserve/preprocess.py:121-156, 464-481):
 *   waveform   -> log-mel spectrogram rows  [n, T, 65]        (mrm_logmel)
 *   uint8 frame -> resized, padded, patchified [n, h*w, 768]  (mrm_frames_to_patches)
 * written directly in the layout and dtype MerlotReserve.embed_video reads.  File decoding (ffmpeg) is not here.
 *
 * Conventions, as in mreserve_hip.h:
 *  - extern "C", plain pointers and sizes.  The library shares no handle, option or symbol with libmreserve_hip.so.
 *  - Every launching function takes a `void* stream` (a hipStream_t; NULL = default stream) and returns 0 on success, a negative
 *    MRM_E* code otherwise; mrm_last_error() returns a thread-local description.
 *  - Caller-owned buffers, no allocation inside; all pointers are device pointers.  Arguments are validated before any launch.
 */
#ifndef MRESERVE_MEDIA_H
#define MRESERVE_MEDIA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MRM_OK 0
#define MRM_EINVAL (-1)   /* bad argument / unsupported shape */
#define MRM_ELAUNCH (-2)  /* HIP launch error */

#define MRM_DT_BF16 0
#define MRM_DT_F32 1

/* the fixed geometry of the pretraining spectrograms (preprocess.py:130-138) */
#define MRM_NFFT 1536
#define MRM_HOP 588
#define MRM_NBINS 769     /* MRM_NFFT / 2 + 1 */
#define MRM_NMELS 64
#define MRM_PATCH 16

int mrm_version(void);
const char* mrm_last_error(void);

/* Frames per waveform of L samples: 1 + L / MRM_HOP (centred frames); <= 0 for L < MRM_NBINS (reflect padding needs L > MRM_NFFT / 2). */
int64_t mrm_logmel_frames(int64_t L);

/* Batched log-mel: wave fp32 [n, L] (row stride ldw elements) -> out [n, T, 65] contiguous, T = mrm_logmel_frames(L), out_dtype MRM_DT_F32 / MRM_DT_BF16.
 *   p[j]      = wave[reflect(j - 768)]                               numpy 'reflect' padding by MRM_NFFT / 2 on both sides
 *   frame t   = p[588 t : 588 t + 1536] * window
 *   S[t, k]   = |sum_n frame[n] exp(-2 pi i n k / 1536)|^2           k = 0 .. 768
 *   out[t, m] = log(sum_k fb[m, k] S[t, k] + 0.1) - log(0.1)         m = 0 .. 63 (fp32 natural log);    out[t, 64] = playback_speed
 * Host-made fp32 tables: window [1536]; twiddle [2, 1536] = cos(2 pi i / 1536), sin(2 pi i / 1536); fb [64, 769] row-major.  The twiddles are
 * looked up at the integer (n k) mod 1536; both products run on the fp32-input MFMA in a fixed order, one workgroup per 16 frames of one row: a
 * row's result does not depend on n or on the other rows.  MRM_EINVAL for L < 769, ldw < L, a null pointer or an unknown dtype. */
int mrm_logmel(const float* wave, int64_t ldw, int64_t n, int64_t L, const float* window, const float* twiddle, const float* fb,
               float playback_speed, void* out, int32_t out_dtype, void* stream);

/* Batched resize + pad + patchify: frames uint8 [n, H, W, 3] -> out [n, (dh / 16) (dw / 16), 768], patch order (block row, block col) x (dy, dx, c).
 * The separable filter comes as host-made tap tables, per output row y (ytaps) and column x (xtaps):
 *   range [dh, 2] int32 = (first input index, number of taps), weights [dh, ky] fp32 (normalised over the in-range taps)
 *   out(y, x, c) = clip(sum_jy wy sum_jx wx u8[jy, jx, c], 0, 255) / 255           (a true division)
 * An output row / column with zero taps is padding and comes out exactly 0.  Input indices are clamped to the frame.  The bf16 result is the
 * round-to-nearest-even of the fp32 result.  MRM_EINVAL for dh / dw not multiples of 16, ky / kx < 1, a null pointer or an unknown dtype. */
int mrm_frames_to_patches(const uint8_t* frames, int64_t n, int64_t H, int64_t W, int64_t dh, int64_t dw, const int32_t* yrange,
                          const float* yweights, int64_t ky, const int32_t* xrange, const float* xweights, int64_t kx, void* out,
                          int32_t out_dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif
