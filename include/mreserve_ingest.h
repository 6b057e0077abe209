/* libmreserve_ingest.so: decoded media as decoders hand it out -> what the media front end takes, for AMD gfx950 (MI355X).
 *
 * The two steps the reference leaves to ffmpeg and numpy before any frame or sample reaches its preprocessing (mreserve/preprocess.py:34-59,
 * 115-118, 216-217, 290-291):
 *   PCM of any integer rate / channel layout -> mono fp32 at 22050 Hz, and its peak   (mri_resample_mono)
 *   uint8 frames -> the bounding rows / columns of everything that is not black bar    (mri_content_bounds)
 * File decoding (ffmpeg) is not here.
 *
 * Conventions, as in mreserve_media.h:
 *  - extern "C", plain pointers and sizes.  The library shares no handle, option or symbol with the other three libraries.
 *  - Every launching function takes a `void* stream` (a hipStream_t; NULL = default stream) and returns 0 on success, a negative
 *    MRI_E* code otherwise; mri_last_error() returns a thread-local description.
 *  - Caller-owned buffers, no allocation inside; all pointers are device pointers.  Arguments are validated before any launch.
 */
#ifndef MRESERVE_INGEST_H
#define MRESERVE_INGEST_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MRI_OK 0
#define MRI_EINVAL (-1)   /* bad argument / unsupported shape */
#define MRI_ELAUNCH (-2)  /* HIP launch error */

#define MRI_DT_S16 0      /* int16 samples */
#define MRI_DT_F32 1      /* fp32 samples */

#define MRI_SR 22050      /* the output rate */

int mri_version(void);
const char* mri_last_error(void);

/* Output samples of N input samples resampled by L / M: ceil(N L / M); <= 0 for N, L or M < 1 or a product past 2^62. */
int64_t mri_resample_len(int64_t N, int64_t L, int64_t M);

/* Downmix + polyphase resampling by L / M (L = 22050 / g, M = sr_in / g, g = gcd(sr_in, 22050)) + peak, one launch.
 *   x          int16 (MRI_DT_S16) or fp32 (MRI_DT_F32) samples, C channels of N samples, sample i of channel c at x[c ch_stride + i sample_stride]
 *              (strides in elements): planar [C, N] is (N, 1), interleaved [N, C] is (1, C)
 *   m[i]       = (x[0, i] + x[1, i] + ... in fp32, channel order) / C          a true division; m[i] = 0 outside [0, N)
 *   taps       fp32 [L, K] host-made polyphase filter, K = 2 half; row p serves the outputs n with n mod L = p
 *   y[n]       = sum_j taps[n mod L, j] m[floor(n M / L) + j - half + 1]        fmaf in ascending j from 0; n = 0 .. mri_resample_len(N, L, M) - 1
 *   peak       uint32, zeroed by the caller: the bit pattern of max_n |y[n]| (an integer maximum of the patterns: the order of arrival does not
 *              matter; a NaN in the input leaves a NaN pattern here, nothing else is done about it)
 * An output's bits do not depend on N_out, on the grid or on which workgroup computes it.  The index n M is 64-bit.
 * MRI_EINVAL for a null pointer, N, C, L or M < 1, K < 2 or odd, an unknown dtype, a zero stride, or a ratio M / L with K so large that 64 outputs'
 * input span does not fit the 48 KB staging buffer (rates past ~ 2.8 MHz). */
int mri_resample_mono(const void* x, int32_t dtype, int64_t C, int64_t N, int64_t ch_stride, int64_t sample_stride, const float* taps,
                      int64_t L, int64_t M, int64_t K, float* y, uint32_t* peak, void* stream);

/* The reduction of _detect_black_bars_from_video: frames uint8 [n, H, W, 3] contiguous, has_content(y, x) = any frame, any channel >= threshold.
 *   bounds     int32 [4] = {first row, last row, first column, last column} with content, initialised by the caller to {H, -1, W, -1} (what an
 *              all-dark stack leaves); integer atomic minima / maxima.
 * MRI_EINVAL for a null pointer, n, H or W < 1, H W 3 >= 2^30, or a threshold outside 0 .. 255. */
int mri_content_bounds(const uint8_t* frames, int64_t n, int64_t H, int64_t W, int32_t threshold, int32_t* bounds, void* stream);

#ifdef __cplusplus
}
#endif
#endif
