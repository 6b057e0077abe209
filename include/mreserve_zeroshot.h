/* libmreserve_zeroshot.so: the zero-shot head, for AMD gfx950 (MI355X).
 *
 * What every zero-shot consumer of the reference ends with (demo/demo_video.py:43-50, zero_shot_eval_ek100.py:146-171,
 * zero_shot_qa/inference.py:55-69): logits = scale * queries @ labels^T, their soft-max, and a stable descending sort -- here as one
 * call that returns the k best labels per query, the log-sum-exp (probability = exp(logit - lse)), optionally every logit, and optionally
 * the k best label GROUPS (the verb / noun marginal of the action table).
 *
 * Conventions, as in mreserve_media.h:
 *  - extern "C", plain pointers and sizes.  The library shares no handle, option or symbol with the other two libraries.
 *  - Every launching function takes a `void* stream` (a hipStream_t; NULL = default stream) and returns 0 on success, a negative
 *    MRZ_E* code otherwise; mrz_last_error() returns a thread-local description.
 *  - Caller-owned buffers, no allocation inside; all pointers are device pointers.  Arguments are validated before any launch.
 *  - Deterministic: no float atomics, a fixed reduction order, and the split of the work depends on (L, G, k) only: a query row's outputs
 *    are bit-identical whatever Q is and wherever the row sits in the batch.
 */
#ifndef MRESERVE_ZEROSHOT_H
#define MRESERVE_ZEROSHOT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MRZ_OK 0
#define MRZ_EINVAL (-1)   /* bad argument / unsupported shape */
#define MRZ_ELAUNCH (-2)  /* HIP launch error */

#define MRZ_DT_BF16 0
#define MRZ_DT_F32 1

#define MRZ_SLICE 512     /* labels per workgroup: L is cut into ceil(L / MRZ_SLICE) slices whose partial results a second launch merges */
#define MRZ_MAX_K 64
#define MRZ_MAX_H 2048

int mrz_version(void);
const char* mrz_last_error(void);

/* Bytes of scratch mrz_score_topk needs for these sizes (G = 0: no groups); 0 when none is needed (one slice, no groups); negative
 * (MRZ_EINVAL) for sizes outside the supported ranges.  The scratch needs 16-byte alignment and no initialisation. */
int64_t mrz_workspace_bytes(int64_t Q, int64_t L, int64_t G, int64_t k);

/* queries [Q, H] (row stride ldq elements, q_dtype) x labels [L, H] (row stride ldl, l_dtype), each MRZ_DT_F32 or MRZ_DT_BF16:
 *   dot[q, l]   = sum_h queries[q, h] labels[l, h]      fp32 accumulation of the exact operand values (fp32 operands are NOT rounded to bf16)
 *   logit[q, l] = fl32(scale * dot[q, l])               one multiply after the accumulation
 *   top_val / top_idx [Q, k]  fp32 / int32: the k largest logits of the row, by value descending and by LOWER label index among equal values
 *                             (a stable argsort of -logit; -0.0 == +0.0); for k > L the tail is -inf / -1
 *   lse [Q]                   fp32 log(sum_l exp(logit)), max-subtracted
 *   logits [Q, L]             fp32, contiguous; written only when the pointer is non-null
 * With groups [L] (int32, each in [0, G)) non-null, the score of a group is the largest logit of its labels, its representative the lowest-indexed
 * label attaining it, and gtop_val / gtop_group / gtop_label [Q, k] (fp32 / int32 / int32) are the k best groups by score descending, then by lower
 * representative: the first k distinct groups met when walking the sorted label list.  Empty groups never appear; the tail is -inf / -1 / -1.
 * A group value outside [0, G) is ignored (its label takes part in no group).
 * MRZ_EINVAL unless H % 64 == 0, 64 <= H <= 2048, 1 <= k <= 64, 1 <= L < 2^24, 1 <= Q < 2^31 - 16, 0 <= G <= L (G >= 1 with groups), strides >= H,
 * 16-byte aligned rows, known dtypes, non-null queries / labels / outputs (group outputs with groups; workspace when mrz_workspace_bytes > 0). */
int mrz_score_topk(const void* queries, int64_t ldq, int32_t q_dtype, const void* labels, int64_t ldl, int32_t l_dtype, int64_t Q, int64_t L,
                   int64_t H, float scale, int64_t k, float* top_val, int32_t* top_idx, float* lse, float* logits_or_null,
                   const int32_t* groups_or_null, int64_t G, float* gtop_val, int32_t* gtop_group, int32_t* gtop_label, void* workspace,
                   void* stream);

#ifdef __cplusplus
}
#endif
#endif
