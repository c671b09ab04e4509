/* TRAINING WITH A PER-SAMPLE CONDITION: the layer forward and backward of pwv_hip_train.h for the transposed-conv conditioning
 * (models.py:109-124), whose condition changes every sample -- the projection can no longer be made at frame rate, so the conditioning
 * product and its gradients happen INSIDE the sample-rate layer kernels.  An EXTENSION of the C ABI in a header of its own: pwv_hip.h
 * (PWV_HIP_VERSION 301) and pwv_hip_train.h are what they were; a client includes this header (which includes both) and finds the
 * pwv_train_cond_* entry points in the same library.  Plain C99. */
#ifndef PWV_HIP_TRAIN_COND_H
#define PWV_HIP_TRAIN_COND_H

#include "pwv_hip_train.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------
 * The math per layer, uniform [N, T] batches, exact-fp32 MFMA (v_mfma_f32_32x32x2_f32); everything that is not named here is as in
 * pwv_hip_train.h (x, x_out, u, v, the look-back and the look-ahead, the two forms, the TF layouts, tile32 activations):
 *   FG[t]      = [x[t-d] | x[t]] Wfg + c[t] Gc + b          Gc = [gc_filter[0] | gc_gate[0]]  (C x 128),  b = [filter_bias | gate_bias]
 *   d_gc       = sum_t c[t]^T dFG[t]                        scattered to d_gc_filter / d_gc_gate, TF layout [1, C, 64]
 *   d_b        = sum_t dFG[t]                               d_filter_bias / d_gate_bias [64]
 *   d_cond[t] (+)= dFG[t] Gc^T
 * `cond` is the per-sample condition, fp32, row-major: the row of sample t of utterance n lies at (n cond_utt_rows + t) cond_row_stride
 * floats, C = cond_channels of them are read.  A caller may therefore pass a pointer into the UNCROPPED [N, T + hop, C] tensor
 * (cond + (hop / 2) C, cond_utt_rows = T + hop) and skip the crop.  `d_cond` has the same addressing: every row belongs to one 32-row
 * unit, so it is a plain read-modify-write by that unit -- d_cond_accumulate = 0 writes, 1 adds; the calls of a step run in stream order,
 * which makes d_cond the same bits whatever the grid.  C is a run-time field, even, 2 <= C <= PWV_TRAIN_COND_MAX; in LDS the condition
 * tile is padded to 96 columns of zeros, and rows >= C of gc_filter / gc_gate are never read.  A bias pointer may be NULL: it reads as
 * zeros and its gradient is not written.
 *
 * Weight gradients as in pwv_hip_train.h: every workgroup writes ONE partial, now kLayerPart + C 128 + 128 floats (dWfg | d dense |
 * d dense_bias | d_gc | d_b), and a second launch adds the partials in the fixed order and writes the TF layouts.  No floating-point
 * atomics: a gradient is the same bits run after run at a given max_workgroups.  pwv_train_cond_workspace_bytes is the size for these
 * N, T, max_workgroups and C; it is at least pwv_train_workspace_bytes, so the head and front calls of a step may use the same workspace.
 *
 * LDS.  The backward stages [x[t-d] | x[t]] (32 x 129), FG / dFG (32 x 129), g, d o and o (32 x 65 each) and the condition tile
 * (32 x 97): 70.4 KB side by side, over the 64 KiB a kernel may declare statically.  d o and o ALIAS: the gating pass reads d o[r][c] and
 * writes o[r][c] in its place, the same thread the same element, and nothing reads d o afterwards.  That leaves 62080 bytes of static
 * LDS (forward: 53760; no launch requests dynamic LDS), and two workgroups share a CU's 160 KiB, as in pwv_hip_train.h.
 *
 * Every call only enqueues on `stream`.  Refused with PWV_EINVAL before a device is touched, pwv_last_error naming the field: args NULL,
 * a wrong train.struct_size, what pwv_hip_train.h refuses (N, T < 1, N T >= 2^31 - 64, dilation < 1, a NULL pointer the entry point
 * needs), cond NULL, cond_channels odd or outside 2 .. 96, cond_row_stride < cond_channels, cond_utt_rows < T, N cond_utt_rows >= 2^31,
 * a non-NULL train.proj or train.d_proj (there is no frame-rate projection here), gc_filter / gc_gate NULL, the backward's d_cond,
 * d_gc_filter or d_gc_gate NULL, workspace too small.  cond_hop, cond_offset, cond_frames and the row strides of train are not read.
 * ------------------------------------------------------------------------------------- */
#define PWV_TRAIN_COND_MAX 96

typedef struct pwv_train_cond_args {
    pwv_train_args train;                  /* train.struct_size = sizeof(pwv_train_cond_args) as the caller was compiled */
    const float* cond;                     /* the condition rows */
    const float *gc_filter, *gc_gate;      /* [1, C, 64] */
    const float *filter_bias, *gate_bias;  /* [64] or NULL */
    float* d_cond;                         /* layer backward */
    float *d_gc_filter, *d_gc_gate;        /* [1, C, 64] */
    float *d_filter_bias, *d_gate_bias;    /* [64] or NULL */
    int32_t cond_channels;                 /* C */
    int32_t cond_row_stride;               /* floats between the rows of cond and of d_cond */
    int32_t cond_utt_rows;                 /* rows between the utterances of cond and of d_cond, >= T */
    int32_t d_cond_accumulate;             /* 0: d_cond = ..., 1: d_cond += ... */
} pwv_train_cond_args;

size_t pwv_train_cond_workspace_bytes(const pwv_train_cond_args* args);      /* reads N, T, max_workgroups, cond_channels; 0 if refused */

/* x, cond, filter, gate, gc_filter, gc_gate (, the biases, dense, dense_bias) -> x_out; both forms */
int pwv_train_cond_layer_fwd_f32(const pwv_train_cond_args* args, pwv_stream_t stream);
/* ... (dense, u_next, v_next, next_dilation | d_o) -> u, v, d_cond, d_filter, d_gate, d_gc_filter, d_gc_gate (, d_filter_bias, d_gate_bias,
 * d_dense, d_dense_bias) */
int pwv_train_cond_layer_bwd_f32(const pwv_train_cond_args* args, pwv_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PWV_HIP_TRAIN_COND_H */
