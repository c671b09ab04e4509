/* TRAINING ON PACKED BATCHES: utterances of different lengths, one after the other, without padding.  The packed forms of the four
 * training entry points of pwv_hip_train.h that depend on where an utterance begins and ends (front forward, layer forward, layer
 * backward, front backward) and of the loss head of pwv_hip_train_loss.h.  An EXTENSION of the C ABI in a header of its own: pwv_hip.h
 * (PWV_HIP_VERSION 301), pwv_hip_train.h and pwv_hip_train_loss.h are what they were; a client includes this header (which includes
 * both) and finds the pwv_train_varlen_* / pwv_train_loss_varlen_* entry points in the same library.  Plain C99. */
#ifndef PWV_HIP_TRAIN_VARLEN_H
#define PWV_HIP_TRAIN_VARLEN_H

#include "pwv_hip_train.h"
#include "pwv_hip_train_loss.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------
 * Packed geometry.  Utterance i (0 <= i < n) owns rows cu_rows[i] .. cu_rows[i + 1] - 1 of every [rows] / tile32 buffer and P rows
 * cu_frames[i] .. cu_frames[i + 1] - 1 of `proj` / `d_proj`; row r of utterance i is its sample t = r - cu_rows[i] of T_i =
 * cu_rows[i + 1] - cu_rows[i], and everything pwv_hip_train.h says per utterance holds with that t and T_i:
 *   the P row of the sample is cu_frames[i] + (t + cond_offset) / cond_hop
 *   the look-back x[t - d] is zero for t < d; the look-ahead V[t + d] is added only while t + d < T_i
 *   the front's in[t - 1] and g_0[t + 1] stop at the utterance's ends
 * cu_rows and cu_frames are DEVICE int32 [n + 1], cu_rows[0] = cu_frames[0] = 0; the host passes n, rows = cu_rows[n] and proj_rows =
 * cu_frames[n] alone (grid sizes and buffer extents), so a call never waits for the tables.  The fields N, T and cond_frames of
 * pwv_train_args are not read.  A 32-row unit may hold parts of several utterances (the shortest is one hop): 33 threads locate the rows
 * of a unit and the first row behind it once, by a search of cu_rows, and leave (t, T_i, P row) in LDS for the unit's loads.  The kernel
 * clamps what it derives from the tables -- 0 <= t <= r, r + (T_i - t) <= rows, a P row to its utterance's last frame and to
 * 0 .. proj_rows - 1, a dP slot to 0 .. K - 1: stale tables give wrong numbers, never an access outside x, u, v, proj or d_proj.
 *
 * dP as in pwv_hip_train.h: K = (cond_hop + 30) / 32 + 1 slots per P row, unit u writes its share of frame f to slot
 * u - (first packed row of the frame) / 32, the caller zeroes the buffer (proj_rows K rows of d_proj_row_stride floats) and adds the
 * slots in index order.  Weight-gradient partials, the second launch, the grid rule and the workspace are those of pwv_hip_train.h:
 * pwv_train_workspace_bytes with N = 1, T = rows gives the size.  No floating-point atomics: a gradient is the same bits run after run
 * at a given max_workgroups.  The head is row-independent: pwv_train_head_fwd_f32 / pwv_train_head_bwd_f32 with N = 1, T = rows.
 *
 * Refused with PWV_EINVAL before a device is touched, pwv_last_error naming the field: what pwv_hip_train.h refuses, and cu_rows or
 * cu_frames NULL, n < 1, rows < n, rows >= 2^31 - 64, proj_rows < n, a wrong struct_size, workspace too small.
 * ------------------------------------------------------------------------------------- */
typedef struct pwv_train_varlen_args {
    size_t struct_size;                    /* = sizeof(pwv_train_varlen_args) as the caller was compiled */
    int32_t N, T;                          /* not read */
    int32_t form;                          /* PWV_TRAIN_RESIDUAL / PWV_TRAIN_LAST */
    int32_t dilation, next_dilation;
    int32_t cond_hop, cond_offset, cond_frames;      /* cond_frames: not read */
    int32_t proj_row_stride, d_proj_row_stride;
    int32_t max_workgroups;                /* 0 = two per compute unit */
    int32_t accumulate;
    /* activations */
    const float* in;                       /* [rows] */
    const float* x;                        /* tile32 */
    float* x_out;                          /* tile32 */
    const float* proj;                     /* proj_rows P rows, this layer's 128 columns */
    float* y;                              /* not used by the packed entry points (the head) */
    /* weights, TF layouts */
    const float* causal_filter;
    const float *filter, *gate, *dense, *dense_bias;
    const float *skip, *skip_bias, *post1, *post1_bias, *post2, *post2_bias;      /* not used (the head) */
    /* gradients that arrive */
    const float* d_out;                    /* [rows] */
    const float* d_mul;                    /* not used (the head) */
    const float* scale;                    /* [rows] or NULL */
    const float *u_next, *v_next;          /* tile32 */
    const float* d_o;                      /* tile32 */
    /* gradients that leave */
    float *u, *v;                          /* tile32 */
    float* d_o_out;                        /* not used (the head) */
    float* d_in;                           /* [rows] or NULL */
    float* d_proj;                         /* proj_rows K slots, this layer's 128 columns */
    float* d_causal_filter;
    float *d_filter, *d_gate, *d_dense, *d_dense_bias;
    float *d_skip, *d_skip_bias, *d_post1, *d_post1_bias, *d_post2, *d_post2_bias;      /* not used (the head) */
    void* workspace;
    size_t workspace_bytes;
    /* the packed batch */
    const int32_t* cu_rows;                /* device [n + 1] */
    const int32_t* cu_frames;              /* device [n + 1] */
    int32_t n;                             /* utterances */
    int32_t rows;                          /* = cu_rows[n] */
    int32_t proj_rows;                     /* = cu_frames[n] */
} pwv_train_varlen_args;

/* in, causal_filter -> x_out = x_0 */
int pwv_train_varlen_front_fwd_f32(const pwv_train_varlen_args* args, pwv_stream_t stream);
/* x, proj, filter, gate (+ dense, dense_bias) -> x_out */
int pwv_train_varlen_layer_fwd_f32(const pwv_train_varlen_args* args, pwv_stream_t stream);
/* x, proj, filter, gate, (dense, u_next, v_next, next_dilation | d_o) -> u, v, d_proj, d_filter, d_gate (, d_dense, d_dense_bias) */
int pwv_train_varlen_layer_bwd_f32(const pwv_train_varlen_args* args, pwv_stream_t stream);
/* in, causal_filter, u_next, v_next, next_dilation (, d_out, scale) -> d_causal_filter, d_in */
int pwv_train_varlen_front_bwd_f32(const pwv_train_varlen_args* args, pwv_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * The packed loss head: the arithmetic of pwv_train_loss_f32 (float64 direct DFT per frame, overlap-add as a gather, two launches, no
 * atomics) with the lengths read ON THE DEVICE.  Utterance i = samples cu_rows[i] .. cu_rows[i + 1] - 1 of `out`, `y` and `d_out`
 * (bounds clamped to 0 .. rows and to their predecessor, as pwv_hip_score.h does), F_i = 1 + (T_i - win) / hop frames if T_i >= win,
 * else none; a frame never crosses a boundary.  result[n][4] is the table of pwv_hip_score.h, per utterance.  The scales are the
 * batch's:
 *   d_out = weight_l1 sgn(out - y) / rows  +  weight_power 4 / (B sum_i F_i) (...)         B = nfft / 2 + 1
 * and an utterance without a frame contributes to the L1 alone.  With weight_power > 0 and sum_i F_i = 0 there is nothing to average
 * over: the power term of d_out is then left out (the caller, who knows the lengths, refuses that batch).
 * Workspace slots per utterance, as in pwv_hip_score.h: frame slots cu_rows[i] / hop + i .. out of rows / hop + n (each a partial and
 * win gradient values), tile slots cu_rows[i] / PWV_SCORE_TILE + i .. out of rows / PWV_SCORE_TILE + n; no slot is shared, none need
 * be initialised.  d_out and a row of result are the same bits run after run; a row of result does not depend on the other utterances.
 * Refused with PWV_EINVAL before a device is touched: args NULL, a wrong struct_size, NULL pointers (out, y, cu_rows, d_out, result,
 * workspace), n < 1, rows < n, rows >= 2^31 - 64, hop_length < 1, win_length < 0 or > PWV_SCORE_MAX_WIN, a negative or non-finite
 * weight, workspace_bytes too small.
 * ------------------------------------------------------------------------------------- */
typedef struct pwv_train_loss_varlen_args {
    size_t struct_size;                    /* = sizeof(pwv_train_loss_varlen_args) as the caller was compiled */
    const float* out;                      /* device [rows]: the predictions */
    const float* y;                        /* device [rows]: the ground truth */
    const int32_t* cu_rows;                /* device [n + 1] */
    int32_t n;                             /* utterances */
    int32_t rows;                          /* = cu_rows[n] */
    int32_t win_length, hop_length;
    double weight_l1, weight_power;
    float* d_out;                          /* device [rows] */
    double* result;                        /* device [n, 4] */
    void* workspace;                       /* device, pwv_train_loss_varlen_workspace_bytes */
    size_t workspace_bytes;
} pwv_train_loss_varlen_args;

size_t pwv_train_loss_varlen_workspace_bytes(const pwv_train_loss_varlen_args* args);      /* 0 for arguments that are refused */
int pwv_train_loss_varlen_f32(const pwv_train_loss_varlen_args* args, pwv_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PWV_HIP_TRAIN_VARLEN_H */
