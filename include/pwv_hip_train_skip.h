/* TRAINING THE SKIP-CONNECTION ARCHITECTURE (model.use_skip_connection True; modules.py:142-147, :242-250): the head of a net reads
 * the sum of ALL layers' skip outputs instead of the last layer's alone.  The layer forward and backward and the head of
 * pwv_hip_train.h with that sum in them, for uniform [N, T] batches and for the packed batches of pwv_hip_train_varlen.h alike.  An
 * EXTENSION of the C ABI in a header of its own: pwv_hip.h (PWV_HIP_VERSION 301), pwv_hip_train.h and pwv_hip_train_varlen.h are what
 * they were; a client includes this header (which includes them) and finds the pwv_train_skip_* entry points in the same library.
 * The front calls (pwv_train_front_fwd_f32 / _bwd_f32 and their packed forms) are the existing ones.  Plain C99. */
#ifndef PWV_HIP_TRAIN_SKIP_H
#define PWV_HIP_TRAIN_SKIP_H

#include "pwv_hip_train_varlen.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------
 * The math, per net of L layers; everything not named is as in pwv_hip_train.h:
 *   forward   S[t]    = sum_j ( o_j[t] skip_j + skip_bias_j )      summed in layer order j = 0 .. L - 1, fp32, [rows, 128]
 *             y[t]    = relu(relu(S) post1 + b1) post2 + b2
 *             x_{j+1} = x_j + o_j dense_j + dense_bias_j           j < L - 1: the last layer's dense is never read
 *   backward  dS      = relu'(S) * ((relu'(h1) * (dy post2^T)) post1^T)      once per net, from the head
 *             d o_j   = g_j dense_j^T + dS skip_j^T                (PWV_TRAIN_LAST: g = 0, the second term alone; `d_o` is not read)
 *             d skip_j = sum_t o_j[t]^T dS[t]
 *             d skip_bias_j = sum_t dS[t]                          the same vector for every j: the head backward writes it once
 *             dF, dG, U, V, dWfg, d dense, d dense_bias, dP: unchanged
 * S and dS are tile32 with 128 channels: pwv_tile32_floats(rows, 128) floats each.  A row of S belongs to one 32-row unit and the
 * layer calls of a step run in stream order, so S is the same bits whatever the grid.  The layer forward writes S
 * (skip_accumulate 0: layer 0) or adds to it (1: S + (o skip + skip_bias), one rounding); it touches the rows of the batch alone,
 * and no entry point reads a padding row of the last block of S or dS.  A PWV_TRAIN_LAST layer forward writes no x_out.
 *
 * What a training step keeps: x_j of every layer and S per net (512 bytes per row); no layer's o.
 *
 * The layer backward accumulates d skip_j over a workgroup's units in registers; its partial is the one of pwv_hip_train.h with
 * 64 x 128 floats behind it, and the second launch adds them in the same fixed order.  No floating-point atomics.
 * pwv_train_skip_workspace_bytes is enough for any entry point of this header and for the front calls at the same rows and
 * max_workgroups.
 *
 * The batch: cu_rows == NULL is a uniform batch (train.N, train.T, train.cond_frames as in pwv_hip_train.h); otherwise the packed
 * tables of pwv_hip_train_varlen.h (cu_rows, cu_frames: device int32 [n + 1]; rows = cu_rows[n]; proj_rows = cu_frames[n]) and
 * train.N, train.T, train.cond_frames are not read.  The head entry points read no frame: cu_frames and proj_rows may be 0 there.
 *
 * The weights of the call are train.filter .. train.dense_bias, train.skip [1,64,128] and train.skip_bias [128] (this layer's;
 * a bias may be NULL) and, for the head, train.post1 .. train.post2_bias; train.d_skip and train.d_skip_bias are not read: the
 * gradients of this header leave through the fields below.
 *
 * Refused with PWV_EINVAL before a device is touched, pwv_last_error naming the field: what pwv_hip_train.h and
 * pwv_hip_train_varlen.h refuse, and skip_sum, d_skip_sum, d_skip_sum_out, d_skip or train.skip NULL where the entry point needs
 * it, and a workspace smaller than pwv_train_skip_workspace_bytes gives.
 * ------------------------------------------------------------------------------------- */
typedef struct pwv_train_skip_args {
    pwv_train_args train;                  /* train.struct_size = sizeof(pwv_train_skip_args) */
    float* skip_sum;                       /* tile32, 128 channels: S (layer forward: written / added to; head: read) */
    const float* d_skip_sum;               /* tile32, 128 channels: the dS that arrives (layer backward) */
    float* d_skip_sum_out;                 /* tile32, 128 channels: dS (head backward) */
    float* d_skip;                         /* [1,64,128]: this layer's (layer backward) */
    float* d_skip_bias;                    /* [128] or NULL: the column sums of dS (head backward), every layer's d skip_bias */
    int32_t skip_accumulate;               /* layer forward: 0 = write S, 1 = add to it */
    /* the packed batch; cu_rows NULL: a uniform batch */
    const int32_t* cu_rows;                /* device [n + 1] */
    const int32_t* cu_frames;              /* device [n + 1] */
    int32_t n;                             /* utterances */
    int32_t rows;                          /* = cu_rows[n] */
    int32_t proj_rows;                     /* = cu_frames[n] */
} pwv_train_skip_args;

size_t pwv_train_skip_workspace_bytes(const pwv_train_skip_args* args);      /* reads the batch and max_workgroups; 0 if refused */

/* x, proj, filter, gate, skip (, skip_bias) (+ dense, dense_bias -> x_out) -> skip_sum */
int pwv_train_skip_layer_fwd_f32(const pwv_train_skip_args* args, pwv_stream_t stream);
/* skip_sum, post1 .. post2_bias -> y */
int pwv_train_skip_head_fwd_f32(const pwv_train_skip_args* args, pwv_stream_t stream);
/* skip_sum, d_out (, d_mul), post1 .. post2_bias -> d_skip_sum_out, d_skip_bias, d_post1 .. d_post2_bias */
int pwv_train_skip_head_bwd_f32(const pwv_train_skip_args* args, pwv_stream_t stream);
/* x, proj, filter, gate, skip, d_skip_sum (, dense, u_next, v_next, next_dilation) -> u, v, d_proj, d_filter, d_gate, d_skip
 * (, d_dense, d_dense_bias) */
int pwv_train_skip_layer_bwd_f32(const pwv_train_skip_args* args, pwv_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PWV_HIP_TRAIN_SKIP_H */
