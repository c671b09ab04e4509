/* TRAINING: the forward with saved activations and the backward pass of the default architecture (filter_width 2, R = D = 64, S = 128,
 * Q = 1, frame-rate 'repeat' conditioning, no normalisers, no skip accumulation), one net per call, exact-fp32 MFMA arithmetic
 * (v_mfma_f32_32x32x2_f32, the class of PWV_PREC_F32).  An EXTENSION of the C ABI in a header of its own: pwv_hip.h and PWV_HIP_VERSION
 * are what they were; a client includes this header (which includes pwv_hip.h) and finds the pwv_train_* entry points in the same
 * library.  Plain C99.  Reference call sites: modules.py:129-259 (the net), models.py:31-70 (the flows), models.py:80-103 (the loss). */
#ifndef PWV_HIP_TRAIN_H
#define PWV_HIP_TRAIN_H

#include "pwv_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------
 * The math, per net; layer j has dilation d, t is utterance-local, x[t-d] = 0 for t < d:
 *   x_0[t]     = in[t-1] cf[0] + in[t] cf[1]                                             causal layer, in[-1] = 0
 *   FG[t]      = [x_j[t-d] | x_j[t]] Wfg + P_j[frame(t)]     Wfg = [[filter[0] | gate[0]], [filter[1] | gate[1]]]  (128 x 128)
 *   o[t]       = tanh(F) sigmoid(G)
 *   x_{j+1}[t] = x_j[t] + o[t] dense + dense_bias                                        every layer but the last
 *   y[t]       = relu(relu(o skip + skip_bias) post1 + b1) post2 + b2                    the last layer's o
 * P_j = frames [gc_filter | gc_gate] + [filter_bias | gate_bias] is made by the caller at frame rate, in the NATURAL column order
 * (filter 0..63, gate 64..127; not the forward kernels' order) and unscaled; the P row of sample t of utterance n is
 * n cond_frames + (t + cond_offset) / cond_hop, floats proj_row_stride apart; `proj` points at this layer's 128 columns.
 *
 * Weights are read in their TensorFlow layouts and every weight gradient is written in the same layout: filter / gate [2,64,64], dense
 * [1,64,64], skip [1,64,128], postprocess1 [1,128,128], postprocess2 [1,128,1], causal_layer/filter [2,1,64], biases [64] / [128] / [1].
 * A bias pointer may be NULL (use_biases False): it reads as zeros and its gradient is not written.  Activations are tile32 (pwv_hip.h),
 * 64 channels, pwv_tile32_floats(N T, 64) floats; the padding rows of the last block may be written.
 *
 * What a training step keeps: x_j for every layer (one tile32 buffer per net-layer, no ping-pong) and the last layer's o:
 *   bytes per net-layer = 4 * 64 * round32(N T);  a model whose flow f has L_f layers keeps 2 nets * sum_f (L_f + 1) such buffers
 *   (the default model, L = 10, 10, 10, 30, at 8 x 4000 samples: 8.2 MB each, 2 * 64 of them = 1.05 GB).
 * F, G, o of the other layers and the head's hidden layers are RECOMPUTED by the backward kernels from x_j and P_j.
 *
 * Backward of a layer, g[t] = the gradient that arrives for x_{j+1}[t]:
 *   do = g dense^T   (PWV_TRAIN_LAST: do is read from `d_o`, the output of pwv_train_head_bwd_f32, and g = 0)
 *   dF = do sigmoid(G) (1 - tanh^2 F),  dG = do tanh F sigmoid(G) (1 - sigmoid(G))
 *   U[t] = g[t] + dFG[t] Wfg[64:128]^T,   V[t] = dFG[t] Wfg[0:64]^T         written to `u`, `v`
 *   the gradient for x_j[t] is U[t] + V[t + d] while t + d is inside the utterance: the kernel of layer j - 1 (and the front) forms it
 *   when it loads its g, from `u_next`, `v_next` and `next_dilation` = this layer's d.  No atomics: the look-ahead mirrors the
 *   forward's look-back.
 *   dWfg = sum_t a^T dFG (scattered to d_filter / d_gate),  d_dense = sum_t o^T g,  d_dense_bias = sum_t g
 *   dP[frame] = sum over the frame's t of dFG[t]: `d_proj` holds, per P row f, K = (cond_hop + 30) / 32 + 1 slots of d_proj_row_stride
 *   floats (slot k of row f at d_proj + (f K + k) d_proj_row_stride, this layer's 128 columns): the 32-row unit u writes its share of
 *   frame f to slot u - (first row of the frame) / 32, and the caller adds the K slots of a row in index order.  The caller ZEROES the
 *   buffer first: a frame shorter than K units leaves slots unwritten.  A slot's value depends on the unit alone, not on the grid.
 * Weight gradients are sums over all rows: every workgroup accumulates the rows of its units on the fp32 MFMA (rows as the K
 * dimension), writes ONE partial to `workspace`, and a second launch adds the partials in a fixed order (eight contiguous runs of
 * partials, each in index order, then the eight sums in order) and writes the TF layouts.  No floating-point atomics anywhere: a
 * gradient is the same bits run after run.  The grid is min(units, max_workgroups) workgroups, max_workgroups = 0: two per compute
 * unit; unit u goes to workgroup u mod grid.  pwv_train_workspace_bytes is enough for any entry
 * point at these N, T, max_workgroups; the workspace need not be initialised, and one workspace serves calls on one stream.
 *
 * Every call only enqueues on `stream`.  Refused with PWV_EINVAL before a device is touched, pwv_last_error naming the field: args NULL,
 * a wrong struct_size, a NULL pointer the entry point needs, N, T < 1, N T >= 2^31 - 64, dilation < 1, cond_hop < 1, workspace too small.
 * ------------------------------------------------------------------------------------- */
#define PWV_TRAIN_RESIDUAL 0
#define PWV_TRAIN_LAST 1

typedef struct pwv_train_args {
    size_t struct_size;                    /* = sizeof(pwv_train_args) as the caller was compiled */
    int32_t N, T;                          /* utterances, samples per utterance */
    int32_t form;                          /* PWV_TRAIN_RESIDUAL / PWV_TRAIN_LAST */
    int32_t dilation, next_dilation;       /* this layer's d; the d of the layer whose u / v are u_next / v_next */
    int32_t cond_hop, cond_offset, cond_frames;
    int32_t proj_row_stride, d_proj_row_stride;
    int32_t max_workgroups;                /* 0 = two per compute unit */
    int32_t accumulate;                    /* front backward: 1 = add to d_in instead of starting from d_out * scale */
    /* activations */
    const float* in;                       /* [N T]: the flow's input (front) */
    const float* x;                        /* tile32: x_j (layer), the last layer's o (head) */
    float* x_out;                          /* tile32: x_{j+1} or, PWV_TRAIN_LAST, o (layer forward); x_0 (front forward) */
    const float* proj;                     /* P rows, this layer's 128 columns */
    float* y;                              /* [N T]: the net's output (head forward) */
    /* weights, TF layouts */
    const float* causal_filter;
    const float *filter, *gate, *dense, *dense_bias;
    const float *skip, *skip_bias, *post1, *post1_bias, *post2, *post2_bias;
    /* gradients that arrive */
    const float* d_out;                    /* [N T]: of the flow's output (head backward, front backward) */
    const float* d_mul;                    /* [N T] or NULL: head backward takes dy = d_out * d_mul (the scaler: ds = d out * in) */
    const float* scale;                    /* [N T] or NULL: front backward starts d_in = d_out * scale (the affine: d in = d out * s) */
    const float *u_next, *v_next;          /* tile32: of the layer above (layer backward, PWV_TRAIN_RESIDUAL), of layer 0 (front backward) */
    const float* d_o;                      /* tile32: layer backward, PWV_TRAIN_LAST */
    /* gradients that leave */
    float *u, *v;                          /* tile32 (layer backward) */
    float* d_o_out;                        /* tile32: d o of the last layer (head backward) */
    float* d_in;                           /* [N T]: of the flow's input (front backward), or NULL */
    float* d_proj;                         /* layer backward; see above */
    float* d_causal_filter;
    float *d_filter, *d_gate, *d_dense, *d_dense_bias;
    float *d_skip, *d_skip_bias, *d_post1, *d_post1_bias, *d_post2, *d_post2_bias;
    void* workspace;
    size_t workspace_bytes;
} pwv_train_args;

size_t pwv_train_workspace_bytes(const pwv_train_args* args);      /* reads N, T, max_workgroups; 0 for arguments that are refused */

/* forward with saved activations: in, causal_filter -> x_out = x_0 */
int pwv_train_front_fwd_f32(const pwv_train_args* args, pwv_stream_t stream);
/* x, proj, filter, gate (+ dense, dense_bias) -> x_out */
int pwv_train_layer_fwd_f32(const pwv_train_args* args, pwv_stream_t stream);
/* x = o, skip .. post2_bias -> y */
int pwv_train_head_fwd_f32(const pwv_train_args* args, pwv_stream_t stream);

/* x = o, d_out (, d_mul), head weights -> d_o_out, d_skip .. d_post2_bias */
int pwv_train_head_bwd_f32(const pwv_train_args* args, pwv_stream_t stream);
/* x, proj, filter, gate, (dense, u_next, v_next, next_dilation | d_o) -> u, v, d_proj, d_filter, d_gate (, d_dense, d_dense_bias) */
int pwv_train_layer_bwd_f32(const pwv_train_args* args, pwv_stream_t stream);
/* the causal layer and the affine: in, causal_filter, u_next, v_next, next_dilation (, d_out, scale) -> d_causal_filter, d_in */
int pwv_train_front_bwd_f32(const pwv_train_args* args, pwv_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PWV_HIP_TRAIN_H */
