/* TRAINING THE SHARED-NET ARCHITECTURE (model.shared_nets True; a build extension, the reference has no such code): each flow has ONE
 * WaveNet with two output channels, out = in * y[..., 0] + y[..., 1], instead of a scaler net and a shifter net.  The layer kernels,
 * the front kernels, the loss head and the optimiser do not know how many nets a flow has; the output width Q is known to the net's
 * head alone (postprocess2 [1,128,Q]).  So this header is the Q = 2 head, forward and backward, on either input: the last layer's
 * gated output o (pwv_hip_train.h) or the skip sum S (pwv_hip_train_skip.h).  An EXTENSION of the C ABI in a header of its own:
 * pwv_hip.h (PWV_HIP_VERSION 301) and every older training header are what they were; a client includes this header (which includes
 * them) and finds the pwv_train_shared_* entry points in the same library.  Plain C99. */
#ifndef PWV_HIP_TRAIN_SHARED_H
#define PWV_HIP_TRAIN_SHARED_H

#include "pwv_hip_train_skip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------
 * The math, per row r of the net; everything not named is as in pwv_hip_train.h / pwv_hip_train_skip.h:
 *   forward   h1     = relu(o skip + skip_bias)        PWV_TRAIN_HEAD_IN_GATED: train.x = the last layer's o (tile32, 64 channels)
 *             h1     = relu(S)                         PWV_TRAIN_HEAD_IN_SKIPSUM: skip_sum = S (tile32, 128 channels)
 *             h2     = relu(h1 post1 + b1)
 *             y_q[r] = h2[r] . post2[:, q] + b2[q]     q = 0, 1: train.y = the SCALE plane y_0, y_shift = the SHIFT plane y_1
 *   backward  dy_0   = d_out * d_mul,  dy_1 = d_out    d_mul = the flow's input: out = in y_0 + y_1 (d_mul NULL reads as ones)
 *             dz2    = relu'(h2) * (dy_0 post2[:, 0] + dy_1 post2[:, 1])     the sum always in this order
 *             d post2[c, q] = sum_r h2[r, c] dy_q[r],  d b2[q] = sum_r dy_q[r]
 *             d post1, d b1 and what lies behind them: the existing heads' -- GATED: d skip, d skip_bias and d o (train.d_o_out,
 *             tile32, 64 channels); SKIPSUM: dS (d_skip_sum_out, tile32, 128 channels) and its column sums (train.d_skip_bias:
 *             every layer's d skip_bias)
 * postprocess2 is [1,128,2] in TensorFlow's layout: element (c, q) at 2 c + q; postprocess2_bias is [2]; their gradients are written
 * in the same layouts.  The two planes are two contiguous [rows] arrays and not an interleaved [rows, 2]: pwv_train_front_bwd_f32
 * takes the scale plane as its `scale` as it is.
 *
 * The rows are train.N * train.T; the head is row-local, so a packed batch calls it with N = 1, T = rows.  Rows at or beyond that
 * are neither read as data nor written.  y_q does not depend on the grid; a gradient is the same bits run after run: every workgroup
 * writes ONE partial (the existing head's partial + 128 floats for the second column of d post2 + 1 for the second d b2) and a second
 * launch adds the partials in the fixed order of pwv_hip_train.h.  No floating-point atomics.  pwv_train_shared_workspace_bytes is
 * enough for either entry point in either mode at these N, T, max_workgroups.
 *
 * Refused with PWV_EINVAL before a device is touched, pwv_last_error naming the field: what pwv_hip_train.h refuses (args NULL,
 * train.struct_size, N, T < 1, N T >= 2^31 - 64, max_workgroups < 0), an unknown head_in, a pointer the mode or the entry point needs
 * being NULL (GATED: train.x, train.skip; SKIPSUM: skip_sum; both: post1, post2; forward: train.y, y_shift; backward: train.d_out and
 * train.d_o_out / d_skip_sum_out), and a workspace smaller than pwv_train_shared_workspace_bytes gives.  A bias may be NULL: it reads
 * as zeros and its gradient is not written.
 * ------------------------------------------------------------------------------------- */
#define PWV_TRAIN_HEAD_IN_GATED 0
#define PWV_TRAIN_HEAD_IN_SKIPSUM 1

typedef struct pwv_train_shared_args {
    pwv_train_args train;                  /* train.struct_size = sizeof(pwv_train_shared_args) */
    int32_t head_in;                       /* PWV_TRAIN_HEAD_IN_GATED / PWV_TRAIN_HEAD_IN_SKIPSUM */
    const float* skip_sum;                 /* tile32, 128 channels: S (SKIPSUM) */
    float* d_skip_sum_out;                 /* tile32, 128 channels: dS (SKIPSUM, backward) */
    float* y_shift;                        /* [N T]: the shift plane y[..., 1] (forward); train.y is the scale plane y[..., 0] */
} pwv_train_shared_args;

size_t pwv_train_shared_workspace_bytes(const pwv_train_shared_args* args);  /* reads N, T, max_workgroups; 0 if refused */

/* x = o, skip (, skip_bias) | skip_sum;  post1 .. post2_bias -> y, y_shift */
int pwv_train_shared_head_fwd_f32(const pwv_train_shared_args* args, pwv_stream_t stream);
/* the same inputs, d_out (, d_mul) -> d_o_out, d_skip, d_skip_bias | d_skip_sum_out, d_skip_bias;  d_post1 .. d_post2_bias */
int pwv_train_shared_head_bwd_f32(const pwv_train_shared_args* args, pwv_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PWV_HIP_TRAIN_SHARED_H */
