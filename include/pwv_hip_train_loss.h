/* The LOSS HEAD of training: the reference's whole cost (models.py:90-99), weight_l1 * l1_loss(out, y) + weight_power * power_loss(out, y),
 * and its gradient for `out`, in one call on the device.  pwv_hip_score.h measures the same two terms forward only; pwv_hip_train.h
 * starts its backward from an arbitrary d_out [N T] -- this call makes that d_out.  An EXTENSION of the C ABI in a header of its own:
 * pwv_hip.h (PWV_HIP_VERSION 301), pwv_hip_score.h and pwv_hip_train.h are what they were; a client includes this header (which includes
 * pwv_hip_score.h for PWV_SCORE_MAX_WIN and the meaning of the table) and finds the two entry points in the same library.  Plain C99. */
#ifndef PWV_HIP_TRAIN_LOSS_H
#define PWV_HIP_TRAIN_LOSS_H

#include "pwv_hip_score.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------
 * Uniform batches only: utterance i is samples i T .. (i + 1) T - 1 of `out` and `y`.  Row i of
 *   result[n][4] = { abs_sum, samples, power_sum, terms }      (float64)
 * has exactly the meaning of pwv_hip_score.h: periodic Hann window w[j] = 0.5 - 0.5 cos(2 pi j / win), frame f = samples
 * f hop .. f hop + win - 1, zero-padded behind to nfft = the smallest power of two >= win, F = 1 + (T - win) / hop frames, B = nfft / 2 + 1
 * bins; a frame never crosses an utterance boundary.  The loss of the batch is
 *   weight_l1 * (sum_i abs_sum) / (n T)  +  weight_power * (sum_i power_sum) / (n F B)
 * (the reference's reduce_mean over all elements; the rfft bins only, no Hermitian doubling), and with
 *   a_j = w[j] out[f hop + j],   Ar_b = sum_j a_j cos(2 pi b j / nfft),   Ai_b = sum_j a_j sin(2 pi b j / nfft),   Br_b, Bi_b the same of y,
 *   D_b = (Ar_b^2 + Ai_b^2) - (Br_b^2 + Bi_b^2)
 * its gradient is
 *   d_out[i T + t] = weight_l1 sgn(out - y) / (n T)
 *                  + weight_power 4 / (n F B) sum_{f : 0 <= t - f hop < win} w[j] sum_{b = 0 .. nfft / 2} D_b (Ar_b cos(2 pi b j / nfft) + Ai_b sin(2 pi b j / nfft)),
 *                    j = t - f hop;   sgn(0) = 0.
 * EVERY element of d_out is written; a sample that no frame covers (behind the last frame; between frames when hop > win) gets the L1
 * term alone.  Every product and sum is float64 on the float32 inputs; d_out is rounded to float32 once.
 *   weight_power == 0 or win_length == 0     the L1 alone: power_sum = terms = 0, no frame is formed, T may be shorter than win_length.
 * Two launches, no floating-point atomics.  The first: one workgroup per (utterance, frame) -- a direct real DFT of both frames from an
 * LDS table of twiddles, then the same table run backward over D_b (Ar_b, Ai_b) into the frame's win gradient values, kept in `workspace`
 * -- and one per (utterance, tile of PWV_SCORE_TILE samples) for the partial sums of |out - y|.  The second: one workgroup per tile GATHERS
 * d_out -- a sample adds the contributions of its frames in ascending f -- and one per utterance adds that utterance's partials in an order
 * that depends on their index alone.  d_out and result are the same bits run after run, and utterance i's part of both does not depend on
 * the contents of the other utterances.
 * Workspace: n F + n ceil(T / PWV_SCORE_TILE) + n F win doubles (pwv_train_loss_workspace_bytes; 0 for arguments that are refused); it need
 * not be initialised.  The call only enqueues on `stream`.
 * Refused with PWV_EINVAL before a device is touched, pwv_last_error naming the field: args NULL, a wrong struct_size, NULL pointers (out,
 * y, d_out, result, workspace), n < 1, T < 1, hop_length < 1, win_length < 0 or > PWV_SCORE_MAX_WIN, weight_power > 0 with
 * 0 < T < win_length (no frame: the reference's mean would be over nothing), a negative or non-finite weight, n T beyond int32,
 * workspace_bytes too small.
 * ------------------------------------------------------------------------------------- */
typedef struct pwv_train_loss_args {
    size_t struct_size;                    /* = sizeof(pwv_train_loss_args) as the caller was compiled */
    const float* out;                      /* device [n T]: the predictions */
    const float* y;                        /* device [n T]: the ground truth */
    int32_t n, T;                          /* utterances, samples per utterance */
    int32_t win_length, hop_length;
    double weight_l1, weight_power;
    float* d_out;                          /* device [n T]: the gradient of the loss for `out` */
    double* result;                        /* device [n, 4] */
    void* workspace;                       /* device, pwv_train_loss_workspace_bytes; need not be initialised */
    size_t workspace_bytes;
} pwv_train_loss_args;

size_t pwv_train_loss_workspace_bytes(const pwv_train_loss_args* args);
int pwv_train_loss_f32(const pwv_train_loss_args* args, pwv_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PWV_HIP_TRAIN_LOSS_H */
