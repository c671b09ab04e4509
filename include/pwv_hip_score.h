/* SCORING generated audio on the device: the L1 and the STFT power loss of a prediction against its ground truth.  An EXTENSION of the C
 * ABI, declared in a header of its own: pwv_hip.h (52 entry points, PWV_HIP_VERSION 301), pwv_hip_mel_stream.h and pwv_hip_live_tick.h are
 * what they were; a client includes this header (which includes pwv_hip.h) and finds pwv_score_workspace_bytes and pwv_score_f32 in the
 * same library.  Plain C99. */
#ifndef PWV_HIP_SCORE_H
#define PWV_HIP_SCORE_H

#include "pwv_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------
 * One call scores n utterances: utterance i is L_i float32 samples of `out` against the same samples of `y`, and fills row i of
 *   result[n][4] = { abs_sum, samples, power_sum, terms }      (float64)
 *   abs_sum    sum over t of |out[t] - y[t]|;  samples = L_i
 *   power_sum  sum over frames f and bins b of (P_out[f, b] - P_y[f, b])^2, P = |rfft|^2 of the frame f hop .. f hop + win - 1 under the
 *              periodic Hann window w[j] = 0.5 - 0.5 cos(2 pi j / win), zero-padded behind to fft_length = the smallest power of two
 *              >= win (tf.contrib.signal.stft at its defaults: no centring, pad_end = False)
 *   terms      F (fft_length / 2 + 1),  F = 0 for L_i < win, else 1 + (L_i - win) / hop
 * Every product and sum is float64 on the float32 inputs.  A caller forms l1 = abs_sum / samples and power = power_sum / terms per
 * utterance, or the ratios of the column sums per batch.
 *   win_length == 0     L1 only: power_sum = terms = 0 (this is how two mels are compared: a row = the values of one mel).
 *   uniform form        cu_rows == NULL: utterance i is samples i T .. (i + 1) T - 1; rows >= n T.
 *   packed form         cu_rows = device int32 [n + 1], utterance i is samples cu_rows[i] .. cu_rows[i + 1] - 1.  The lengths are read ON THE
 *                       DEVICE: the host passes the capacities n and rows alone, the grid depends on nothing else, and a captured call is
 *                       replayed for any lengths that fit.  A bound outside 0 .. rows (or below its predecessor) is clamped: a stale
 *                       table gives a wrong row of `result`, never an access outside the buffers.
 * Two launches.  The first writes one partial per (utterance, frame) and one per (utterance, tile of PWV_SCORE_TILE samples counted from
 * the utterance's own start) into `workspace`; the second, one workgroup per utterance, adds that utterance's partials in an order that
 * depends on their index within the utterance alone.  No floating-point atomics: a row of `result` is the same bits whether its
 * utterance is scored alone, in a uniform batch or in a packed one, at any position, and run after run.
 * Workspace slots: utterance i owns frame slots cu_rows[i] / hop + i .. cu_rows[i + 1] / hop + i (F_i <= L_i / hop + 1 of them are
 * used) out of rows / hop + n, and tile slots cu_rows[i] / TILE + i .. out of rows / TILE + n; a slot no utterance uses is neither
 * written nor read.  pwv_score_workspace_bytes gives the size (0 for arguments pwv_score_f32 refuses).
 * Refused with PWV_EINVAL before a device is touched, pwv_last_error naming the field: args NULL, a wrong struct_size, NULL pointers
 * (out, y, result, workspace), n < 1, hop_length < 1, win_length < 0 or > PWV_SCORE_MAX_WIN, rows < 0 or beyond int32, T < 0 or
 * n T > rows in the uniform form, workspace_bytes too small.
 * ------------------------------------------------------------------------------------- */
#define PWV_SCORE_MAX_WIN 1024   /* the largest win_length (fft_length <= 1024: the frames and the twiddles of a workgroup stay in 35 KiB of LDS) */
#define PWV_SCORE_TILE 1024      /* samples per L1 partial */
typedef struct pwv_score_args {
    size_t struct_size;                    /* = sizeof(pwv_score_args) as the caller was compiled */
    const float* out;                      /* device [rows]: the predictions */
    const float* y;                        /* device [rows]: the ground truth, laid out as `out` */
    const int32_t* cu_rows;                /* device [n + 1], or NULL for the uniform form */
    int32_t n;                             /* utterances */
    int32_t T;                             /* samples per utterance (uniform form; ignored with cu_rows) */
    int64_t rows;                          /* samples `out` and `y` hold: the capacity */
    int32_t win_length, hop_length;
    double* result;                        /* device [n, 4] */
    void* workspace;                       /* device, pwv_score_workspace_bytes; need not be initialised */
    size_t workspace_bytes;
} pwv_score_args;
size_t pwv_score_workspace_bytes(const pwv_score_args* args);
int pwv_score_f32(const pwv_score_args* args, pwv_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PWV_HIP_SCORE_H */
