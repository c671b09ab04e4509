/* The streaming mel front-end of libpwv_hip.so: an EXTENSION of the C ABI of pwv_hip.h, declared in a header of its own.
 * pwv_hip.h, its 52 entry points and PWV_HIP_VERSION (301) are what they were; a client that streams the front-end includes this
 * header (which includes pwv_hip.h) and finds pwv_wav_to_mel_db_stream_f32 in the same library.  Plain C99. */
#ifndef PWV_HIP_MEL_STREAM_H
#define PWV_HIP_MEL_STREAM_H

#include "pwv_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------
 * STREAMING the mel front-end: wav chunks in, the frames of pwv_wav_to_mel_db_f32 (normalise != 0) on the whole utterance out, bit
 * for bit -- both kernels include one text of the frame arithmetic (csrc/pwv_mel_frame_body.inc) and differ in the sample fetch only.
 * h = n_fft / 2; R = the samples a session has received; L = the utterance's final length.
 *   What a frame reads   frame k reads samples t = k hop - h .. k hop + h - 1; t < 0 is read at -t; t >= L at 2 (L - 1) - t, clamped.
 *   READY rule    a frame is emitted as soon as every sample it reads has arrived, no right mirror involved: frame 0 at R >= h + 1
 *                 (its left mirror reads sample h), frame k >= 1 at R >= k hop + h.  K(R) = 0 for R < h + 1, else 1 + (R - h) / hop
 *                 frames are ready; a push emits frames K(R before) .. K(R after) - 1, possibly none.
 *   FINISH rule   finishing fixes L = R and emits frames K(L) .. L / hop -- 1 + L / hop in all, as the one-shot --, the right mirror
 *                 taken at L.  L <= h is refused, as by the one-shot.
 *   CARRY rule    between pushes a session keeps samples c .. R - 1, c = max(0, min(K(R) hop - h, R - h - 1)): every sample a later
 *                 frame can read, pushed or finishing at any later L (the h + 1 newest among them: a right mirror's reach).  That is
 *                 fewer than n_fft samples; a state block is n_fft floats, a session owns two (a push reads one, writes the other).
 *   top_db        the one-shot clips raw dB at max(utterance) - top_db before normalising, which changes nothing while that floor
 *                 is <= min_db.  The streaming form applies NO floor; it keeps the largest raw dB of a session in max_key[word] as
 *                 an order-preserving integer (key = bits >= 0 ? bits : bits ^ 0x7fffffff of the float, atomic max; the caller sets
 *                 the word to INT32_MIN when an utterance begins).  A session whose maximum exceeds min_db + top_db has frames that
 *                 are NOT the one-shot's: the caller checks.
 * One call = one ragged push: N sessions, session i described by record i of PWV_MEL_STREAM_REC int64:
 *   [0] absolute index of the carry's first sample (c)   [1] carry length                 [2] offset of its chunk in `wav`
 *   [3] chunk length (0: finishing)                      [4] first frame to emit           [5] number of frames to emit
 *   [6] final length L, or -1 while the utterance goes on  [7] state block read           [8] state block written (!= [7])
 *   [9] first row of its frames in `mel`                 [10] c after the push (L = -1)    [11] its word of max_key
 * given twice: `rec` on the device for the kernel, `rec_host` on the host, from which the call is checked and sized -- nothing is read
 * back.  One launch: a workgroup per (frame, session) and one per session that writes the new carry.
 * Refused with PWV_EINVAL before a device is touched, pwv_last_error naming the field: NULL pointers (window, mel_basis, state, max_key,
 * rec, rec_host; wav with wav_len > 0; mel with mel_rows > 0), n_fft odd or > 2048, hop < 1, max_db == min_db, struct_size short, a
 * finishing record with final_len <= n_fft / 2 or != the samples received, and every record whose frames would read a sample
 * outside [c, R), whose chunk, rows, blocks or word leave wav_len, mel_rows, n_blocks or n_words.
 * ------------------------------------------------------------------------------------- */
#define PWV_MEL_STREAM_REC 12
typedef struct pwv_mel_stream_args {
    size_t struct_size;                    /* = sizeof(pwv_mel_stream_args) as the caller was compiled (as in pwv_persist_args) */
    const float* wav;                      /* device [wav_len]: the sessions' chunks, packed */
    const float* window;                   /* device [n_fft]: the analysis window, zero-padded to n_fft */
    const float* mel_basis;                /* device [n_mels, 1 + n_fft / 2] */
    float* mel;                            /* device [mel_rows, n_mels]: the emitted frames, packed in record order */
    float* state;                          /* device [n_blocks, n_fft]: the carries */
    int32_t* max_key;                      /* device [n_words] */
    const int64_t* rec;                    /* device [N, PWV_MEL_STREAM_REC] */
    const int64_t* rec_host;               /* host   [N, PWV_MEL_STREAM_REC], the same values */
    int64_t wav_len, mel_rows;
    int32_t N, n_fft, hop, n_mels;
    int32_t n_blocks, n_words;
    float amin, max_db, min_db;            /* amplitude floor (1e-5); the dB range that maps to [-1, 1] */
} pwv_mel_stream_args;
int pwv_wav_to_mel_db_stream_f32(const pwv_mel_stream_args* args, pwv_stream_t stream);


#ifdef __cplusplus
}
#endif

#endif /* PWV_HIP_MEL_STREAM_H */
