/* The LIVE tick of libpwv_hip.so -- the streaming mel front-end inside a captured ragged streaming tick: wav chunks in, the sessions' next
 * samples out, one graph launch.  An EXTENSION of the C ABI, declared in a header of its own: pwv_hip.h (52 entry points,
 * PWV_HIP_VERSION 301) and pwv_hip_mel_stream.h (one entry point) are what they were; a client includes this header (which includes
 * pwv_hip_mel_stream.h) and finds pwv_live_tick_mel and pwv_live_tick_commit in the same library.  Plain C99. */
#ifndef PWV_HIP_LIVE_TICK_H
#define PWV_HIP_LIVE_TICK_H

#include "pwv_hip_mel_stream.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------
 * A LIVE tick = the CAPACITY form of pwv_wav_to_mel_db_stream_f32 at the head of a ragged streaming tick (pwv_hip.h, "A RAGGED
 * streaming tick") and a front-end commit at its end:
 *
 *   [staging copies]  pwv_live_tick_mel  pwv_stream_tick_ragged_begin  sampler  unit map  the push  pwv_stream_tick_ragged_commit
 *   pwv_live_tick_commit
 *
 * Both calls take the same struct and launch one kernel each whose grid depends on N, mel_rows and nothing else, so they are captured
 * once and replayed for any tick that fits: everything a tick decides reaches them through device memory.
 *   sess      the FRONT-END session table, int64 [n_slots, 4] = {generation, samples received, frames emitted, over}: session s reads
 *             state block 2 s + generation and writes block 2 s + 1 - generation (the record does not say which).
 *   rec       the tick's N records of PWV_LIVE_TICK_REC int64, written by the host before every replay (READY / FINISH / CARRY rules
 *             of pwv_hip_mel_stream.h):
 *               [0] absolute index of the carry's first sample (c)   [1] carry length              [2] offset of its chunk in `wav`
 *               [3] chunk length                                     [4] first frame to emit        [5] number of frames to emit
 *               [6] final length L (the utterance ENDS with this chunk), or -1                      [7] its slot
 *               [8] flags: 1 = active (else the record is skipped), 2 = the utterance STARTS with this chunk (no carry is read, the
 *                   session's counters and maximum are set, not advanced), 4 = its first frame of this tick goes to row [11] of
 *                   `first` (the vocoder side of the session starts in this tick) and the others to rows [9] ...
 *               [9] first row of its frames in `mel`                 [10] c after the tick (L = -1)  [11] its row of `first`
 *   mel       pwv_live_tick_mel: one workgroup per frame and one per carry; a workgroup without a frame or a carry leaves at once.
 *             A frame is the frame of pwv_wav_to_mel_db_f32 on the whole utterance, bit for bit (csrc/pwv_mel_frame_body.inc), and
 *             goes straight to its row of the ragged tick's `mel` (or `first`).  The largest raw dB of record i's frames goes to
 *             scratch[i] (order-preserving key, atomic max), not to the session's word.  EVERY index the kernel derives from a record
 *             is clamped to what the call was given: a stale record -- of a tick behind a refused one -- stays inside the buffers.
 *   commit    pwv_live_tick_commit, ONE workgroup, reads the two sticky words (give-up, range) once.  Both zero: every active record's
 *             session flips its generation; received += chunk length and emitted += frames (a start: set; an end: both 0);
 *             max_key[slot] = max(max_key[slot], scratch[i]) (a start: = scratch[i]); if that exceeds the key of limit_db the
 *             session's `over` becomes 1 (sticky: the host clears it); an end then puts the word back to INT32_MIN.  Otherwise
 *             nothing of the sessions changes.  Either way scratch[0 .. N - 1] is INT32_MIN afterwards.
 * rec_host, when not NULL, is the host's copy of `rec`: the call is checked against it.
 * Refused with PWV_EINVAL before a device is touched, pwv_last_error naming the field: NULL tables (window, mel_basis, mel, state,
 * max_key, scratch, sess, rec, words; wav with wav_cap > 0; first with n_first > 0), struct_size short, n_fft odd or > 2048, hop < 1,
 * max_db == min_db, N or n_slots < 1, and every active record of rec_host whose chunk leaves wav_cap, whose rows leave mel_rows, whose
 * slot has no blocks (outside n_slots), whose `first` row or scratch word is outside n_first / N, whose carry exceeds n_fft or whose
 * final length is not above n_fft / 2.
 * ------------------------------------------------------------------------------------- */
#define PWV_LIVE_TICK_REC 12
typedef struct pwv_live_tick_args {
    size_t struct_size;                    /* = sizeof(pwv_live_tick_args) as the caller was compiled */
    const float* wav;                      /* device [wav_cap]: the tick's chunks, packed */
    const float* window;                   /* device [n_fft] */
    const float* mel_basis;                /* device [n_mels, 1 + n_fft / 2] */
    float* mel;                            /* device [mel_rows, n_mels]: the ragged tick's mel */
    float* first;                          /* device [n_first, n_mels]: the ragged tick's first frames of starting entries */
    float* state;                          /* device [2 n_slots, n_fft]: the carries */
    int32_t* max_key;                      /* device [n_slots] */
    int32_t* scratch;                      /* device [N]: the tick's maxima, INT32_MIN between ticks */
    int64_t* sess;                         /* device [n_slots, 4] */
    const int64_t* rec;                    /* device [N, PWV_LIVE_TICK_REC] */
    const int64_t* rec_host;               /* host [N, PWV_LIVE_TICK_REC] or NULL */
    const int32_t* words;                  /* the two sticky words the ragged tick's commit reads */
    int64_t wav_cap, mel_rows;
    int32_t N, n_slots, n_first, n_fft, hop, n_mels;
    float amin, max_db, min_db;            /* as pwv_mel_stream_args */
    float limit_db;                        /* min_db + top_db: a session whose largest raw dB exceeds it is marked `over` */
} pwv_live_tick_args;
int pwv_live_tick_mel(const pwv_live_tick_args* args, pwv_stream_t stream);
int pwv_live_tick_commit(const pwv_live_tick_args* args, pwv_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PWV_HIP_LIVE_TICK_H */
