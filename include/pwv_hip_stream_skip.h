/* STREAMING WITH SKIP ACCUMULATION (model.use_skip_connection; DESIGN.md section 9, "Streaming the skip-connection architecture"): the
 * streaming layer launch of pwv_hip.h ("STREAMING") for layers that add o @ skip_w + skip_bias to an accumulator the head reads
 * (pwv_layer_args.skip, modules.py:243-250, :142-147).  The skip sum of row t of a chunk depends on row t's gated outputs alone: it
 * needs no history of its own, and the accumulator is a buffer of the CHUNK (N x T rows x 128, tile32).  The look-back rows come from
 * the session's history exactly as in pwv_wavenet_layer_stream_f32.  An EXTENSION of the C ABI in a header of its own: pwv_hip.h
 * (PWV_HIP_VERSION 301) is what it was, no struct of it changes; a client includes this header (which includes pwv_hip.h) and finds
 * the entry points in the same library.  Plain C99. */
#ifndef PWV_HIP_STREAM_SKIP_H
#define PWV_HIP_STREAM_SKIP_H

#include "pwv_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------
 * The causal layer of a chunk (modules.py:179-180, filter width 2, 64 channels, no bias): pwv_iaf_front_f32 with s == NULL for N
 * sessions x T rows, except that x[-1] of session n is not zero but the ONE float at hist->scalar_off of the block the session reads,
 * and x[T-1] is stored there in the block it writes.  h[g] (tile32, N*T rows x 64) gets the front's own bits: the one-shot forward of
 * a skip model never rebuilds the causal layer inside layer 0 (pwv_layer_args.x_first excludes skip accumulation, and the folded form
 * rounds differently), it runs layer 0 on these rows -- so the stream does too, and layer 0 keeps a ROW history like every other layer.
 * Reads of `hist`: struct_size, hist_rd, hist_wr, block_stride, slot_tab, scalar_off.  PWV_EINVAL: a NULL pointer, G outside
 * [1, PWV_MAX_NETS], N or T < 1, hist->cu_rows, a scalar that leaves its block.
 * ------------------------------------------------------------------------------------- */
int pwv_iaf_front_stream_f32(const float* x, int G, const float* const* filt, float* const* h, int N, int T,
                             const pwv_stream_args* hist, pwv_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * One layer of all the nets of a flow on one chunk of N sessions x T rows, with skip accumulation, in one of two forms:
 *   a residual layer  x_in -> x_out, out_mode PWV_OUT_RESIDUAL (layer 0 included: x_in = the rows of pwv_iaf_front_stream_f32)
 *   the last layer    out_mode PWV_OUT_GATED: x_out receives the gated output o, which nothing reads -- what pwv_wavenet_stack_f32
 *                     does for this layer, so that its skip contribution has the one-shot bits
 * and in both: skip[g] (+)= o @ skip_w + skip_bias on the chunk's accumulator (tile32, N*T rows x 128; skip_init = 1 for layer 0, as in
 * pwv_layer_args); reads and writes the row history at hist->row_off[g].  pwv_wavenet_head_f32 with PWV_HEAD_IN_SKIPSUM -- row-local,
 * the ordinary launch -- runs behind the last layer.  args->packed is a layer packed with_skip = 1.  Every row goes through the
 * instructions of pwv_wavenet_layer_f32 with the same skip in their order, the accumulator is read and written in layer order (no
 * atomics): the chunks of a session concatenate to the one-shot result bit for bit.  The history fields of `hist`, the slot table and
 * pwv_stream_carry_f32 are those of pwv_hip.h.
 *
 * Refused with PWV_EINVAL before a device is touched, pwv_last_error naming the reason: args NULL; a struct_size of `hist` that does
 * not cover the history fields; a NULL history or slot table; hist->cu_rows (no packed form); PWV_PREC_F16; args->skip[g] NULL; a
 * per-sample condition (cond / cond_channels); a fused head (args->head_packed); x_first / first_fold (no layer-0 form: see above); a
 * row history that leaves its block or two nets' histories that overlap.
 * ------------------------------------------------------------------------------------- */
int pwv_wavenet_layer_stream_skip_f32(const pwv_layer_args* args, const pwv_stream_args* hist, pwv_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PWV_HIP_STREAM_SKIP_H */
