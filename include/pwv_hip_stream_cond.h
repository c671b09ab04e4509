/* STREAMING WITH A PER-SAMPLE CONDITION (model.cond_upsample_method 'transposed_conv'; DESIGN.md section 9, "Streaming transposed-conv
 * conditioning"): the streaming layer launch of pwv_hip.h ("STREAMING") for layers whose condition is a [N T, 80] tensor at sample rate
 * instead of a frame-rate projection.  The condition of row t of a chunk is row t of the chunk's `cond`: it enters the layer through
 * the 1x1 product cond[t] [gc_filter | gc_gate] and needs no history of its own; the look-back rows come from the session's history
 * exactly as in pwv_wavenet_layer_stream_f32.  An EXTENSION of the C ABI in a header of its own: pwv_hip.h (PWV_HIP_VERSION 301) is
 * what it was, no struct of it changes; a client includes this header (which includes pwv_hip.h) and finds the entry point in the same
 * library.  Plain C99. */
#ifndef PWV_HIP_STREAM_COND_H
#define PWV_HIP_STREAM_COND_H

#include "pwv_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------
 * One layer of all the nets of a flow on one chunk of N sessions x T rows, in one of three forms:
 *   layer 0       args->x_first + first_fold (the folded form), out_mode PWV_OUT_RESIDUAL; reads hist->scalar_off
 *   layer j >= 1  x_in -> x_out, out_mode PWV_OUT_RESIDUAL; reads and writes the row history at hist->row_off[g]
 *   the last      the same with out_mode PWV_OUT_GATED: x_out receives the gated output o (tile32, 64 channels), and
 *                 pwv_wavenet_head_f32 with PWV_HEAD_IN_GATED -- row-local, the ordinary launch -- runs behind it.  There is no fused
 *                 head here: filter|gate + skip + postprocess1 fill the 160 KB of LDS, the condition weights are 40 KB more.
 * args->cond is the chunk's condition in the form the one-shot per-sample kernels read (PWV_PREC_F32: tile32, 80 channels;
 * PWV_PREC_F16X3: the two planes of pwv_cond_split_f16), args->cond_channels = 80, args->packed a layer packed WITH the condition
 * weights (pwv_pack_layer_f32, cond_channels = 80), args->proj the bias-only row (cond_hop = 0).  Every row goes through the
 * instructions of pwv_wavenet_layer_f32 with the same cond in their order: the chunks of a session concatenate to the one-shot result
 * bit for bit.  The history fields of `hist`, the slot table and pwv_stream_carry_f32 are those of pwv_hip.h.
 *
 * Refused with PWV_EINVAL before a device is touched, pwv_last_error naming the reason: args NULL; a struct_size of `hist` that does
 * not cover the history fields; a NULL history or slot table; hist->cu_rows (no packed form); PWV_PREC_F16; skip accumulation
 * (args->skip); cond NULL; cond_channels other than 80; layer 0 without first_fold; a fused head (args->head_packed); a row or scalar
 * history that leaves its block or two nets' histories that overlap; PWV_OUT_GATED on layer 0.
 * ------------------------------------------------------------------------------------- */
int pwv_wavenet_layer_stream_cond_f32(const pwv_layer_args* args, const pwv_stream_args* hist, pwv_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PWV_HIP_STREAM_COND_H */
