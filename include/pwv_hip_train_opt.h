/* The OPTIMISER of training over a gradient ARENA: all gradients of a step packed into one flat float32 buffer (one collective for a
 * replicated trainer instead of one per tensor), and TensorFlow's Adam followed by the reference's EMA (models.py:72-76, :101-103) as ONE
 * launch over that buffer.  An EXTENSION of the C ABI in a header of its own: pwv_hip.h (PWV_HIP_VERSION 301) and every other header are
 * what they were; a client includes this header and finds the three entry points in the same library.  Plain C99.
 *
 * THE ARENA.  n tensors, tensor i of count_i >= 1 floats at float offset off_i of a flat float32 buffer; every off_i is a multiple of 4 (so
 * that a tensor begins on a 16-byte line of a 16-byte-aligned arena) and off_i + count_i <= arena_floats.  The up to 3 floats between the
 * end of a tensor and the next multiple of 4 are PADDING: no entry point here ever writes them, so padding that starts zero stays zero.
 * Gradients, Adam's m and v and the EMA shadows are four such buffers with ONE layout; the variables stay the separate tensors they are and
 * are reached through a table of pointers.
 *
 * THE TABLES.  `table` is n records of PWV_TRAIN_OPT_REC int64: { address of the tensor (device float*, 4-byte aligned), off_i, count_i }.
 * `block_map` is `blocks` records of two int32: { tensor index i, chunk c }, and stands for the floats c * PWV_TRAIN_OPT_CHUNK ..
 * min(count_i, (c + 1) * PWV_TRAIN_OPT_CHUNK) - 1 of tensor i; a layout lists every chunk of every tensor once (the library does not ask
 * for that: a call touches what its map names).  Both are built on the host once per layout and passed twice: `table` / `block_map` on the
 * device for the kernels, `table_host` / `block_map_host` with the same contents on the host, which is what the refusals read.
 *
 * Each launch: min(blocks, PWV_TRAIN_OPT_MAX_GRID) workgroups of 256 lanes that loop over the map; a lane owns 4 consecutive floats of a
 * chunk, 16 bytes per array.  Arena accesses are 16-byte vector loads and stores; so are the tensor's where its address is 16-byte aligned,
 * and four scalar ones where it is not; the last count_i % 4 floats of a tensor go one by one on both sides.  No atomics, no LDS.  The calls
 * only enqueue on `stream`.
 *
 * Refused with PWV_EINVAL before a device is touched, pwv_last_error naming the field: args NULL, a wrong struct_size, a NULL pointer the
 * entry needs (table, block_map, table_host, block_map_host, arena / grad, m, v; shadow when decay >= 0), an arena pointer that is not
 * 16-byte aligned, n < 1, blocks < 1, arena_floats < 1, a record with a NULL or misaligned tensor address, an offset that is negative or no
 * multiple of 4, a count < 1, a tensor that overruns the arena (off + count > arena_floats), a map record whose tensor index is outside
 * 0 .. n - 1 or whose chunk begins behind its tensor's end; and for pwv_train_opt_adam_ema_f32 a non-finite lr_t, eps or grad_scale, eps < 0,
 * beta1 or beta2 outside [0, 1), decay >= 1 (or NaN).  */
#ifndef PWV_HIP_TRAIN_OPT_H
#define PWV_HIP_TRAIN_OPT_H

#include "pwv_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PWV_TRAIN_OPT_REC 3          /* int64 per record of `table` */
#define PWV_TRAIN_OPT_CHUNK 1024     /* floats per record of `block_map`: 256 lanes x 4 */
#define PWV_TRAIN_OPT_MAX_GRID 2048  /* workgroups of a launch at most: 8 per compute unit of an MI355X */

/* ---------------------------------------------------------------------------------------
 * pwv_train_opt_pack_f32:   arena[off_i + e] = tensor_i[e]   for every float e the map names.
 * pwv_train_opt_unpack_f32: tensor_i[e] = arena[off_i + e]   (the inverse; the arena is only read).
 * Copies of bits: NaNs and signed zeros arrive as they were.
 * ------------------------------------------------------------------------------------- */
typedef struct pwv_train_opt_pack_args {
    size_t struct_size;                    /* = sizeof(pwv_train_opt_pack_args) as the caller was compiled */
    const int64_t* table;                  /* device [n, PWV_TRAIN_OPT_REC] */
    const int32_t* block_map;              /* device [blocks, 2] */
    const int64_t* table_host;             /* host, the same contents */
    const int32_t* block_map_host;         /* host, the same contents */
    float* arena;                          /* device [arena_floats], 16-byte aligned */
    int64_t arena_floats;
    int32_t n, blocks;
} pwv_train_opt_pack_args;

int pwv_train_opt_pack_f32(const pwv_train_opt_pack_args* args, pwv_stream_t stream);
int pwv_train_opt_unpack_f32(const pwv_train_opt_pack_args* args, pwv_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * pwv_train_opt_adam_ema_f32: one step of tf.train.AdamOptimizer on the n tensors of `table` (the VARIABLES, updated in place), then the
 * reference's EMA of the UPDATED variables.  The doubles are rounded to float32 once on the host,
 *   b1 = f32(beta1), c1 = f32(1 - beta1), b2 = f32(beta2), c2 = f32(1 - beta2), lr = f32(lr_t), e = f32(eps), s = f32(grad_scale),
 *   d = f32(1 - decay)                                     (the differences formed in float64, then rounded),
 * and every element then goes through exactly these float32 operations, each rounded to nearest-even on its own (no operation is fused
 * with another: round-to-nearest multiplies, adds and subtractions compiled with fp contract(off) -- what __fmul_rn / __fadd_rn promise --,
 * IEEE division, correctly rounded sqrtf), in this order:
 *   g      = s * grad[i]                                   (grad_scale: the 1 / world of a SUM all-reduce; 1 changes nothing)
 *   m      = (b1 * m) + (c1 * g)
 *   v      = (b2 * v) + ((c2 * g) * g)
 *   var    = var - ((lr * m) / (sqrt(v) + e))              (TensorFlow's epsilon, outside the root)
 *   shadow = shadow - (d * (shadow - var))                 (of the updated var; skipped when decay < 0)
 * so the result is a function of the inputs alone -- the same bits on every replica, whatever the grid -- and it is what the same
 * statements give in numpy float32.  lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t) is the caller's (float64).  grad is only read; m, v (and
 * shadow) are read and written at the arena offsets of the table, the variables through their addresses.  decay < 0: no EMA, `shadow` is
 * not touched and may be NULL.
 * ------------------------------------------------------------------------------------- */
typedef struct pwv_train_opt_adam_args {
    size_t struct_size;                    /* = sizeof(pwv_train_opt_adam_args) as the caller was compiled */
    const int64_t* table;                  /* device [n, PWV_TRAIN_OPT_REC]: the variables */
    const int32_t* block_map;              /* device [blocks, 2] */
    const int64_t* table_host;             /* host, the same contents */
    const int32_t* block_map_host;         /* host, the same contents */
    const float* grad;                     /* device [arena_floats], 16-byte aligned: the gradient arena */
    float* m;                              /* device [arena_floats], 16-byte aligned */
    float* v;                              /* device [arena_floats], 16-byte aligned */
    float* shadow;                         /* device [arena_floats], 16-byte aligned; may be NULL when decay < 0 */
    int64_t arena_floats;
    int32_t n, blocks;
    double lr_t, beta1, beta2, eps;
    double decay;                          /* the EMA's decay in [0, 1); < 0: no EMA */
    double grad_scale;
} pwv_train_opt_adam_args;

int pwv_train_opt_adam_ema_f32(const pwv_train_opt_adam_args* args, pwv_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PWV_HIP_TRAIN_OPT_H */
