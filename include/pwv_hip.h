/*
 * pwv_hip.h -- C ABI of libpwv_hip.so: the MI355X (gfx950) kernels of the IAF-WaveNet
 * student generation path of andabi/parallel-wavenet-vocoder.
 *
 * The reference has NO FFI / plugin interface for this path: it is Python calling stock
 * TensorFlow ops.  Each entry point below therefore cites the
 * reference *Python call site* (file:line in /root/reference) whose arithmetic it replaces.
 * The Python host (parallel-wavenet-vocoder_amd/{modules,models}.py) binds them with ctypes;
 * INTEGRATION.md shows the stub a maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (never retained or freed here);
 *     tensors that cross the boundary (mel, z, waveform, weights, the inputs / outputs of the
 *     standalone ops) are float32, channels-last [N, T, C], weights in TensorFlow layout
 *     [width, Cin, Cout]; the scratch activations BETWEEN the fused kernels use the 32-row tiled
 *     layout "tile32" documented below;
 *   - `stream` is a hipStream_t passed as void*; every call only enqueues work on it
 *     (no hidden synchronisation, no internal streams or threads; re-entrant per stream);
 *   - return 0 on success, a negative PWV_E* code otherwise; pwv_last_error() returns a
 *     thread-local message for the last failing call on this thread;
 *   - "packed" buffers hold weights re-laid-out for the MFMA A-operand; their size comes
 *     from the matching pwv_*_packed_floats() call and their content from pwv_pack_*().
 */
#ifndef PWV_HIP_H_
#define PWV_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PWV_OK 0
#define PWV_EINVAL (-1)      /* bad argument / unsupported shape */
#define PWV_EHIP (-2)        /* HIP runtime error (message in pwv_last_error) */

#define PWV_MAX_NETS 2       /* nets evaluated side by side in one launch (scalar, shifter) */

/* arithmetic of the fused layer / head kernels */
#define PWV_PREC_F32 0       /* v_mfma_f32_32x32x2_f32: exact fp32 fma chains */
#define PWV_PREC_F16X3 1     /* 3-term split-fp16 MFMA (hi*hi + hi*lo + lo*hi), fp32 accumulate */
#define PWV_PREC_F16 2       /* BUILD EXTENSION (the reference is fp32 only): fp16 residual stream in HBM,
                              * one fp16 MFMA product, fp32 accumulate.  Activation buffers (x_in/x_out,
                              * buf0/buf1, head `in`, `cond`) then hold fp16 tile32 blocks as written by
                              * pwv_iaf_front_f16 / pwv_cond_to_f16 and are passed through the same
                              * pointer fields; P, net outputs and the waveform chain stay fp32.
                              * No skip accumulation.  ~1e-3 of the fp32 result, not 2e-5. */

typedef void* pwv_stream_t;

const char* pwv_last_error(void);
/* PWV_HIP_VERSION of the library that was loaded: major * 100 + minor.  A change of the major number changes the layout of an
 * argument struct: 3xx = pwv_persist_args begins with `struct_size`.  A client compiled against this header checks
 * pwv_version() / 100 == PWV_HIP_VERSION / 100 once after loading the library.  Fields appended to pwv_persist_args behind
 * `struct_size` (the packed-batch fields cu_rows ... varlen_rows among them) leave the number as it is: a shorter caller's
 * struct reads as zeros behind its end, i.e. as the behaviour it was compiled for. */
#define PWV_HIP_VERSION 301
int pwv_version(void);
/* number of compute units of the current device (grid sizing); <0 on error */
int pwv_device_cus(void);

/* ---------------------------------------------------------------------------------------
 * modules.causal_conv(value, filter_, dilation)                      modules.py:11-43
 *   y[n,t,:] = sum_k x[n, t-(W-1-k)*d, :] @ f[k],  x[t<0] = 0,  len(y) == len(x)
 *   x [N,T,Cin], f [W,Cin,Cout], y [N,T,Cout].  Any W, Cin, Cout, dilation >= 1.
 * ------------------------------------------------------------------------------------- */
int pwv_causal_conv_f32(const float* x, const float* filt, float* y,
                        int N, int T, int Cin, int Cout, int W, int dilation,
                        pwv_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * y[M,Nout] = act(x[M,K] @ w[K,Nout] + bias)   (bias may be NULL; relu: 0/1)
 * The 1x1 convolutions of the path that are plain GEMMs: cond `dense` (models.py:128-130),
 * each conv2d_transpose stage, whose kernel width == stride makes it a per-frame GEMM
 * (models.py:110-120), and the frame-rate projection of the condition through every layer's
 * gc_filter / gc_gate (+ filter_bias / gate_bias) (modules.py:216-228, hoisted).
 * K % 8 == 0, K <= 128, Nout % 4 == 0.
 * ------------------------------------------------------------------------------------- */
int pwv_linear_f32(const float* x, const float* w, const float* bias, float* y,
                   int M, int K, int Nout, int relu, pwv_stream_t stream);

/* same contract in split-fp16 arithmetic (3 fp16 MFMA products per term, fp32 accumulate, ~2^-22
 * relative per product: the arithmetic of PWV_PREC_F16X3); 5x fewer matrix-pipe cycles */
int pwv_linear_split_f32(const float* x, const float* w, const float* bias, float* y,
                         int M, int K, int Nout, int relu, pwv_stream_t stream);
/* The prologue of a 'repeat'-conditioned forward as ONE launch (PWV_PREC_F16X3 / PWV_PREC_F16 arithmetic of pwv_linear_split_f32):
 *   frames[M, C] = relu(mel[M, n_mels] @ dense[n_mels, C])                      models.py:128-130 (no bias)
 *   P[M, Nout]   = frames @ bank_w[C, Nout] + bank_b[Nout]                      the hoisted projections of modules.py:216-228
 *   *range_flag  = 1 if any mel value is non-finite or beyond `limit`           (range guard; range_flag may be NULL)
 * bit-identical to pwv_range_check_f32 + pwv_linear_split_f32 (relu) + pwv_linear_split_f32; n_mels, C multiples of 8, <= 80;
 * `frames` may be NULL when only P is wanted. */
int pwv_cond_project_f32(const float* mel, const float* dense, int n_mels, const float* bank_w, const float* bank_b, float* frames,
                         float* P, int M, int C, int Nout, float limit, int* range_flag, pwv_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * IAFVocoder._upsample_cond, 'repeat' branch: tile + reshape + crop   models.py:131-133
 *   out[n, t, :] = frames[n, (t + offset) / hop, :],  t in [0, T)
 *   frames [N, t_mel, C] (already relu(mel @ dense)), out [N, T, C].
 * ------------------------------------------------------------------------------------- */
int pwv_upsample_repeat_f32(const float* frames, float* out, int N, int t_mel, int C,
                            int T, int hop, int offset, pwv_stream_t stream);

/* out[n, t, :] = in[n, t + offset, :]  (the crop at models.py:124) */
int pwv_crop_time_f32(const float* in, float* out, int N, int T_in, int C, int T_out, int offset,
                      pwv_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Logistic(0,1).sample                                               models.py:32-33
 *   z = log(u) - log1p(-u),  u ~ U(0,1) from a counter-based generator keyed by
 *   (seed, element index + offset): reproducible and shardable.
 * ------------------------------------------------------------------------------------- */
int pwv_logistic_noise_f32(float* z, int64_t n, uint64_t seed, uint64_t offset, pwv_stream_t stream);
/* The same sampler for a launch that is CAPTURED into a HIP graph and replayed (arguments passed by value would repeat the counter
 * range).  state = four uint64 in DEVICE memory: {seed, offset, 0, skip}.  A launch draws z[i] = the sample of counter offset + i and
 * -- its last block to finish -- advances state[1] by n, so replay k draws what pwv_logistic_noise_f32(seed, offset + k*n) draws;
 * state[3] != 0: z is left as the caller filled it and nothing advances; state[2] is the launch's own ticket (zero between launches).
 * ONE launch per `state` in flight at a time: two launches that share a state must be ordered (one stream, or one graph replayed on
 * one stream) -- overlapping ones would share the ticket. */
int pwv_logistic_noise_stream_f32(float* z, int64_t n, uint64_t* state, pwv_stream_t stream);
/* The sampler of a PACKED batch (n utterances, rows = cu_rows[n] rows) with one counter stream per utterance, read from DEVICE memory:
 *   cu_rows  device int32 [n+1], cu_rows[0] = 0, ascending, cu_rows[n] = rows (the prefix sums of pwv_persist_args.cu_rows)
 *   streams  device uint64 [n][2] = {seed_i, offset_i}
 * Row r of utterance i (cu_rows[i] <= r < cu_rows[i+1]) gets the sample of counter offset_i + (r - cu_rows[i]) under seed_i, so
 * z[cu_rows[i] .. cu_rows[i+1]) is BIT-IDENTICAL to what pwv_logistic_noise_f32(z_i, len_i, seed_i, offset_i) writes: an utterance's noise
 * depends on its own stream only, not on its companions or its position.  Nothing is read on the host, so a captured launch replays
 * with whatever tables the caller wrote before the replay.  Any n (binary search per row); rows <= 2^31 - 1; vector stores only. */
int pwv_logistic_noise_packed_f32(float* z, const int32_t* cu_rows, const uint64_t* streams, int32_t n, int64_t rows,
                                  pwv_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Range guard of the split-fp16 arithmetic (PWV_PREC_F16X3).  The reference computes in fp32 (models.py:81-82);
 * the split-fp16 kernels convert GEMM operands to fp16 hi/lo pairs, which keeps fp32's ~22-bit products but has
 * fp16's EXPONENT range: an operand beyond 65504 would become inf where fp32 is fine.  The host bounds every GEMM
 * operand from the weights (pack time) and from two run-time maxima -- the flow input and the mel input -- which
 * the kernels check against the limits the host derived:
 *   pwv_range_flag(&p)      process-wide sticky int32 in pinned, device-visible host memory (0 = in range);
 *                           the host reads it after any synchronisation, no device -> host copy needed.
 *   pwv_range_check_f32     sets *flag = 1 when any x[i] is non-finite or |x[i]| > limit.
 * A raised flag means: the result of that forward is not trustworthy in PWV_PREC_F16X3 -- rerun it in
 * PWV_PREC_F32 (the Python host raises PwvRangeError / reruns).
 * ------------------------------------------------------------------------------------- */
int pwv_range_flag(int** flag);
/* A caller's OWN pair of sticky words in pinned, device-visible host memory (both zero): words[0] for pwv_persist_args.status,
 * words[1] as the range flag of any entry point that takes one.  One pair per (device, stream) or per thread keeps concurrent
 * callers apart (the process-wide words above are shared by everybody who does not bring their own).  Free with
 * pwv_status_words_free when no launch that was handed them can still be running. */
int pwv_status_words_alloc(int** words);
int pwv_status_words_free(int* words);
int pwv_range_check_f32(const float* x, int64_t n, float limit, int* flag, pwv_stream_t stream);
/* pack-time statistics of one layer (R = D = 64, S = 128; TF layouts) for the host's bound on the residual stream:
 * out8 = max|filter|, max|gate|, max|dense|, max|skip|, max|gc_filter|, max|gc_gate| (0 when NULL),
 *        max_out sum_in |dense| + max|dense_bias|, max_out sum_in |skip| + max|skip_bias|;  C = rows of gc_* */
int pwv_range_stats_f32(const float* filter, const float* gate, const float* dense, const float* dense_bias, const float* skip,
                        const float* skip_bias, const float* gc_filter, const float* gc_gate, int C, float* out8, pwv_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * "tile32": the layout of every [rows = N*T, C] ACTIVATION buffer the fused kernels below read or
 * write (residual stream C = 64, skip sums C = 128, per-sample condition C = 80).  Rows are stored
 * in blocks of 32; block u holds rows 32u..32u+31 as [C/4 channel quads][32 rows][4 floats]:
 *     float index of (row, c) = (row/32)*32*C + (c/4)*128 + (row%32)*4 + c%4
 * so that a wavefront (32 rows, lane (t,h) owning channel quads 2g+h) moves 1 KB of contiguous
 * memory per vector load / store.  Buffers hold pwv_tile32_floats(rows, C) floats (whole blocks).
 * These are scratch buffers between pwv_iaf_front_f32 and pwv_wavenet_head_f32; the converters are
 * for callers that bring their own channels-last tensors (multi-channel input, per-sample condition).
 * ------------------------------------------------------------------------------------- */
size_t pwv_tile32_floats(int64_t rows, int C);
int pwv_rows_to_tile32_f32(const float* in, float* out, int64_t rows, int C, pwv_stream_t stream);
int pwv_tile32_to_rows_f32(const float* in, float* out, int64_t rows, int C, pwv_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * LinearIAFLayer affine + the next flow's causal layer, fused.
 *   x[r] = z[r]*s[r*sb_stride] + b[r*sb_stride]          modules.py:59   (x = z if s == NULL)
 *   h_g[n,t,:] = sum_k x[n, t-(W-1-k), 0] * filt_g[k,0,:]  modules.py:179-180 (no bias)
 * z [N*T]; s, b strided views of the previous flow's net outputs; x_out [N*T] (may be NULL
 * when s == NULL); for g < G: filt[g] is [W,1,R], h[g] is a tile32 buffer of N*T rows x R channels
 * (see below).  G may be 0 (affine only).  W <= 8 and W*R <= 2048 (the filter is staged in LDS).
 * ------------------------------------------------------------------------------------- */
int pwv_iaf_front_f32(const float* z, const float* s, const float* b, int sb_stride,
                      float* x_out, int G, const float* const* filt, float* const* h,
                      int N, int T, int W, int R, pwv_stream_t stream);

/* PWV_PREC_F16 front end: same arithmetic as pwv_iaf_front_f32 (R == 64, G >= 1) but h16[g] is an fp16
 * tile32 buffer: block u = rows 32u..32u+31 as [8 chunks][32 rows][8 halfs]; chunk s*2+h, half q holds
 * channel 16s + 8(q>>2) + 4h + (q&3) (the order the MFMA B operand consumes);
 * pwv_tile32_floats(rows, 64) HALFS. */
int pwv_iaf_front_f16(const float* z, const float* s, const float* b, int sb_stride,
                      float* x_out, int G, const float* const* filt, void* const* h16,
                      int N, int T, int W, int R, pwv_stream_t stream);

/* PWV_PREC_F16: per-sample condition [N,T,80] fp32 channels-last (models.py:110-124) -> fp16 tile32
 * (10 chunks per row, same channel order), pwv_tile32_floats(rows, 80) halfs */
int pwv_cond_to_f16(const float* cond, void* out16, int N, int T, int C, pwv_stream_t stream);

/* PWV_PREC_F16X3: the same conversion plus the `lo` plane fp16(v - fp16(v)) stored behind the `hi` plane
 * (2 x pwv_tile32_floats(rows, 80) halfs in total): the split-fp16 layer kernel reads both operands of its
 * condition GEMM from these planes (the condition is constant over the 120 net-layers of a forward, so it is
 * split once instead of 120 times) */
int pwv_cond_split_f16(const float* cond, void* out16, int N, int T, int C, pwv_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Fused gated-residual layer: WaveNet._create_dilation_layer          modules.py:185-259
 * for R = D = 64, S = 128, filter_width 2 (hparams/default.yaml:22-25), G <= 2 nets per launch.
 *
 *   F‖G = [x[t-d] ‖ x[t]] @ [[filter0‖gate0],[filter1‖gate1]] + P[frame(t)]   (+ cond[t] @ gc)
 *   o   = tanh(F) * sigmoid(G)                                                  modules.py:236
 *   out = x[t] + o @ dense + dense_bias        (out_mode PWV_OUT_RESIDUAL)     modules.py:239-251
 *   out = o                                    (out_mode PWV_OUT_GATED: last layer -> head)
 *   skip (+)= o @ skip_w + skip_bias           (when skip != NULL)              modules.py:243-250
 *
 * P is the frame-rate projection of the condition through gc_filter‖gc_gate plus
 * filter_bias‖gate_bias, in the kernel's column order (pwv_proj_column_map); the row used by
 * sample t of utterance n is  n*cond_frames + (t + cond_offset)/cond_hop  (cond_hop == 0:
 * always row 0, i.e. biases only / no conditioning).  `cond` (per-sample condition, 80 channels,
 * transposed-conv upsampling) is NULL in hoisted mode; its form depends on `precision`: fp32 tile32
 * (PWV_PREC_F32), pwv_cond_split_f16 planes (PWV_PREC_F16X3), pwv_cond_to_f16 blocks (PWV_PREC_F16).
 * ------------------------------------------------------------------------------------- */
#define PWV_OUT_RESIDUAL 0
#define PWV_OUT_GATED 1

/* floats of one layer's packed buffer; with_skip / with_cond select optional sections */
size_t pwv_layer_packed_floats(int with_skip, int cond_channels);

/* gather TF-layout weights (device) into the packed layout (device).
 * filter, gate [2,64,64]; dense [1,64,64]; dense_bias [64] or NULL;
 * skip [1,64,128] + skip_bias [128]/NULL when with_skip; gc_filter, gc_gate [1,C,64] when
 * cond_channels > 0 (per-sample conditioning). */
int pwv_pack_layer_f32(const float* filter, const float* gate, const float* dense,
                       const float* dense_bias, const float* skip, const float* skip_bias,
                       const float* gc_filter, const float* gc_gate, int with_skip,
                       int cond_channels, int precision, float* packed, pwv_stream_t stream);

/* column order of P: map[col] = channel index into [filter(0..63) ‖ gate(64..127)] */
int pwv_proj_column_map(int* map128);

/* One layer's 128 columns of the frame-rate projection operands, packed on the device:
 *   proj_w [C, 128*n_layers] (+ column 128*layer): gc_filter ‖ gc_gate [1,C,64] each, in the P column order, pre-multiplied by
 *   the exp2 scales of the gate (-2 log2 e for filter columns, -log2 e for gate columns); proj_b [128*n_layers]: the same
 *   for filter_bias ‖ gate_bias [64] (zeros when NULL).  gc_* may be NULL (no conditioning: only proj_b is written).
 *   P = frames @ proj_w + proj_b is then one pwv_linear_*_f32 call per net (modules.py:216-228, hoisted to frame rate). */
int pwv_pack_proj_f32(const float* gc_filter, const float* gc_gate, const float* filter_bias, const float* gate_bias, int C,
                      int layer, int n_layers, float* proj_w, float* proj_b, pwv_stream_t stream);

typedef struct pwv_layer_args {
    int G;                                 /* nets in this launch (1 or 2) */
    const float* x_in[PWV_MAX_NETS];       /* tile32, N*T rows x 64 */
    float* x_out[PWV_MAX_NETS];            /* tile32, N*T rows x 64 */
    const float* packed[PWV_MAX_NETS];     /* pwv_pack_layer_f32 output */
    const float* proj[PWV_MAX_NETS];       /* P rows for THIS layer (128 floats each) */
    int proj_row_stride;                   /* floats between consecutive P rows */
    const float* cond;                     /* per-sample condition in the form `precision` wants, or NULL */
    int cond_channels;                     /* 0 or 80 */
    float* skip[PWV_MAX_NETS];             /* tile32, N*T rows x 128: accumulators, or NULL */
    int skip_init;                         /* 1: skip = ..., 0: skip += ... */
    int N, T, dilation;
    int cond_hop, cond_offset, cond_frames;
    int out_mode;                          /* PWV_OUT_RESIDUAL / PWV_OUT_GATED */
    int precision;                         /* PWV_PREC_* */
    int max_workgroups;                    /* 0 = one per CU */
    /* Layer 0 of a scalar-input net without a materialised causal layer (PWV_PREC_F16X3 / PWV_PREC_F32, no skip accumulation,
     * filter width 2): when x_first != NULL, x_in is ignored and the kernel evaluates
     *     h[t] = x_first[t-1] * causal_filter[0,0,:] + x_first[t] * causal_filter[1,0,:]      modules.py:179-180
     * for rows t and t-d itself, with the operations (and bits) of pwv_iaf_front_f32: 4 B instead of 768 B of
     * traffic per sample for this layer and no front launch.  x_first is [N*T] float32 (the flow's input). */
    const float* x_first;
    const float* causal_filter[PWV_MAX_NETS];   /* [2,1,64] each */
    /* optional, with x_first: pwv_pack_first_fold_f16x3's (PWV_PREC_F16X3, PWV_PREC_F16) / _f32's (PWV_PREC_F32) output per net (all or none).  Layer 0's
     * filter|gate convolution then runs on the four scalars x[t-d-1], x[t-d], x[t-1], x[t] themselves -- one MFMA k-step
     * instead of eight: the same function (h[t] is linear in x[t-1], x[t]), rounded differently: within the path's
     * tolerance of the unfolded form, not bit-identical to it.  pwv_persist_args.first_fold does exactly the same. */
    const float* first_fold[PWV_MAX_NETS];
    /* The LAST layer with the post-processing head fused behind it (PWV_PREC_F16X3 / PWV_PREC_F32, out_mode PWV_OUT_GATED, no skip
     * accumulation, no per-sample condition): when head_packed[g] != NULL the gated output stays in registers and
     * feeds pwv_wavenet_head_f32's arithmetic directly; head_out[g] receives [N,T,head_q]; x_out is not written. */
    const float* head_packed[PWV_MAX_NETS];     /* pwv_pack_head_f32 output */
    float* head_out[PWV_MAX_NETS];
    int head_q;
    /* PWV_PREC_F16X3 range guard (see pwv_range_check_f32): with x_first set and range_flag != NULL, layer 0 sets
     * *range_flag = 1 when a flow-input sample is non-finite or |x| > x_limit. */
    float x_limit;
    int* range_flag;
} pwv_layer_args;

int pwv_wavenet_layer_f32(const pwv_layer_args* args, pwv_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * STREAMING: the same layer on a CHUNK of a longer utterance                        modules.py:185-259 (the reference has no
 * chunked form: models.py:23-78 generates a whole utterance per sess.run; the call sites replaced are the layer's own)
 *
 * A launch of N x T rows continues N SESSIONS: utterance n's rows are the T samples that follow what the session has seen.  The
 * look-back x[t-d] of a row with t < d is not zero but the session's HISTORY of this layer's input, and the last d input rows of
 * the chunk are stored as the next history.  Every row then runs the instructions of pwv_wavenet_layer_f32 in their order: the
 * chunks of a session, concatenated, equal the one-shot launch BIT FOR BIT, whatever the chunk lengths (T < d included).  A history
 * of zeros is the one-shot left edge (a fresh session).
 *
 * History layout.  `hist_rd` / `hist_wr` point at arrays of BLOCKS, `block_stride` floats apart (a multiple of 4; the two may be one
 * array).  A block is one session's state in one generation; the caller chooses what goes where inside it:
 *   row history of a layer (dilation d, one per net): a tile32 buffer of round32(d) rows x 64 channels at float offset row_off[g]
 *       (a multiple of 4); row k (k < d) is the layer's input at chunk time k - d, i.e. row t < d of a chunk looks back at row t;
 *   scalar history of layer 0 (x_first; dilation d): d + 1 floats at float offset scalar_off; element k is x_first at chunk
 *       time k - (d + 1).
 * slot_tab  device int32 [N][2]: utterance n READS block slot_tab[2n] of hist_rd and WRITES block slot_tab[2n+1] of hist_wr.  The
 *       two must differ (a chunk with T < d reads rows a lane of the same launch would overwrite): keep two generations per session
 *       and flip after the chunk is accepted -- which also makes a chunk a transaction: until the flip, the chunk can be run again
 *       from the same state (the range-guard rerun in PWV_PREC_F32).
 * A chunk with T >= d rewrites all d rows of the written block.  With T < d the launch writes rows d-T .. d-1 only; rows 0 .. d-T-1
 * are the read block's rows T .. d-1 and are moved by pwv_stream_carry_f32 -- ONE launch per chunk for all layers of the model:
 *   carry_tab  device int32 [n_carry][4] = {float offset inside a block, rows, floats per row (64: a tile32 row history, 1: a
 *       scalar history), 0}: every history of the model; entries with rows <= T are left alone (the layer launches rewrite them).
 * The carry launch and the layer launches of a chunk write disjoint rows and read only `hist_rd` blocks: any order.
 *
 * The PACKED (ragged) form: sessions of DIFFERENT chunk lengths in one launch.  `cu_rows` (device int32 [N+1], prefix sums) gives session
 * n the rows cu_rows[n] .. cu_rows[n+1]-1 of a packed launch and T_n = cu_rows[n+1] - cu_rows[n] >= 32 samples.  Everywhere above, T is
 * then the session's OWN T_n: rows with t >= T_n - d store to row t + d - T_n of the written block, a chunk with T_n < d writes rows
 * d-T_n .. d-1, and the carry moves that session's rows T_n .. d-1.  Taken by pwv_wavenet_stack_persist_f32 (pwv_persist_args.hist
 * together with pwv_persist_args.cu_rows) and by pwv_stream_carry_f32 (its `T` argument is then not read; entries with rows <= T_n are
 * left alone for that session); pwv_wavenet_layer_stream_f32 returns PWV_EINVAL and names hist->cu_rows: the per-layer kernels have
 * no packed form.
 *
 * Supported: PWV_PREC_F32 / PWV_PREC_F16X3; no skip accumulation, no per-sample condition (PWV_EINVAL otherwise); three forms:
 *   layer 0 with x_first AND first_fold (out_mode PWV_OUT_RESIDUAL; uses scalar_off),
 *   a plain layer (out_mode PWV_OUT_RESIDUAL; uses row_off),
 *   the last layer with head_packed / head_out (out_mode PWV_OUT_GATED; uses row_off).
 * A frame-rate condition is indexed as in pwv_layer_args, relative to the chunk: a chunk that starts at a multiple of cond_hop brings
 * the T / cond_hop + 1 frames from its first sample's frame on.
 * ------------------------------------------------------------------------------------- */
typedef struct pwv_stream_args {
    size_t struct_size;                    /* = sizeof(pwv_stream_args) as the caller was compiled (as in pwv_persist_args) */
    const float* hist_rd;                  /* blocks the launch reads */
    float* hist_wr;                        /* blocks the launch writes */
    size_t block_stride;                   /* floats between two blocks */
    const int32_t* slot_tab;               /* device int32 [N][2] = {block read, block written} */
    size_t row_off[PWV_MAX_NETS];          /* this layer's row history, per net of the launch */
    size_t scalar_off;                     /* x_first: the scalar history */
    const int32_t* carry_tab;              /* pwv_stream_carry_f32 only */
    int32_t n_carry;
    const int32_t* cu_rows;                /* NULL: the uniform [N, T] chunk.  Else device int32 [N+1]: session n's chunk is rows cu_rows[n] .. cu_rows[n+1]-1
                                              of the packed launch (T_n = their difference) */
} pwv_stream_args;

int pwv_wavenet_layer_stream_f32(const pwv_layer_args* args, const pwv_stream_args* hist, pwv_stream_t stream);
int pwv_stream_carry_f32(const pwv_stream_args* hist, int N, int T, pwv_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * WaveNet post-processing head                                         modules.py:145-165
 *   total = o @ skip_w + skip_bias   (in_mode PWV_HEAD_IN_GATED: use_skip_connection False,
 *                                     only the last layer's skip is live, modules.py:147)
 *   total = skip_sum                 (in_mode PWV_HEAD_IN_SKIPSUM)
 *   y = relu(relu(total) @ post1 + b1) @ post2 + b2                    y [N,T,Q], Q <= 4
 * ------------------------------------------------------------------------------------- */
#define PWV_HEAD_IN_GATED 0
#define PWV_HEAD_IN_SKIPSUM 1

size_t pwv_head_packed_floats(int Q);
/* Layer 0 of a scalar-input net (W = 2 causal filter [2,1,64] in front of a [2,64,64] filter / gate pair, modules.py:174-183 and
 * :216-222) folded onto its four input scalars: 2048 floats (8 KB) of split-fp16 A fragments for pwv_persist_args.first_fold.
 * The fold is accumulated in fp64. */
#define PWV_FIRST_FOLD_FLOATS 2048
int pwv_pack_first_fold_f16x3(const float* causal_filter, const float* filter, const float* gate, float* folded, pwv_stream_t stream);
/* the same fold for PWV_PREC_F32 (two fp32 MFMA k-steps per row tile instead of 64): 1024 floats of `folded` are written */
int pwv_pack_first_fold_f32(const float* causal_filter, const float* filter, const float* gate, float* folded, pwv_stream_t stream);

/* skip [1,64,128], skip_bias [128]/NULL, post1 [1,128,128], post1_bias [128]/NULL,
 * post2 [1,128,Q], post2_bias [Q]/NULL */
int pwv_pack_head_f32(const float* skip, const float* skip_bias, const float* post1,
                      const float* post1_bias, const float* post2, const float* post2_bias,
                      int Q, int precision, float* packed, pwv_stream_t stream);

typedef struct pwv_head_args {
    int G;
    const float* in[PWV_MAX_NETS];         /* tile32: gated o (64 channels) or skip sum (128) */
    const float* packed[PWV_MAX_NETS];
    float* out[PWV_MAX_NETS];              /* [N,T,Q] */
    int N, T, Q;
    int in_mode;
    int precision;
    int max_workgroups;
} pwv_head_args;

int pwv_wavenet_head_f32(const pwv_head_args* args, pwv_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Whole dilated stack + head of G structurally identical nets in one call: the loop of
 * WaveNet.__call__ (modules.py:138-165) without a host round trip per layer.
 *   buf0[g] holds the causal layer's output on entry; buf0/buf1 ping-pong through the layers;
 *   out[g] receives the net output [N,T,Q].
 * With PWV_PREC_F16X3 or PWV_PREC_F32, no skip accumulation and no per-sample condition the head runs inside the last layer's
 * launch (pwv_layer_args.head_packed) unless `separate_head` is set.
 * streams[0] only (streams[1] == NULL): every layer is one launch covering all G nets.
 * Two streams and G == 2: net g's chain runs on streams[g] with `max_workgroups` workgroups per
 * launch (0 = half of the CUs), launches interleaved -- the two independent chains then hide each
 * other's launch gaps and tails.  The caller orders the streams against its own work.
 * ------------------------------------------------------------------------------------- */
typedef struct pwv_stack_args {
    int G;
    int n_layers;
    const int* dilations;                         /* HOST array [n_layers] */
    float* buf0[PWV_MAX_NETS];                    /* tile32, N*T rows x 64 */
    float* buf1[PWV_MAX_NETS];                    /* tile32, N*T rows x 64 */
    const float* packed_layers[PWV_MAX_NETS];     /* n_layers packed layer buffers, back to back */
    size_t packed_layer_stride;                   /* floats between consecutive layers */
    const float* proj[PWV_MAX_NETS];              /* P rows holding all layers: layer j at +128*j */
    int proj_row_stride;
    const float* cond;                            /* per-sample condition in the form `precision` wants, or NULL */
    int cond_channels;
    float* skip[PWV_MAX_NETS];                    /* tile32, N*T rows x 128, or NULL (use_skip_connection) */
    const float* packed_head[PWV_MAX_NETS];
    float* out[PWV_MAX_NETS];
    int Q;
    int N, T;
    int cond_hop, cond_offset, cond_frames;
    int precision;
    int max_workgroups;
    /* optional timing hooks (hipEvent_t, may be NULL): ev_begin[c] is recorded on chain c's stream in front of its
     * first layer launch, ev_end[c] behind its last RESIDUAL layer launch (layer n_layers-2) -- elapsed / (n_layers-1)
     * is the mean launch duration of the dominant kernel on the production launch path (bench.py's roofline).
     * One chain (c = 0) in single-stream mode, one per net with two streams. */
    void* ev_begin[PWV_MAX_NETS];
    void* ev_end[PWV_MAX_NETS];
    /* optional: layer 0 evaluates the causal layer itself (see pwv_layer_args.x_first); buf0 then only serves as the
     * ping-pong partner of buf1 and need not be initialised */
    const float* x_first;
    const float* causal_filter[PWV_MAX_NETS];
    int separate_head;                            /* 1: never fuse the head into the last layer's launch */
    float x_limit;                                /* forwarded to layer 0 (pwv_layer_args.x_limit / range_flag) */
    int* range_flag;
    const float* first_fold[PWV_MAX_NETS];        /* optional, forwarded to layer 0 (pwv_layer_args.first_fold) */
} pwv_stack_args;

int pwv_wavenet_stack_f32(const pwv_stack_args* args, pwv_stream_t const* streams);

/* ---------------------------------------------------------------------------------------
 * Normalisers (modules.normalize, modules.py:263-284) and the elementwise ops of the un-fused WaveNet path.
 *   pwv_instance_norm_f32   method 'in' (modules.py:274-284): per (utterance, channel) mean / biased variance over the
 *                           TIME axis, y = gamma (x - mean) / sqrt(var + eps) + beta, eps = 1e-8 in the reference;
 *                           x, y [N, T, C] channels-last; gamma / beta [C] or NULL; three launches (fp64 partial sums per
 *                           time chunk, no atomics: bitwise repeatable), workspace from pwv_instance_norm_workspace_bytes.
 *   pwv_channel_affine_f32  y = act(x * scale[c] + bias[c]) -- method 'bn' at inference (modules.py:266: scale =
 *                           gamma / sqrt(moving_variance + 1e-3), bias = beta - moving_mean * scale) where no GEMM follows
 *                           that the host could fold it into; also bias adds and relu.  scale / bias may be NULL;
 *                           tile32 != 0: x, y are tile32 buffers (C % 4 == 0); in place (x == y) allowed.
 *   pwv_add_f32, pwv_gate_f32   out = a + b;  out = tanh(f) * sigmoid(g) (modules.py:236).
 * ------------------------------------------------------------------------------------- */
size_t pwv_instance_norm_workspace_bytes(int N, int T, int C);
int pwv_instance_norm_f32(const float* x, float* y, int N, int T, int C, const float* gamma, const float* beta, float eps,
                          void* workspace, size_t workspace_bytes, pwv_stream_t stream);
int pwv_channel_affine_f32(const float* x, float* y, int64_t rows, int C, const float* scale, const float* bias, int tile32,
                           int relu, pwv_stream_t stream);
int pwv_add_f32(const float* a, const float* b, float* out, int64_t n, pwv_stream_t stream);
int pwv_gate_f32(const float* f, const float* g, float* out, int64_t n, pwv_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * wav -> (normalised) dB mel-spectrogram, the conditioning input of generate.py           data_load.py:51-54
 *   audio.wav2melspec_db (audio.py:341-356): |STFT| (librosa.stft: centred, reflect-padded; `window` is the analysis
 *   window already zero-padded to n_fft) -> mel_basis [n_mels, 1 + n_fft/2] (librosa.filters.mel, audio.py:241) ->
 *   amplitude_to_db (10 log10 max(amin^2, .^2), then clipped to top_db below the utterance maximum) -> if `normalise`:
 *   (clip((db - min_db) / (max_db - min_db), 0, 1) - 0.5) * 2  (audio.py:254-286).
 *   wav [N, L] -> mel [N, 1 + L/hop, n_mels]; fp64 accumulation inside; n_fft even, <= 2048.
 * ------------------------------------------------------------------------------------- */
int pwv_wav_to_mel_db_f32(const float* wav, const float* window, const float* mel_basis, float* mel, int N, int L, int n_fft,
                          int hop, int n_mels, float amin, float top_db, float max_db, float min_db, int normalise,
                          pwv_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * A run of consecutive RESIDUAL layers (out_mode PWV_OUT_RESIDUAL, no skip accumulation, no per-sample condition,
 * PWV_PREC_F16X3 or PWV_PREC_F32) of G nets as ONE persistent launch: the inner iterations of the loop in WaveNet.__call__
 * (modules.py:138-143) without a kernel boundary, a weight-staging phase and a ramp-up / ramp-down per layer.
 *   x_ring[g]  three full-size tile32 buffers (N*T rows x 64) per net, `ring_stride` floats apart (>= pwv_tile32_floats(N*T, 64)).
 *   Layer j of the run reads buffer (j + 2 + r) % 3 and writes buffer (j + r) % 3, r = ring_rotation: the input of the run is
 *   in buffer (2 + r) % 3 on entry, its output in buffer (n_layers - 1 + r) % 3 on return; the third buffer holds
 *   intermediate layers (a stack can be cut into several runs that hand the ring on: r' = (output buffer + 1) % 3).  Layer j reads
 *   packed_layers[g] + j*packed_layer_stride and the P columns proj[g] + 128*j.
 *   Results are bit-identical to n_layers calls of pwv_wavenet_layer_f32.
 * Every workgroup owns the same contiguous rows in every layer and walks layer after layer over them; what it needs of
 * its neighbours' rows (the x[t-d] look-back) is handed over through per-workgroup progress words in `workspace`;
 * csrc/pwv_stack_persist.hip has the protocol.  The call enqueues (unless `workspace_clean`) a kernel that zeroes the control words and one kernel
 * (grid <= one workgroup per CU; max_workgroups > 0 limits it further, e.g. to share the chip with another stream).
 *   pwv_persist_workspace_bytes   size of `workspace` (device memory, 256-byte aligned, contents don't care) for the shape in
 *                                 `args` (G, N, T, n_layers, dilations, max_workgroups, min_units_per_workgroup, tail_q, tail_dilation are read);
 *                                 0 = this shape cannot run as a persistent launch (pwv_last_error says why): use the
 *                                 per-layer launches
 *   pwv_persist_status(&p)        process-wide sticky int32 in pinned host memory: 0, or != 0 once a launch gave up
 *                                 (a poll that ran into its bound: the workgroups were not all resident, e.g. because
 *                                 another process held CUs); the outputs of that launch are then invalid and the caller
 *                                 uses the per-layer path.
 * ------------------------------------------------------------------------------------- */
typedef struct pwv_persist_args {
    size_t struct_size;                           /* = sizeof(pwv_persist_args) as the CALLER was compiled.  The library reads that many bytes and
                                                   * treats every field behind them as zero / NULL, so fields appended in later minor versions
                                                   * (the status word, the tail, the affine) cannot be read out of a shorter caller's memory;
                                                   * 0 or less than the fields up to `min_units_per_workgroup` is PWV_EINVAL.  Zero-initialise
                                                   * the struct (`pwv_persist_args a = {0}; a.struct_size = sizeof a;`) before filling it in. */
    int G;
    int n_layers;                                 /* 2..32 layers in this launch */
    const int* dilations;                         /* HOST array [n_layers] */
    float* x_ring[PWV_MAX_NETS];
    size_t ring_stride;                           /* floats between two of a net's three buffers */
    int ring_rotation;                            /* 0, 1 or 2 */
    const float* packed_layers[PWV_MAX_NETS];     /* the run's first layer */
    size_t packed_layer_stride;
    const float* proj[PWV_MAX_NETS];              /* the run's first layer's columns */
    int proj_row_stride;
    int N, T;
    int cond_hop, cond_offset, cond_frames;
    void* workspace;
    size_t workspace_bytes;
    int workspace_clean;                          /* != 0: `workspace` is all zero on entry (fresh, or last used by this entry point, which
                                                   * zeroes it again before it returns the chip): no zeroing kernel is enqueued */
    int precision;                                /* PWV_PREC_F16X3 or PWV_PREC_F32 (packed_layers packed accordingly) */
    int max_workgroups;                           /* 0 = one per CU */
    int min_units_per_workgroup;                  /* short inputs: use fewer workgroups rather than ranges below this (0 = 4) */
    /* optional: the run starts with the net's layer 0, which evaluates the causal layer itself from the scalar input [N*T]
     * (pwv_layer_args.x_first: same operations, same bits); buffer (2 + r) % 3 is then not read */
    const float* x_first;
    const float* causal_filter[PWV_MAX_NETS];
    float x_limit;                                /* range guard on x_first (pwv_layer_args.x_limit / range_flag) */
    int* range_flag;
    /* optional, with x_first: pwv_pack_first_fold_f16x3's (PWV_PREC_F16X3) or pwv_pack_first_fold_f32's (PWV_PREC_F32) output per net (all nets or none).  Layer 0's
     * filter|gate GEMM then runs on the four scalars x[t-d-1], x[t-d], x[t-1], x[t] themselves (one MFMA k-step instead of
     * eight): the same function (h[t] is linear in x[t-1], x[t]), rounded differently -- within the path's tolerance of the
     * unfolded form, not bit-identical to it */
    const float* first_fold[PWV_MAX_NETS];
    /* optional: this call's own sticky give-up word (pwv_status_words_alloc: words[0]); NULL = the process-wide word of
     * pwv_persist_status.  Two threads / streams with their own words cannot consume or clear each other's flags. */
    int* status;
    /* optional TAIL (tail_q > 0, either arithmetic; the run must be the LAST run of the stack): behind the run's layers every
     * workgroup runs the net's last layer (dilation tail_dilation, packed weights tail_layer[g], P columns proj[g] + 128*n_layers)
     * with the post-processing head behind it (tail_head[g] = pwv_pack_head_f32's output; modules.py:145-165) on its own rows and
     * writes tail_out[g] [N*T, tail_q] -- what pwv_wavenet_layer_f32 with head_packed / head_out computes, bit for bit, without
     * the two kernel boundaries.  With affine_x (the flow's input [N*T]) the IAF affine out = x*s + b (modules.py:59) is evaluated
     * too: s = net 0, b = net 1 (G = 2, tail_q = 1; by whichever of the two nets' workgroups of a row range finishes second) or
     * s, b = the two outputs of one net (G = 1, tail_q = 2); affine_out [N*T].  A flow is then ONE launch. */
    const float* tail_layer[PWV_MAX_NETS];
    const float* tail_head[PWV_MAX_NETS];
    float* tail_out[PWV_MAX_NETS];
    int tail_q;
    int tail_dilation;
    const float* affine_x;
    float* affine_out;
    /* optional PACKED ("varlen") batch: N utterances of different lengths, concatenated.  Utterance i has len_i >= 32 rows (a multiple of
     * cond_hop with a frame-rate condition) and t_mel_i = len_i / cond_hop + 1 frames; its sample t is row cu_rows[i] + t of every [R, .]
     * buffer (x_ring in tile32 blocks of the R rows, x_first, tail_out, affine_x / affine_out), its P row for sample t is
     * cu_frames[i] + (t + cond_offset) / cond_hop, and its look-back x[t-d] is zero for t < d.  T and cond_frames are ignored.
     *   cu_rows    device int32 [N+1], cu_rows[0] = 0, cu_rows[N] = R
     *   cu_frames  device int32 [N+1], cu_frames[0] = 0 (required with cond_hop > 0)
     *   unit_map   device int32 [ceil(R/32)][PWV_VARLEN_REC_INTS]: pwv_varlen_unit_map(cu_rows, cu_frames, ...) -- built once per batch,
     *              shared by every launch of the forward
     *   varlen_rows  HOST copy of R (the plan and the grid are sized on the host; nothing is read back)
     * All NULL / 0: the uniform batch of N x T rows.  Any of them set without the others (or R < 32 N) is PWV_EINVAL; read by
     * pwv_persist_workspace_bytes and pwv_persist_short_input too.  A batch with a shorter utterance has no persistent form (the engine
     * pads it).  Results are bit-identical to each utterance's own uniform launch. */
    const int* cu_rows;
    const int* cu_frames;
    const int* unit_map;
    long long varlen_rows;
    /* optional STREAMING (see "STREAMING" above pwv_stream_args): the launch continues N sessions -- its N x T rows are the T samples that
     * follow what each session has seen.  The two changes pwv_wavenet_layer_stream_f32 makes against pwv_wavenet_layer_f32, for every layer
     * of the launch and the tail's: the look-back x[t-d] of a row with t < d is the session's history of that layer's input (a run that
     * starts at x_first: the scalar history at hist->scalar_off), and the last d input rows of the chunk are stored as the next history.
     * Results are bit-identical to the L calls of pwv_wavenet_layer_stream_f32 plus the affine that the launch replaces -- outputs and
     * every written history row; a history of zeros gives the one-shot launch's bits.  With T < d the launch writes rows d-T .. d-1 of a
     * history only: pwv_stream_carry_f32 moves the rest, as for the per-layer launches.
     * The PACKED (ragged) form: with cu_rows / cu_frames / unit_map / varlen_rows set AND hist->cu_rows == cu_rows (the same device
     * table) the launch continues N sessions of different chunk lengths T_n = cu_rows[n+1] - cu_rows[n] (each >= 32): rows map to
     * (session, time, condition frame) as in a packed batch, slot_tab is indexed by the session, and T in "rows with t >= T - d store to
     * row t + d - T" is the session's own T_n.  Bit-identical, outputs and written history rows, to the uniform streaming launches of the
     * sessions grouped by length.
     *   hist          NULL: the one-shot launch.  Read: struct_size, hist_rd, hist_wr, block_stride, slot_tab, scalar_off (row_off is not:
     *                 a launch has many layers)
     *   hist_row_off  per net a HOST array [n_layers + (tail_q > 0 ? 1 : 0)]: the float offset (a multiple of 4) of the row history of the
     *                 run's layer j inside a block -- entry 0 is not read when the run starts at x_first --; the last entry is the tail's layer
     * PWV_EINVAL (before a device is needed, pwv_last_error names the field): hist together with cu_rows (any packed field) while
     * hist->cu_rows is NULL -- a caller whose pwv_stream_args describes a uniform chunk never gets a packed launch by accident --,
     * hist->cu_rows set while the launch is not packed, hist->cu_rows different from cu_rows; hist with
     * a precision other than PWV_PREC_F16X3 / PWV_PREC_F32, with x_first but no first_fold, without hist_row_off[g] for a net of the launch,
     * hist->struct_size == 0, hist->slot_tab == NULL.  pwv_persist_workspace_bytes and pwv_persist_short_input do not read these fields:
     * the plan is on rows. */
    const pwv_stream_args* hist;
    const size_t* hist_row_off[PWV_MAX_NETS];
} pwv_persist_args;

/* PWV_VARLEN_REC_INTS ints per 32-row unit of a packed batch: {n, cu_rows[n], cu_frames[n], cu_rows[n+1], cu_frames[n+1], 0, 0, 0}
 * with n the utterance that holds the unit's first row (cu_frames NULL: the frame entries are 0).  Enqueued on `stream`; no host
 * synchronisation, so lengths that are already on the device need no round trip.  units = ceil(R / 32). */
#define PWV_VARLEN_REC_INTS 8
int pwv_varlen_unit_map(const int* cu_rows, const int* cu_frames, int n_utt, int units, int* out, pwv_stream_t stream);

size_t pwv_persist_workspace_bytes(const pwv_persist_args* args);
/* 1 if pwv_wavenet_stack_persist_f32 takes its SHORT-INPUT instantiation for `args` (round 6; at most 7 units of 32 rows per workgroup and layer, i.e. up to
 * about 28000 rows for two nets on 256 CUs: progress words per unit instead of per workgroup, a unit stays on one wave through all layers -- its own rows never
 * leave the registers --, a loader wave refills the weights; same results bit for bit), 0 if the general one, -1 on arguments the launch would refuse.
 * Reads what pwv_persist_workspace_bytes reads, and x_first, first_fold, cond_hop, cond_frames, proj_row_stride. */
int pwv_persist_short_input(const pwv_persist_args* args);
int pwv_persist_status(int** status);
int pwv_wavenet_stack_persist_f32(const pwv_persist_args* args, pwv_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * A streaming TICK with its session state on the device (graph replay of a push: nothing of a tick is decided on the host).
 *
 * State (device memory, owned by the caller, one row per session slot):
 *   sess  int64 [n_slots][4] = {generation a chunk READS (0 / 1), samples emitted, noise seed (uint64 bits), 0}
 *   kept  float [n_slots][n_mels]: the last mel frame the session was given (the first frame of its next chunk)
 * Per tick the caller writes `entries` (int32 [N][2] = {slot, live}; distinct slots) and the chunk's mel [N][frames][n_mels].
 *
 * pwv_stream_tick_begin, for entry i with slot s and g = sess[s][0]:
 *   slot_tab[i]  = {2s + g, 2s + 1 - g}                       (pwv_stream_args.slot_tab: block read, block written)
 *   streams[i]   = {sess[s][2], sess[s][1]},  cu_rows[i] = i * T, cu_rows[N] = N * T      (the tables of pwv_logistic_noise_packed_f32;
 *                                                                                           both NULL: the noise is the caller's)
 *   chunk[i][0]  = kept[s],  chunk[i][1 .. frames] = mel[i]   (chunk: float [N][frames + 1][n_mels], what the prologue conditions on)
 * pwv_stream_tick_commit, the LAST launch of a tick: reads words[0] (give-up) and words[1] (range) of a pwv_status_words_alloc pair with
 * system-scope atomic loads.  Both zero: every entry with live != 0 is COMMITTED -- sess[s][0] ^= 1, sess[s][1] += T, kept[s] =
 * mel[i][frames - 1] -- and counters[0] += 1.  Otherwise nothing changes and counters[1] += 1: the words are sticky, so once a tick is
 * refused every later one is, and the committed ticks are a prefix of the enqueued ones.  An entry with live == 0 (a FILLER) is never
 * committed: it read generation g and wrote generation 1 - g, which is scratch until a flip.
 * A slot outside 0 .. n_slots-1 is read as a filler of slot 0, so that no address leaves the arrays (the caller keeps slots in range).
 * One launch each, nothing read on the host: a captured pair replays with whatever the tables hold then.
 * PWV_EINVAL before a device is needed (pwv_last_error names the field): a NULL pointer, N < 1, frames < 1, n_mels < 1, T < 1,
 * n_slots < 1, streams without cu_rows or the reverse, struct_size short of the fields the call reads.
 * ------------------------------------------------------------------------------------- */
typedef struct pwv_stream_tick_args {
    size_t struct_size;                    /* = sizeof(pwv_stream_tick_args) as the caller was compiled */
    int64_t* sess;                         /* device int64 [n_slots][4] */
    float* kept;                           /* device float [n_slots][n_mels] */
    const int32_t* entries;                /* device int32 [N][2] = {slot, live} */
    const float* mel;                      /* device float [N][frames][n_mels] */
    int32_t n_slots, N, frames, n_mels;
    int32_t T;                             /* samples of the tick per session (frames * hop) */
    /* pwv_stream_tick_begin writes: */
    int32_t* slot_tab;                     /* device int32 [N][2] */
    uint64_t* streams;                     /* device uint64 [N][2], or NULL together with cu_rows */
    int32_t* cu_rows;                      /* device int32 [N + 1] */
    float* chunk;                          /* device float [N][frames + 1][n_mels] */
    /* pwv_stream_tick_commit reads / advances: */
    const int* words;                      /* the sticky pair (mapped host memory) the tick's launches report into */
    int64_t* counters;                     /* device int64 [2] = {ticks committed, ticks refused} */
} pwv_stream_tick_args;

int pwv_stream_tick_begin(const pwv_stream_tick_args* args, pwv_stream_t stream);
int pwv_stream_tick_commit(const pwv_stream_tick_args* args, pwv_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * A RAGGED streaming tick with its session state on the device (graph replay of a push_varlen: every session its own frame count, and
 * the counts too are read on the device).  The state -- sess, kept -- is that of "A streaming TICK" above, unchanged.
 *
 * Per tick the caller writes `entries` (int32 [N][4] = {slot, live, frames, 0}; distinct slots) and `mel` (float [in_frames][n_mels]:
 * the sessions' new frames in entry order, without kept frames).  The CAPACITY is fixed: N entries, in_frames frames in all
 * (in_frames * hop rows), and min_frames >= 1, the fewest frames an entry may have (the packed persistent launches need 32 rows per
 * session).  The frame counts as the device reads them:
 *   cu_in[0] = 0;   f_i = clamp(entries[i].frames, min_frames, in_frames - cu_in[i] - (N-1-i) * min_frames)   for i < N-1;
 *   f_{N-1} = in_frames - cu_in[N-1];   cu_in[i+1] = cu_in[i] + f_i
 * so WHATEVER the table holds the N sessions have at least min_frames frames each and fill in_frames exactly: no address leaves the
 * arrays and the unit map built from cu_rows / cu_frames is well formed.  (The caller writes counts that need no clamping; an entry
 * that stands for no session is a FILLER, live = 0, with the frames that are left.)
 *
 * pwv_stream_tick_ragged_begin, for entry i with slot s and g = sess[s][0]:
 *   slot_tab[i]  = {2s + g, 2s + 1 - g}
 *   streams[i]   = {sess[s][2], sess[s][1]}                   (NULL: the noise is the caller's)
 *   cu_rows[i]   = hop * cu_in[i],  cu_frames[i] = cu_in[i] + i        (i = 0 .. N: the packed layout of pwv_persist_args and of
 *                                                                        pwv_logistic_noise_packed_f32 / pwv_varlen_unit_map)
 *   chunk[cu_frames[i]] = kept[s],  chunk[cu_frames[i] + 1 + f] = mel[cu_in[i] + f]  for f < f_i     (chunk: float [in_frames + N][n_mels])
 * pwv_stream_tick_ragged_commit, the LAST launch of a tick, makes the decision of pwv_stream_tick_commit: words[0] and words[1] are
 * read once with system-scope atomic loads; both zero: every entry with live != 0 is COMMITTED -- sess[s][0] ^= 1, sess[s][1] +=
 * hop * f_i, kept[s] = mel[cu_in[i] + f_i - 1] -- and counters[0] += 1; otherwise nothing changes and counters[1] += 1.  The committed
 * ticks are a prefix of the enqueued ones, a filler is never committed, and a slot outside 0 .. n_slots-1 is read as a filler of slot 0.
 * One launch each, nothing read on the host: a captured pair replays with whatever the tables hold then.
 *
 * STARTS (optional: `starts` non-NULL selects the starts instantiations of both kernels).  A fresh session given the frames m_0 .. m_f
 * is a running session whose kept frame is m_0, whose history is zeros, whose counter is 0 and whose new frames are m_1 .. m_f: so an
 * entry that begins a new utterance in this tick -- on a fresh slot or on a running one, whose old utterance ends there -- carries
 * frames = f in `entries` and m_1 .. m_f in `mel` like any other entry, and the caller writes besides
 *   starts  int64 [N][2] = {flag, seed (uint64 bits)}: entry i STARTS iff flag != 0 and it is no filler (live != 0, slot in range)
 *   first   float [N][n_mels]: first[i] = m_0 of a starting entry (read for starting entries only)
 *   zero_block: the index of a history block that holds zeros and that nothing ever writes (>= 2 * n_slots: no session's block)
 * For a starting entry, begin writes slot_tab[i] = {zero_block, 2s + 1 - g}, streams[i] = {starts[i].seed, 0} and
 * chunk[cu_frames[i]] = first[i]; commit -- clean words, as for every entry -- does sess[s][0] ^= 1, sess[s][1] = hop * f_i (set, not
 * added), sess[s][2] = starts[i].seed, and kept[s] as for every entry.  Everything else is as above; a refused tick changes nothing
 * for a starting entry either.  Only the FLAG of `starts` decides an address: whatever else the table holds, nothing leaves the arrays.
 * The three fields are trailing and optional: a caller compiled against the struct without them (struct_size = the offset of `starts`)
 * is served as before, the fields read as zero.
 *
 * PWV_EINVAL before a device is needed (pwv_last_error names the field): a NULL pointer (streams alone may be NULL; cu_rows and
 * cu_frames are required with or without it), N < 1, N > 1024, min_frames < 1, hop < 1, n_mels < 1, n_slots < 1,
 * in_frames < N * min_frames, in_frames * hop or (in_frames + N) * n_mels beyond 2^31 - 1, struct_size short of the fields up to
 * `counters`, starts without first, starts with zero_block < 2 * n_slots.
 * ------------------------------------------------------------------------------------- */
typedef struct pwv_stream_tick_ragged_args {
    size_t struct_size;                    /* = sizeof(pwv_stream_tick_ragged_args) as the caller was compiled */
    int64_t* sess;                         /* device int64 [n_slots][4] */
    float* kept;                           /* device float [n_slots][n_mels] */
    const int32_t* entries;                /* device int32 [N][4] = {slot, live, frames, 0} */
    const float* mel;                      /* device float [in_frames][n_mels] */
    int32_t n_slots, N, in_frames, n_mels;
    int32_t hop;                           /* samples per frame */
    int32_t min_frames;                    /* the fewest frames of an entry */
    /* pwv_stream_tick_ragged_begin writes: */
    int32_t* slot_tab;                     /* device int32 [N][2] */
    uint64_t* streams;                     /* device uint64 [N][2], or NULL */
    int32_t* cu_rows;                      /* device int32 [N + 1] */
    int32_t* cu_frames;                    /* device int32 [N + 1] */
    float* chunk;                          /* device float [in_frames + N][n_mels] */
    /* pwv_stream_tick_ragged_commit reads / advances: */
    const int* words;                      /* the sticky pair (mapped host memory) the tick's launches report into */
    int64_t* counters;                     /* device int64 [2] = {ticks committed, ticks refused} */
    /* optional, trailing (STARTS above); a struct_size that ends in front of a field reads it as zero: */
    const int64_t* starts;                 /* device int64 [N][2] = {flag, seed bits}, or NULL: no entry starts */
    const float* first;                    /* device float [N][n_mels]: the first frame of a starting entry; required with starts */
    int32_t zero_block;                    /* a history block of zeros that is never written, >= 2 * n_slots; read with starts */
} pwv_stream_tick_ragged_args;

int pwv_stream_tick_ragged_begin(const pwv_stream_tick_ragged_args* args, pwv_stream_t stream);
int pwv_stream_tick_ragged_commit(const pwv_stream_tick_ragged_args* args, pwv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PWV_HIP_H_ */
