// The loss head of training (include/pwv_hip_train_loss.h, include/pwv_hip_train_varlen.h; DESIGN.md section 9, "Training" and "Packed
// training"): weight_l1 * mean |out - y| + weight_power * mean over frames and bins of (|STFT out|^2 - |STFT y|^2)^2, the table of
// pwv_hip_score.h, and the gradient of that sum for `out`.  The STFT is the one of csrc/pwv_score.hip (tf.contrib.signal.stft at its
// defaults).  Everything is fp64 on the fp32 inputs.  Two launches, no floating-point atomics, each body written once over a SPAN POLICY:
//   loss_frames_body     one workgroup per frame (pwv_train_loss_frame.h): the direct real DFT of both windowed frames, one thread per
//                        bin, twiddles from an LDS table of sincospi; D_b (Ar_b, Ai_b) of every bin goes back into LDS and the same
//                        table runs backward, one thread per sample of the window, into w[j] sum_b D_b (Ar_b cos + Ai_b sin) -- the
//                        frame's gradient, win doubles in the workspace.  Further workgroups, one per tile of samples, add |out - y|.
//   loss_gather_body     one workgroup per tile: a sample adds what its frames left for it in ascending f, adds the L1 term, rounds to
//                        fp32 once and writes d_out -- also where no frame covers it.  Further workgroups, one per utterance, add the
//                        utterance's partials of the first launch in an order that depends on their index alone.
//   DenseSpans           uniform [n, T] batches (loss_frames_kernel, loss_gather_kernel): a slot's utterance is a division, utterance i's
//                        partials and frame gradients lie at i frames and i tiles, scale_power comes from the host.
//   TableSpans           packed batches (the _varlen kernels): the lengths are read on the device, the grids are sized from the
//                        capacities n and rows, every workgroup finds its utterance by bisection and leaves if its slot is not in use
//                        (pwv_spans.h, the scheme of csrc/pwv_score.hip); scale_power is a workgroup sum over the table.
// The Nyquist bin has no sine part and its cosine is (-1)^j: it is a workgroup reduction instead of a 257th bin for 256 threads.
#include <cfloat>

#include "pwv_common.h"
#include "pwv_hip_train_loss.h"
#include "pwv_hip_train_varlen.h"
#include "pwv_train_loss_frame.h"

namespace pwv {

struct LossParams {
    const float* out;
    const float* y;
    float* d_out;
    double* result;
    double* part;                       // [frame_slots] power partials, then [tile_slots] L1 partials
    double* grad;                       // [frame_slots][win]: the frames' gradients, unscaled
    double scale_l1, power;             // weight_l1 / samples;  dense: weight_power 4 / (n F B), table: weight_power 4 (the kernel
                                        // divides by B sum_i F_i)
    int n, T, win, hop, nfft;           // win = 0: the L1 alone;  T: dense
    int frames, tiles;                  // per utterance, dense (frames = 0: the L1 alone)
    const int* cu;                      // table: the device table of bounds (pwv_spans.h) and the capacity it is clamped to
    long long rows;
    long long frame_slots, tile_slots;  // of the batch; the host's and the table kernels' (a dense kernel multiplies n by frames, tiles)
};

// where a workgroup works: utterance i = samples s .. s + L - 1 with F frames, and the slot's index within it
template <class Idx>
struct LossAt {
    int i;
    Idx idx, L, F;
    long long s;
};

// ------------------------------------------------------------------------------------------------------------------------------
// span policies: which utterance a slot belongs to, where its partials and frame gradients lie, where scale_power comes from
//   Idx          the type of an index within an utterance            utterance    the place of utterance i
//   frame, tile  the place of a frame slot / a tile slot; false: the slot is not in use (uniform over the workgroup)
//   frame_base, tile_base    the utterance's first frame slot / tile slot       frame_slots, tile_slots    all of them
//   tiles        the utterance's tiles
// ------------------------------------------------------------------------------------------------------------------------------
struct DenseSpans {
    typedef int Idx;
    typedef LossAt<int> At;
    __device__ static __forceinline__ void utterance(const LossParams& p, int i, At& w) {
        w.i = i;
        w.s = (long long)i * p.T;
        w.L = p.T;
        w.F = p.frames;
    }
    __device__ static __forceinline__ bool frame(const LossParams& p, long long slot, At& w) {
        utterance(p, (int)(slot / p.frames), w);
        w.idx = (int)(slot % p.frames);
        return true;
    }
    __device__ static __forceinline__ bool tile(const LossParams& p, long long slot, At& w) {
        utterance(p, (int)(slot / p.tiles), w);
        w.idx = (int)(slot % p.tiles);
        return true;
    }
    __device__ static __forceinline__ size_t frame_base(const LossParams& p, const At& w) { return (size_t)w.i * p.frames; }
    __device__ static __forceinline__ size_t tile_base(const LossParams& p, const At& w) { return (size_t)w.i * p.tiles; }
    __device__ static __forceinline__ long long frame_slots(const LossParams& p) { return (long long)p.n * p.frames; }
    __device__ static __forceinline__ long long tile_slots(const LossParams& p) { return (long long)p.n * p.tiles; }
    __device__ static __forceinline__ int tiles(const LossParams& p, const At&) { return p.tiles; }
    __device__ static __forceinline__ double scale_power(const LossParams& p, double*) { return p.power; }
};

struct TableSpans {
    typedef long long Idx;
    typedef LossAt<long long> At;
    __device__ static __forceinline__ Spans spans(const LossParams& p) { return Spans{p.cu, p.rows, p.n, 0, p.win, p.hop}; }
    __device__ static __forceinline__ void utterance(const LossParams& p, int i, At& w) {
        long long e;
        w.i = i;
        span_of(spans(p), i, w.s, e);
        w.L = e - w.s;
        w.F = span_frames(spans(p), w.L);
    }
    __device__ static __forceinline__ bool frame(const LossParams& p, long long slot, At& w) {
        utterance(p, span_owner(spans(p), slot, p.hop, w.idx), w);
        return w.idx >= 0 && w.idx < w.F;
    }
    __device__ static __forceinline__ bool tile(const LossParams& p, long long slot, At& w) {
        utterance(p, span_owner(spans(p), slot, kLossTile, w.idx), w);
        return w.idx >= 0 && w.idx * kLossTile < w.L;
    }
    __device__ static __forceinline__ size_t frame_base(const LossParams& p, const At& w) { return (size_t)(w.s / p.hop + w.i); }
    __device__ static __forceinline__ size_t tile_base(const LossParams&, const At& w) { return (size_t)(w.s / kLossTile + w.i); }
    __device__ static __forceinline__ long long frame_slots(const LossParams& p) { return p.frame_slots; }
    __device__ static __forceinline__ long long tile_slots(const LossParams& p) { return p.tile_slots; }
    __device__ static __forceinline__ long long tiles(const LossParams&, const At& w) { return (w.L + kLossTile - 1) / kLossTile; }
    // weight_power 4 / (B sum_i F_i): the batch's frames are integers, exact in any order
    __device__ static __forceinline__ double scale_power(const LossParams& p, double* red) {
        if (p.win < 1) return 0.0;
        double tot = 0.0;
        for (int k = threadIdx.x; k < p.n; k += kLossThreads) {
            At w;
            utterance(p, k, w);
            tot += (double)w.F;
        }
        tot = block_sum(tot, red);
        return tot > 0.0 ? p.power / (tot * (p.nfft / 2 + 1)) : 0.0;
    }
};

// blockIdx.x < frame_slots: a frame slot; else a tile slot
template <class S>
__device__ __forceinline__ void loss_frames_body(const LossParams& p) {
    extern __shared__ __attribute__((aligned(16))) double loss_sm[];
    typedef typename S::Idx Idx;
    double* red = loss_sm;
    const int tid = threadIdx.x;
    const long long n_frames = S::frame_slots(p);
    long long slot = blockIdx.x;
    typename S::At w;
    if (slot < n_frames) {
        if (!S::frame(p, slot, w)) return;                                // (before any barrier)
        const long long at = w.s + (long long)w.idx * p.hop;              // the frame ends at s + idx hop + win - 1 <= s + L - 1 < rows
        loss_frame(p.out + at, p.y + at, p.win, p.nfft, red, p.part + slot, p.grad + (size_t)slot * p.win);
        return;
    }
    slot -= n_frames;
    if (!S::tile(p, slot, w)) return;
    const Idx first = w.idx * kLossTile;
    const float* a = p.out + w.s;
    const float* b = p.y + w.s;
    double acc = 0.0;
    for (Idx t = first + tid; t < first + kLossTile && t < w.L; t += kLossThreads) acc += fabs((double)a[t] - (double)b[t]);
    acc = block_sum(acc, red);
    if (tid == 0) p.part[n_frames + slot] = acc;
}

// blockIdx.x < tile_slots: d_out of a tile of samples; else the table row of utterance blockIdx.x - tile_slots
template <class S>
__device__ __forceinline__ void loss_gather_body(const LossParams& p) {
    __shared__ double red[kLossThreads];
    typedef typename S::Idx Idx;
    const int tid = threadIdx.x;
    const long long n_tiles = S::tile_slots(p), slot = blockIdx.x;
    typename S::At w;
    if (slot < n_tiles) {
        if (!S::tile(p, slot, w)) return;                                 // (before any barrier)
        const double scale_power = S::scale_power(p, red);
        const Idx first = w.idx * kLossTile;
        const double* g = p.grad + S::frame_base(p, w) * p.win;
        for (Idx t = first + tid; t < first + kLossTile && t < w.L; t += kLossThreads) {
            const double diff = (double)p.out[w.s + t] - (double)p.y[w.s + t];
            double v = p.scale_l1 * (diff > 0.0 ? 1.0 : (diff < 0.0 ? -1.0 : 0.0));
            if (w.F > 0) {
                // the frames f with 0 <= t - f hop < win, in ascending order; none behind the last frame or in a gap (hop > win)
                const Idx lo = t >= p.win ? (t - p.win) / p.hop + 1 : 0;
                const Idx hi = t / p.hop < w.F - 1 ? t / p.hop : w.F - 1;
                double sum = 0.0;
                for (Idx f = lo; f <= hi; ++f) sum += g[(size_t)f * p.win + (t - f * p.hop)];
                v = fma(scale_power, sum, v);
            }
            p.d_out[w.s + t] = (float)v;
        }
        return;
    }
    // thread t adds the partials t, t + 256, ... of the utterance in that order, the 256 sums go through the tree
    S::utterance(p, (int)(slot - n_tiles), w);
    const Idx tiles = S::tiles(p, w);
    double pw = 0.0, l1 = 0.0;
    const double* part = p.part + S::frame_base(p, w);
    for (Idx f = tid; f < w.F; f += kLossThreads) pw += part[f];
    part = p.part + S::frame_slots(p) + S::tile_base(p, w);
    for (Idx t = tid; t < tiles; t += kLossThreads) l1 += part[t];
    pw = block_sum(pw, red);
    l1 = block_sum(l1, red);
    if (tid == 0) {
        double* r = p.result + 4 * (size_t)w.i;
        r[0] = l1;
        r[1] = (double)w.L;
        r[2] = pw;
        r[3] = (double)w.F * (double)(w.F > 0 ? p.nfft / 2 + 1 : 0);
    }
}

__global__ __launch_bounds__(256) void loss_frames_kernel(LossParams p) { loss_frames_body<DenseSpans>(p); }
__global__ __launch_bounds__(256) void loss_gather_kernel(LossParams p) { loss_gather_body<DenseSpans>(p); }
// (the host refuses a packed call without its table; told so, the compiler drops span_bound's uniform branch and the scalar registers
// it would cost these two over their earlier selves)
__global__ __launch_bounds__(256) void loss_frames_varlen_kernel(LossParams p) {
    __builtin_assume(p.cu != nullptr);
    loss_frames_body<TableSpans>(p);
}
__global__ __launch_bounds__(256) void loss_gather_varlen_kernel(LossParams p) {
    __builtin_assume(p.cu != nullptr);
    loss_gather_body<TableSpans>(p);
}

// ------------------------------------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------------------------------------
static size_t loss_workspace_doubles(const LossParams& p) {
    return (size_t)p.frame_slots + (size_t)p.tile_slots + (size_t)p.frame_slots * p.win;
}

// What pwv_train_loss_args and pwv_train_loss_varlen_args share, under the same field names: the settings, the buffers and the
// workspace.  The caller has checked the struct and its batch.  `form(power)` is the entry point's own part once the settings hold:
// what it still refuses about the batch, then the batch, the scales and the slot counts.  `sizer`: the name of its size function.
template <class Args, class Form>
static int loss_params(const Args* a, const char* who, const char* sizer, LossParams* p, bool need_buffers, Form form) {
    PWV_CHECK_ARG(a->hop_length >= 1, "%s: hop_length %d must be >= 1", who, a->hop_length);
    PWV_CHECK_ARG(a->win_length >= 0 && a->win_length <= PWV_SCORE_MAX_WIN, "%s: win_length %d must be 0 (L1 only) .. %d", who, a->win_length,
                  PWV_SCORE_MAX_WIN);
    PWV_CHECK_ARG(a->weight_l1 >= 0.0 && a->weight_l1 <= DBL_MAX, "%s: weight_l1 %g must be finite and >= 0", who, a->weight_l1);
    PWV_CHECK_ARG(a->weight_power >= 0.0 && a->weight_power <= DBL_MAX, "%s: weight_power %g must be finite and >= 0", who, a->weight_power);
    const bool power = a->weight_power > 0.0 && a->win_length > 0;
    *p = LossParams{};
    p->out = a->out; p->y = a->y; p->d_out = a->d_out; p->result = a->result; p->part = (double*)a->workspace;
    p->win = power ? a->win_length : 0;
    p->hop = a->hop_length;
    if (power)
        for (p->nfft = 1; p->nfft < a->win_length; p->nfft <<= 1) {}
    if (int e = form(power)) return e;
    if (!need_buffers) return PWV_OK;
    PWV_CHECK_ARG(a->out, "%s: out is a NULL pointer", who);
    PWV_CHECK_ARG(a->y, "%s: y is a NULL pointer", who);
    PWV_CHECK_ARG(a->d_out, "%s: d_out is a NULL pointer", who);
    PWV_CHECK_ARG(a->result, "%s: result is a NULL pointer", who);
    PWV_CHECK_ARG(a->workspace, "%s: workspace is a NULL pointer", who);
    const size_t need = loss_workspace_doubles(*p) * sizeof(double);
    PWV_CHECK_ARG(a->workspace_bytes >= need, "%s: workspace_bytes %zu is too small (%s: %zu)", who, a->workspace_bytes, sizer, need);
    p->grad = p->part + p->frame_slots + p->tile_slots;
    return PWV_OK;
}

static int loss_dense_params(const pwv_train_loss_args* a, const char* who, LossParams* p, bool need_buffers) {
    PWV_CHECK_ARG(a, "%s: args is NULL", who);
    PWV_CHECK_ARG(a->struct_size >= sizeof(pwv_train_loss_args), "%s: struct_size %zu is short of pwv_train_loss_args (%zu bytes)", who,
                  a->struct_size, sizeof(pwv_train_loss_args));
    PWV_CHECK_ARG(a->n >= 1, "%s: n %d must be >= 1", who, a->n);
    PWV_CHECK_ARG(a->T >= 1, "%s: T %d must be >= 1", who, a->T);
    PWV_CHECK_ARG((long long)a->n * a->T <= 0x7fffffffll, "%s: n T = %lld is beyond int32 (n %d, T %d)", who, (long long)a->n * a->T, a->n, a->T);
    return loss_params(a, who, "pwv_train_loss_workspace_bytes", p, need_buffers, [&](bool power) {
        PWV_CHECK_ARG(!power || a->T >= a->win_length, "%s: T %d is shorter than win_length %d with weight_power %g > 0: there is no frame", who, a->T,
                      a->win_length, a->weight_power);
        p->frames = power ? 1 + (a->T - a->win_length) / a->hop_length : 0;
        p->tiles = (int)(((long long)a->T + kLossTile - 1) / kLossTile);
        p->n = a->n;
        p->T = a->T;
        p->scale_l1 = a->weight_l1 / ((double)a->n * a->T);
        p->power = power ? a->weight_power * 4.0 / ((double)a->n * p->frames * (p->nfft / 2 + 1)) : 0.0;
        p->frame_slots = (long long)a->n * p->frames;
        p->tile_slots = (long long)a->n * p->tiles;
        PWV_CHECK_ARG(p->frame_slots + p->tile_slots <= 0x7fffffffll, "%s: n %d, T %d at hop_length %d: more workgroups than a grid holds", who, a->n,
                      a->T, a->hop_length);
        return (int)PWV_OK;
    });
}

static int loss_table_params(const pwv_train_loss_varlen_args* a, const char* who, LossParams* p, bool need_buffers) {
    PWV_CHECK_ARG(a, "%s: args is NULL", who);
    PWV_CHECK_ARG(a->struct_size == sizeof(pwv_train_loss_varlen_args), "%s: struct_size %zu is not sizeof(pwv_train_loss_varlen_args) = %zu", who,
                  a->struct_size, sizeof(pwv_train_loss_varlen_args));
    PWV_CHECK_ARG(a->n >= 1, "%s: n %d must be >= 1", who, a->n);
    PWV_CHECK_ARG(a->rows >= a->n, "%s: rows %d is below n %d", who, a->rows, a->n);
    PWV_CHECK_ARG((long long)a->rows < (1ll << 31) - 64, "%s: rows %d is beyond int32 (2^31 - 64)", who, a->rows);
    return loss_params(a, who, "pwv_train_loss_varlen_workspace_bytes", p, need_buffers, [&](bool power) {
        p->cu = a->cu_rows;
        p->rows = a->rows;
        p->n = a->n;
        p->scale_l1 = a->weight_l1 / (double)a->rows;
        p->power = power ? a->weight_power * 4.0 : 0.0;
        p->frame_slots = power ? (long long)a->rows / a->hop_length + a->n : 0;
        p->tile_slots = (long long)a->rows / kLossTile + a->n;
        PWV_CHECK_ARG(p->frame_slots + p->tile_slots + a->n <= 0x7fffffffll, "%s: rows %d / hop_length %d with n %d: more workgroups than a grid holds",
                      who, a->rows, a->hop_length, a->n);
        // (its place among the buffers is behind out and y: with one of those NULL, that refusal comes first)
        PWV_CHECK_ARG(!need_buffers || !a->out || !a->y || a->cu_rows, "%s: cu_rows is a NULL pointer", who);
        return (int)PWV_OK;
    });
}

// both launches of either form; the grids: frame slots + tile slots, tile slots + n
template <class Kernel>
static int loss_launch(const LossParams& p, Kernel frames_kernel, Kernel gather_kernel, hipStream_t st) {
    const size_t smem = (size_t)(kLossThreads + 2 * p.nfft + 2 * (p.nfft / 2 + 1) + 2 * p.win) * sizeof(double);
    hipLaunchKernelGGL(frames_kernel, dim3((unsigned)(p.frame_slots + p.tile_slots)), dim3(kLossThreads), smem, st, p);
    PWV_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(gather_kernel, dim3((unsigned)(p.tile_slots + p.n)), dim3(kLossThreads), 0, st, p);
    PWV_CHECK_HIP(hipGetLastError());
    return PWV_OK;
}

}  // namespace pwv

using namespace pwv;

extern "C" {

size_t pwv_train_loss_workspace_bytes(const pwv_train_loss_args* a) {
    LossParams p{};
    if (loss_dense_params(a, "pwv_train_loss_workspace_bytes", &p, false) != PWV_OK) return 0;
    return loss_workspace_doubles(p) * sizeof(double);
}

int pwv_train_loss_f32(const pwv_train_loss_args* a, pwv_stream_t stream) {
    LossParams p{};
    if (int e = loss_dense_params(a, "pwv_train_loss_f32", &p, true)) return e;
    return loss_launch(p, loss_frames_kernel, loss_gather_kernel, (hipStream_t)stream);
}

size_t pwv_train_loss_varlen_workspace_bytes(const pwv_train_loss_varlen_args* a) {
    LossParams p{};
    if (loss_table_params(a, "pwv_train_loss_varlen_workspace_bytes", &p, false) != PWV_OK) return 0;
    return loss_workspace_doubles(p) * sizeof(double);
}

int pwv_train_loss_varlen_f32(const pwv_train_loss_varlen_args* a, pwv_stream_t stream) {
    LossParams p{};
    if (int e = loss_table_params(a, "pwv_train_loss_varlen_f32", &p, true)) return e;
    return loss_launch(p, loss_frames_varlen_kernel, loss_gather_varlen_kernel, (hipStream_t)stream);
}

}  // extern "C"
