// The loss head of training (include/pwv_hip_train_loss.h; DESIGN.md section 9, "Training"): weight_l1 * mean |out - y| +
// weight_power * mean over frames and bins of (|STFT out|^2 - |STFT y|^2)^2, the table of pwv_hip_score.h, and the gradient of that sum
// for `out`.  The STFT is the one of csrc/pwv_score.hip (tf.contrib.signal.stft at its defaults), uniform batches only (the packed
// form, csrc/pwv_train_varlen.hip, runs the same frame body: pwv_train_loss_frame.h).
// Everything is fp64 on the fp32 inputs.  Two launches, no floating-point atomics:
//   loss_frames_kernel   one workgroup per (utterance, frame): the direct real DFT of both windowed frames, one thread per bin, twiddles
//                        from an LDS table of sincospi; D_b (Ar_b, Ai_b) of every bin goes back into LDS and the same table runs backward,
//                        one thread per sample of the window, into w[j] sum_b D_b (Ar_b cos + Ai_b sin) -- the frame's gradient, win
//                        doubles in the workspace.  Further workgroups, one per (utterance, tile of samples), add |out - y|.
//   loss_gather_kernel   one workgroup per (utterance, tile): a sample adds what its frames left for it in ascending f, adds the L1 term,
//                        rounds to fp32 once and writes d_out -- also where no frame covers it.  Further workgroups, one per utterance,
//                        add the utterance's partials of the first launch in an order that depends on their index alone.
// The Nyquist bin has no sine part and its cosine is (-1)^j: it is a workgroup reduction instead of a 257th bin for 256 threads.
#include <cfloat>

#include "pwv_common.h"
#include "pwv_hip_train_loss.h"
#include "pwv_train_loss_frame.h"

namespace pwv {

struct LossParams {
    const float* out;
    const float* y;
    float* d_out;
    double* result;
    double* part;                       // [n F] power partials, then [n tiles] L1 partials
    double* grad;                       // [n F][win]: the frames' gradients, unscaled
    double scale_l1, scale_power;       // weight_l1 / (n T);  weight_power 4 / (n F B)
    int n, T, win, hop, nfft;
    int frames, tiles;                  // per utterance; frames = 0: the L1 alone
};

// blockIdx.x < n frames: frame blockIdx.x % frames of utterance blockIdx.x / frames; else a tile of the L1
__global__ __launch_bounds__(256) void loss_frames_kernel(LossParams p) {
    extern __shared__ __attribute__((aligned(16))) double loss_sm[];
    double* red = loss_sm;
    const int tid = threadIdx.x;
    const long long n_frames = (long long)p.n * p.frames;
    long long slot = blockIdx.x;
    if (slot < n_frames) {
        const int i = (int)(slot / p.frames), f = (int)(slot % p.frames);
        const long long at = (long long)i * p.T + (long long)f * p.hop;      // the frame ends at i T + f hop + win - 1 <= (i + 1) T - 1
        loss_frame(p.out + at, p.y + at, p.win, p.nfft, red, p.part + slot, p.grad + (size_t)slot * p.win);
        return;
    }
    slot -= n_frames;
    const int i = (int)(slot / p.tiles);
    const int first = (int)(slot % p.tiles) * kLossTile;
    const float* a = p.out + (long long)i * p.T;
    const float* b = p.y + (long long)i * p.T;
    double acc = 0.0;
    for (int t = first + tid; t < first + kLossTile && t < p.T; t += kLossThreads) acc += fabs((double)a[t] - (double)b[t]);
    acc = loss_block_sum(acc, red);
    if (tid == 0) p.part[n_frames + slot] = acc;
}

// blockIdx.x < n tiles: d_out of a tile of samples; else the table row of utterance blockIdx.x - n tiles
__global__ __launch_bounds__(256) void loss_gather_kernel(LossParams p) {
    __shared__ double red[kLossThreads];
    const int tid = threadIdx.x;
    const long long n_tiles = (long long)p.n * p.tiles, n_frames = (long long)p.n * p.frames;
    const long long slot = blockIdx.x;
    if (slot < n_tiles) {
        const int i = (int)(slot / p.tiles);
        const int first = (int)(slot % p.tiles) * kLossTile;
        const long long base = (long long)i * p.T;
        const double* g = p.grad + (size_t)i * p.frames * p.win;
        for (int t = first + tid; t < first + kLossTile && t < p.T; t += kLossThreads) {
            const double diff = (double)p.out[base + t] - (double)p.y[base + t];
            double v = p.scale_l1 * (diff > 0.0 ? 1.0 : (diff < 0.0 ? -1.0 : 0.0));
            if (p.frames > 0) {
                // the frames f with 0 <= t - f hop < win, in ascending order; none behind the last frame or in a gap (hop > win)
                const int lo = t >= p.win ? (t - p.win) / p.hop + 1 : 0;
                const int hi = t / p.hop < p.frames - 1 ? t / p.hop : p.frames - 1;
                double s = 0.0;
                for (int f = lo; f <= hi; ++f) s += g[(size_t)f * p.win + (t - f * p.hop)];
                v = fma(p.scale_power, s, v);
            }
            p.d_out[base + t] = (float)v;
        }
        return;
    }
    // thread t adds the partials t, t + 256, ... of the utterance in that order, the 256 sums go through the tree
    const int i = (int)(slot - n_tiles);
    double pw = 0.0, l1 = 0.0;
    const double* part = p.part + (long long)i * p.frames;
    for (int f = tid; f < p.frames; f += kLossThreads) pw += part[f];
    part = p.part + n_frames + (long long)i * p.tiles;
    for (int t = tid; t < p.tiles; t += kLossThreads) l1 += part[t];
    pw = loss_block_sum(pw, red);
    l1 = loss_block_sum(l1, red);
    if (tid == 0) {
        double* r = p.result + 4 * (size_t)i;
        r[0] = l1;
        r[1] = (double)p.T;
        r[2] = pw;
        r[3] = (double)p.frames * (double)(p.frames > 0 ? p.nfft / 2 + 1 : 0);
    }
}

static size_t loss_workspace_doubles(const LossParams& p) {
    return (size_t)p.n * p.frames + (size_t)p.n * p.tiles + (size_t)p.n * p.frames * p.win;
}

static int loss_params(const pwv_train_loss_args* a, const char* who, LossParams* p, bool need_buffers) {
    PWV_CHECK_ARG(a, "%s: args is NULL", who);
    PWV_CHECK_ARG(a->struct_size >= sizeof(pwv_train_loss_args), "%s: struct_size %zu is short of pwv_train_loss_args (%zu bytes)", who,
                  a->struct_size, sizeof(pwv_train_loss_args));
    PWV_CHECK_ARG(a->n >= 1, "%s: n %d must be >= 1", who, a->n);
    PWV_CHECK_ARG(a->T >= 1, "%s: T %d must be >= 1", who, a->T);
    PWV_CHECK_ARG((long long)a->n * a->T <= 0x7fffffffll, "%s: n T = %lld is beyond int32 (n %d, T %d)", who, (long long)a->n * a->T, a->n, a->T);
    PWV_CHECK_ARG(a->hop_length >= 1, "%s: hop_length %d must be >= 1", who, a->hop_length);
    PWV_CHECK_ARG(a->win_length >= 0 && a->win_length <= PWV_SCORE_MAX_WIN, "%s: win_length %d must be 0 (L1 only) .. %d", who, a->win_length,
                  PWV_SCORE_MAX_WIN);
    PWV_CHECK_ARG(a->weight_l1 >= 0.0 && a->weight_l1 <= DBL_MAX, "%s: weight_l1 %g must be finite and >= 0", who, a->weight_l1);
    PWV_CHECK_ARG(a->weight_power >= 0.0 && a->weight_power <= DBL_MAX, "%s: weight_power %g must be finite and >= 0", who, a->weight_power);
    const bool power = a->weight_power > 0.0 && a->win_length > 0;
    PWV_CHECK_ARG(!power || a->T >= a->win_length, "%s: T %d is shorter than win_length %d with weight_power %g > 0: there is no frame", who, a->T,
                  a->win_length, a->weight_power);
    int nfft = 0;
    if (power)
        for (nfft = 1; nfft < a->win_length; nfft <<= 1) {}
    const int frames = power ? 1 + (a->T - a->win_length) / a->hop_length : 0;
    const int tiles = (int)(((long long)a->T + kLossTile - 1) / kLossTile);
    *p = LossParams{a->out, a->y, a->d_out, a->result, (double*)a->workspace, nullptr,
                    a->weight_l1 / ((double)a->n * a->T),
                    power ? a->weight_power * 4.0 / ((double)a->n * frames * (nfft / 2 + 1)) : 0.0,
                    a->n, a->T, power ? a->win_length : 0, a->hop_length, nfft, frames, tiles};
    PWV_CHECK_ARG((long long)a->n * frames + (long long)a->n * tiles <= 0x7fffffffll,
                  "%s: n %d, T %d at hop_length %d: more workgroups than a grid holds", who, a->n, a->T, a->hop_length);
    if (!need_buffers) return PWV_OK;
    PWV_CHECK_ARG(a->out, "%s: out is a NULL pointer", who);
    PWV_CHECK_ARG(a->y, "%s: y is a NULL pointer", who);
    PWV_CHECK_ARG(a->d_out, "%s: d_out is a NULL pointer", who);
    PWV_CHECK_ARG(a->result, "%s: result is a NULL pointer", who);
    PWV_CHECK_ARG(a->workspace, "%s: workspace is a NULL pointer", who);
    const size_t need = loss_workspace_doubles(*p) * sizeof(double);
    PWV_CHECK_ARG(a->workspace_bytes >= need, "%s: workspace_bytes %zu is too small (pwv_train_loss_workspace_bytes: %zu)", who, a->workspace_bytes,
                  need);
    p->grad = p->part + (size_t)p->n * frames + (size_t)p->n * tiles;
    return PWV_OK;
}

}  // namespace pwv

using namespace pwv;

extern "C" {

size_t pwv_train_loss_workspace_bytes(const pwv_train_loss_args* a) {
    LossParams p{};
    if (loss_params(a, "pwv_train_loss_workspace_bytes", &p, false) != PWV_OK) return 0;
    return loss_workspace_doubles(p) * sizeof(double);
}

int pwv_train_loss_f32(const pwv_train_loss_args* a, pwv_stream_t stream) {
    LossParams p{};
    const int rc = loss_params(a, "pwv_train_loss_f32", &p, true);
    if (rc != PWV_OK) return rc;
    const unsigned n_frames = (unsigned)((long long)p.n * p.frames), n_tiles = (unsigned)((long long)p.n * p.tiles);
    const size_t smem = (size_t)(kLossThreads + 2 * p.nfft + 2 * (p.nfft / 2 + 1) + 2 * p.win) * sizeof(double);
    hipLaunchKernelGGL(loss_frames_kernel, dim3(n_frames + n_tiles), dim3(kLossThreads), smem, (hipStream_t)stream, p);
    PWV_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(loss_gather_kernel, dim3(n_tiles + (unsigned)p.n), dim3(kLossThreads), 0, (hipStream_t)stream, p);
    PWV_CHECK_HIP(hipGetLastError());
    return PWV_OK;
}

}  // extern "C"
