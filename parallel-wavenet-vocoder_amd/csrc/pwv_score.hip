// Scoring generated audio on the device (include/pwv_hip_score.h; DESIGN.md section 9, "Scoring on the device"): per utterance the sum of
// |out - y| and the sum over frames and bins of (|STFT out|^2 - |STFT y|^2)^2, the two quantities the reference's models.py:90-99 logs
// as loss/likelihood and loss/power, as forward-only metrics.  The STFT is tf.contrib.signal.stft at its defaults (periodic Hann window of
// win_length, frames zero-padded BEHIND to the next power of two, no centring, no end padding) -- not librosa's of the mel front-end, so
// nothing of pwv_mel_frame_body.inc is used here.
// Everything is fp64 on the fp32 inputs: a direct real DFT over the win_length samples of a frame, twiddles from an LDS table of
// sincospi.  A few GFLOP for a batch of seconds of audio; one workgroup per frame.
// Two kernels, no atomics: score_partials_kernel writes one partial per (utterance, frame) and per (utterance, tile of samples),
// score_reduce_kernel adds an utterance's partials in an order that depends on their index within the utterance alone -- a row of the
// result does not depend on what else is in the batch.  The lengths of a packed batch are read on the device (cu_rows): the grid is sized
// from the capacities, every workgroup finds its utterance by bisection and leaves if its slot is not in use (pwv_spans.h, which the
// loss head of training, csrc/pwv_train_loss.hip, shares; the DFT body here is this file's own: its Nyquist bin goes through the twiddle
// table, the loss head's through a reduction).
#include "pwv_common.h"
#include "pwv_hip_score.h"
#include "pwv_spans.h"

namespace pwv {

constexpr int kScoreThreads = kSumThreads;      // workgroup size of both kernels, and the stride of the reduction's first pass
constexpr int kScoreTile = PWV_SCORE_TILE;

struct ScoreParams {
    const float* out;
    const float* y;
    const int* cu;                      // NULL: uniform
    double* result;
    double* part;                       // [frame_slots] power partials, then [tile_slots] L1 partials
    long long rows, frame_slots, tile_slots;
    int n, T, win, hop, nfft;
};

// (the parameters keep the layout they had before pwv_spans.h: both kernels compile to the instruction streams of before)
__device__ __forceinline__ Spans score_spans(const ScoreParams& p) { return Spans{p.cu, p.rows, p.n, p.T, p.win, p.hop}; }

// blockIdx.x < frame_slots: a frame slot; else a tile slot
__global__ __launch_bounds__(256) void score_partials_kernel(ScoreParams p) {
    extern __shared__ __attribute__((aligned(16))) double score_sm[];      // [256] reduction, [win] out frame, [win] y frame, [nfft] cos, [nfft] sin
    double* red = score_sm;
    const int tid = threadIdx.x;
    const Spans sp = score_spans(p);
    long long slot = blockIdx.x, idx, s, e;
    if (slot < p.frame_slots) {
        const int i = span_owner(sp, slot, p.hop, idx);
        span_of(sp, i, s, e);
        if (idx < 0 || idx >= span_frames(sp, e - s)) return;                 // (uniform over the workgroup: before any barrier)
        const int win = p.win, nfft = p.nfft;
        double* fa = red + kScoreThreads;
        double* fb = fa + win;
        double* ct = fb + win;
        double* st = ct + nfft;
        const float* a = p.out + s + idx * p.hop;                         // the frame ends at s + idx hop + win - 1 <= e - 1 < rows
        const float* b = p.y + s + idx * p.hop;
        for (int j = tid; j < win; j += kScoreThreads) {
            const double w = 0.5 - 0.5 * cospi(2.0 * j / win);
            fa[j] = (double)a[j] * w;
            fb[j] = (double)b[j] * w;
        }
        for (int j = tid; j < nfft; j += kScoreThreads) {
            double sn, cs;
            sincospi(2.0 * j / nfft, &sn, &cs);
            ct[j] = cs;
            st[j] = sn;
        }
        __syncthreads();
        double acc = 0.0;
        for (int bin = tid; bin <= nfft / 2; bin += kScoreThreads) {
            double ar = 0.0, ai = 0.0, br = 0.0, bi = 0.0;
            int k = 0;                                                    // (bin * j) mod nfft
            for (int j = 0; j < win; ++j) {
                const double c = ct[k], sn = st[k];
                ar = fma(fa[j], c, ar);
                ai = fma(fa[j], sn, ai);
                br = fma(fb[j], c, br);
                bi = fma(fb[j], sn, bi);
                k = (k + bin) & (nfft - 1);
            }
            const double d = (ar * ar + ai * ai) - (br * br + bi * bi);
            acc = fma(d, d, acc);
        }
        acc = block_sum(acc, red);
        if (tid == 0) p.part[slot] = acc;
        return;
    }
    slot -= p.frame_slots;
    const int i = span_owner(sp, slot, kScoreTile, idx);
    span_of(sp, i, s, e);
    const long long L = e - s, first = idx * kScoreTile;
    if (idx < 0 || first >= L) return;
    double acc = 0.0;
    for (long long t = first + tid; t < first + kScoreTile && t < L; t += kScoreThreads) acc += fabs((double)p.out[s + t] - (double)p.y[s + t]);
    acc = block_sum(acc, red);
    if (tid == 0) p.part[p.frame_slots + slot] = acc;
}

// one workgroup per utterance: thread t adds the partials t, t + 256, ... of the utterance in that order, the 256 sums go through the tree
__global__ __launch_bounds__(256) void score_reduce_kernel(ScoreParams p) {
    __shared__ double red[kScoreThreads];
    const int i = blockIdx.x, tid = threadIdx.x;
    const Spans sp = score_spans(p);
    long long s, e;
    span_of(sp, i, s, e);
    const long long L = e - s, frames = span_frames(sp, L), tiles = (L + kScoreTile - 1) / kScoreTile;
    double pw = 0.0, l1 = 0.0;
    if (frames > 0) {
        const double* part = p.part + (s / p.hop + i);
        for (long long f = tid; f < frames; f += kScoreThreads) pw += part[f];
    }
    const double* part = p.part + p.frame_slots + (s / kScoreTile + i);
    for (long long t = tid; t < tiles; t += kScoreThreads) l1 += part[t];
    pw = block_sum(pw, red);
    l1 = block_sum(l1, red);
    if (tid == 0) {
        double* r = p.result + 4 * (size_t)i;
        r[0] = l1;
        r[1] = (double)L;
        r[2] = pw;
        r[3] = (double)frames * (double)(p.nfft / 2 + 1);
    }
}

static int score_params(const pwv_score_args* a, const char* who, ScoreParams* p, bool need_buffers) {
    PWV_CHECK_ARG(a, "%s: args is NULL", who);
    PWV_CHECK_ARG(a->struct_size >= sizeof(pwv_score_args), "%s: struct_size %zu is short of pwv_score_args (%zu bytes)", who, a->struct_size,
                  sizeof(pwv_score_args));
    PWV_CHECK_ARG(a->n >= 1, "%s: n %d must be >= 1", who, a->n);
    PWV_CHECK_ARG(a->hop_length >= 1, "%s: hop_length %d must be >= 1", who, a->hop_length);
    PWV_CHECK_ARG(a->win_length >= 0 && a->win_length <= PWV_SCORE_MAX_WIN, "%s: win_length %d must be 0 (L1 only) .. %d", who, a->win_length,
                  PWV_SCORE_MAX_WIN);
    PWV_CHECK_ARG(a->rows >= 0 && a->rows <= 0x7fffffffll, "%s: rows %lld out of range (0 .. 2^31 - 1)", who, (long long)a->rows);
    PWV_CHECK_ARG(a->cu_rows || (a->T >= 0 && (long long)a->n * a->T <= a->rows), "%s: T %d: n T = %lld leaves rows %lld", who, a->T,
                  (long long)a->n * a->T, (long long)a->rows);
    int nfft = 0;
    if (a->win_length > 0)
        for (nfft = 1; nfft < a->win_length; nfft <<= 1) {}
    *p = ScoreParams{a->out, a->y, a->cu_rows, a->result, (double*)a->workspace, a->rows,
                     a->win_length > 0 ? a->rows / a->hop_length + a->n : 0, a->rows / kScoreTile + a->n,
                     a->n, a->cu_rows ? 0 : a->T, a->win_length, a->hop_length, nfft};
    PWV_CHECK_ARG(p->frame_slots + p->tile_slots <= 0x7fffffffll, "%s: rows %lld / hop_length %d with n %d: more slots than a grid holds", who,
                  (long long)a->rows, a->hop_length, a->n);
    if (!need_buffers) return PWV_OK;
    PWV_CHECK_ARG(a->out, "%s: out is a NULL pointer", who);
    PWV_CHECK_ARG(a->y, "%s: y is a NULL pointer", who);
    PWV_CHECK_ARG(a->result, "%s: result is a NULL pointer", who);
    PWV_CHECK_ARG(a->workspace, "%s: workspace is a NULL pointer", who);
    const size_t need = (size_t)(p->frame_slots + p->tile_slots) * sizeof(double);
    PWV_CHECK_ARG(a->workspace_bytes >= need, "%s: workspace_bytes %zu is too small (pwv_score_workspace_bytes: %zu)", who, a->workspace_bytes, need);
    return PWV_OK;
}

}  // namespace pwv

using namespace pwv;

extern "C" {

size_t pwv_score_workspace_bytes(const pwv_score_args* a) {
    ScoreParams p{};
    if (score_params(a, "pwv_score_workspace_bytes", &p, false) != PWV_OK) return 0;
    return (size_t)(p.frame_slots + p.tile_slots) * sizeof(double);
}

int pwv_score_f32(const pwv_score_args* a, pwv_stream_t stream) {
    ScoreParams p{};
    const int rc = score_params(a, "pwv_score_f32", &p, true);
    if (rc != PWV_OK) return rc;
    const size_t smem = (size_t)(kScoreThreads + 2 * p.win + 2 * p.nfft) * sizeof(double);
    hipLaunchKernelGGL(score_partials_kernel, dim3((unsigned)(p.frame_slots + p.tile_slots)), dim3(kScoreThreads), smem, (hipStream_t)stream, p);
    PWV_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(score_reduce_kernel, dim3((unsigned)p.n), dim3(kScoreThreads), 0, (hipStream_t)stream, p);
    PWV_CHECK_HIP(hipGetLastError());
    return PWV_OK;
}

}  // extern "C"
