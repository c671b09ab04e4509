// The body of one frame of training's loss head (csrc/pwv_train_loss.hip, both its forms): the direct real DFT of both windowed frames
// in fp64 and the same twiddle table run backward into the frame's gradient.  The workgroup sum is block_sum of pwv_spans.h.
#ifndef PWV_TRAIN_LOSS_FRAME_H
#define PWV_TRAIN_LOSS_FRAME_H

#include "pwv_common.h"
#include "pwv_hip_score.h"
#include "pwv_spans.h"

namespace pwv {

constexpr int kLossThreads = kSumThreads;      // workgroup size of both kernels, and the stride of the reduction's first pass
constexpr int kLossTile = PWV_SCORE_TILE;

typedef double f64x2 __attribute__((ext_vector_type(2)));

// One frame, by the whole workgroup: a, b = the win samples of out and y; the frame's power partial goes to *part, its win gradient
// values (unscaled) to g.  red: LDS, [256] reduction, [nfft] (cos, sin), [nfft / 2 + 1] D (Ar, Ai), [win] (out, y) under the window.
__device__ __forceinline__ void loss_frame(const float* a, const float* b, int win, int nfft, double* red, double* part, double* g) {
    const int tid = threadIdx.x, half = nfft / 2;
    f64x2* tw = (f64x2*)(red + kLossThreads);
    f64x2* cw = tw + nfft;
    f64x2* fr = cw + (half + 1);
    for (int j = tid; j < win; j += kLossThreads) {
        const double w = 0.5 - 0.5 * cospi(2.0 * j / win);
        fr[j] = f64x2{(double)a[j] * w, (double)b[j] * w};
    }
    for (int j = tid; j < nfft; j += kLossThreads) {
        double sn, cs;
        sincospi(2.0 * j / nfft, &sn, &cs);
        tw[j] = f64x2{cs, sn};
    }
    __syncthreads();
    double acc = 0.0;
    // bins 0 .. nfft / 2 - 1 (nfft = 1: its only bin)
    for (int bin = tid; bin < (half > 0 ? half : 1); bin += kLossThreads) {
        double ar = 0.0, ai = 0.0, br = 0.0, bi = 0.0;
        int k = 0;                                                    // (bin * j) mod nfft
        for (int j = 0; j < win; ++j) {
            const f64x2 t = tw[k], v = fr[j];
            ar = fma(v.x, t.x, ar);
            ai = fma(v.x, t.y, ai);
            br = fma(v.y, t.x, br);
            bi = fma(v.y, t.y, bi);
            k = (k + bin) & (nfft - 1);
        }
        const double d = (ar * ar + ai * ai) - (br * br + bi * bi);
        cw[bin] = f64x2{d * ar, d * ai};
        acc = fma(d, d, acc);
    }
    if (half > 0) {                                                   // the Nyquist bin: cos(pi j) = (-1)^j, sin(pi j) = 0
        double na = 0.0, nb = 0.0;
        for (int j = tid; j < win; j += kLossThreads) {
            const f64x2 v = fr[j];
            na += (j & 1) ? -v.x : v.x;
            nb += (j & 1) ? -v.y : v.y;
        }
        na = block_sum(na, red);
        nb = block_sum(nb, red);
        if (tid == 0) {
            const double d = na * na - nb * nb;
            cw[half] = f64x2{d * na, 0.0};
            acc = fma(d, d, acc);
        }
    }
    acc = block_sum(acc, red);                                        // (its barriers also publish cw)
    if (tid == 0) *part = acc;
    for (int j = tid; j < win; j += kLossThreads) {
        double sr = 0.0, si = 0.0;
        int k = 0;                                                    // (bin * j) mod nfft
        for (int bin = 0; bin <= half; ++bin) {
            const f64x2 t = tw[k], c = cw[bin];
            sr = fma(c.x, t.x, sr);
            si = fma(c.y, t.y, si);
            k = (k + j) & (nfft - 1);
        }
        g[j] = (0.5 - 0.5 * cospi(2.0 * j / win)) * (sr + si);
    }
}

}  // namespace pwv

#endif  // PWV_TRAIN_LOSS_FRAME_H
