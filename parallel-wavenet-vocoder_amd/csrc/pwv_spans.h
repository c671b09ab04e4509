// Where the utterances of a batch lie, for the kernels that work per utterance on flat [rows] audio: scoring (csrc/pwv_score.hip) and
// the loss head of training (csrc/pwv_train_loss.hip).  A batch is n utterances, uniform (utterance i = samples i T .. (i + 1) T - 1) or
// packed (a device table cu of n + 1 bounds, read by the kernels: a wrong table never leads a load out of [0, rows)).  The grids are
// sized from the capacities n and rows: utterance i's slots of `unit` samples begin at bound(i) / unit + i, every workgroup finds the
// owner of its slot by bisection and leaves if the slot is not in use.  Beside them the workgroup sum both users reduce with.
#ifndef PWV_SPANS_H
#define PWV_SPANS_H

#include "pwv_common.h"

namespace pwv {

constexpr int kSumThreads = 256;        // the workgroup size block_sum is written for

struct Spans {
    const int* cu;                      // NULL: uniform
    long long rows;
    int n, T, win, hop;                 // (T: uniform batches; win < 1: no frames)
};

// bound i of the batch (0 .. n), inside 0 .. rows whatever the table holds
__device__ __forceinline__ long long span_bound(const Spans& sp, int i) {
    const long long v = sp.cu ? (long long)sp.cu[i] : (long long)i * sp.T;
    return v < 0 ? 0 : (v > sp.rows ? sp.rows : v);
}

// utterance i = samples [s, e)
__device__ __forceinline__ void span_of(const Spans& sp, int i, long long& s, long long& e) {
    s = span_bound(sp, i);
    e = span_bound(sp, i + 1);
    if (e < s) e = s;
}

__device__ __forceinline__ long long span_frames(const Spans& sp, long long L) {
    return sp.win < 1 || L < sp.win ? 0 : 1 + (L - sp.win) / sp.hop;
}

// The utterance that owns `slot` where utterance i's slots begin at bound(i) / unit + i (strictly increasing in i), and the slot's index
// within it (negative: before the first utterance's).  Every thread of the workgroup gets the same answer.
__device__ __forceinline__ int span_owner(const Spans& sp, long long slot, int unit, long long& idx) {
    int lo = 0, hi = sp.n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (span_bound(sp, mid) / unit + mid <= slot) lo = mid; else hi = mid - 1;
    }
    idx = slot - (span_bound(sp, lo) / unit + lo);
    return lo;
}

// the sum of the workgroup's 256 values, added as a fixed tree; every thread gets it
__device__ __forceinline__ double block_sum(double v, double* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = kSumThreads / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

}  // namespace pwv

#endif  // PWV_SPANS_H
