// The unit bodies of training that depend on where an utterance begins and ends ("Training" and "Packed
// training"): front forward, layer forward, layer backward, front backward, written once over a GEOMETRY POLICY and, the two layer
// bodies, a CONDITIONING POLICY (ProjCond below: a row of the frame-rate projection P; SampleCond, csrc/pwv_train_cond.hip: a condition
// row per sample) and a SKIP POLICY (NoSkip below: the head reads the last layer's o; SumSkip: every layer adds o skip + skip_bias to the
// net's skip sum S and takes dS skip^T into its d o, csrc/pwv_train_skip.hip).
//   UniformGeo   utterance n owns rows n T .. (n + 1) T - 1 and P rows n frames ..: t, n and the P row are arithmetic on the row
//                (csrc/pwv_train.hip instantiates the bodies with it under the kernel names of include/pwv_hip_train.h).
//   PackedGeo    utterance i owns rows cu_rows[i] .. cu_rows[i + 1] - 1 and P rows cu_frames[i] ..: 33 threads LOCATE the rows of a
//                unit (and the first row behind it) once, by a search of cu_rows, and leave (t, T_i, P row, first packed row of the
//                frame) in LDS; every bulk load reads them from there (csrc/pwv_train_varlen.hip).
// Every kernel works on UNITS of 32 rows (one tile32 block) with 256 threads = 4 waves.  The operands of a unit's GEMMs are staged in LDS
// as plain row-major [32][odd stride] arrays; a wave computes one 32 x 32 tile per GEMM call:
//   activations x weights    A[i = row][k] from LDS, B[k][j] from the TF-layout weight in global memory (strides pick W or W^T)
//   weight gradients         A[i][k = row] and B[k = row][j] both from LDS: the 32 rows of the unit are the K dimension, the tile stays in
//                            the wave's accumulators over all units of the workgroup and leaves once, as the workgroup's partial.
// A second launch (train_reduce_kernel, csrc/pwv_train.hip) adds the partials in a fixed order and scatters them to the TF layouts.
// Behind the bodies the host text of the four entry-point kinds (train_front_fwd, train_layer_fwd, train_layer_bwd, train_front_bwd),
// once for every ABI struct; what a uniform struct is checked for first is train_check_batch of csrc/pwv_train.hip.
#ifndef PWV_TRAIN_UNITS_H
#define PWV_TRAIN_UNITS_H

#include "pwv_common.h"
#include "pwv_hip_train.h"

namespace pwv {

constexpr int kTrThreads = 256;
constexpr int kLdW = 129;               // LDS row stride of a 128-column array (odd: a column walk over rows is conflict-free)
constexpr int kLdH = 65;                // ... of a 64-column array
constexpr int kLayerPart = 128 * 128 + 64 * 64 + 64;                       // dWfg | d dense | d dense_bias
constexpr int kFrontPart = 128;                                            // d cf[0] | d cf[1]

struct Geom {
    int rows, T, d, dnext, hop, off, frames, pstride, dpstride, kmax;       // (T, frames: uniform batches)
};

// packed batches (PackedGeo): the device tables, int32 [n + 1] each, and the P rows in all; behind every other field of a kernel's
// parameters, where a uniform launch leaves them unread
struct PackedTables {
    const int *cu_rows, *cu_frames;
    int n, prows;
};

__device__ __forceinline__ f32x16 zero16() {
    f32x16 z;
#pragma unroll
    for (int r = 0; r < 16; ++r) z[r] = 0.f;
    return z;
}

// acc[i][j] += sum_{k < K} A[i][k] * B[k][j]:  A in LDS (row stride lda), B[k][j] = B[k * sk + j] in global memory (a weight as it lies:
// the 32 lanes of a half read 128 contiguous bytes)
template <int K>
__device__ __forceinline__ void gemm_xw(f32x16& acc, const float* A, int lda, const float* __restrict__ B, int sk) {
    const int lane = threadIdx.x & 63, i = lane & 31, h = lane >> 5;
    const float* a = A + i * lda + h;
    const float* b = B + (size_t)h * sk + i;
#pragma unroll 8
    for (int k = 0; k < K; k += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[k], b[(size_t)k * sk], acc, 0, 0, 0);
}

// the same with the weight TRANSPOSED: B[k][j] = B[j * sj + k].  A lane walks along k in its own row of the weight, so it loads 16 bytes
// at a time: of every 8 values of k the lane half h takes 4 h .. 4 h + 3 (which k meets which MFMA step only orders the sum)
template <int K>
__device__ __forceinline__ void gemm_xwt(f32x16& acc, const float* A, int lda, const float* __restrict__ B, int sj) {
    const int lane = threadIdx.x & 63, i = lane & 31, h = lane >> 5;
    const float* a = A + i * lda + 4 * h;
    const float* b = B + (size_t)i * sj + 4 * h;
#pragma unroll 4
    for (int k = 0; k < K; k += 8) {
        const f32x4 bv = *reinterpret_cast<const f32x4*>(b + k);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[k + e], bv[e], acc, 0, 0, 0);
    }
}

// acc[i][j] += sum_{k < 32} A[k][i0 + i] * B[k][j0 + j]:  both in LDS, the unit's rows are k
__device__ __forceinline__ void gemm_tn(f32x16& acc, const float* A, int lda, int i0, const float* B, int ldb, int j0) {
    const int lane = threadIdx.x & 63, i = lane & 31, h = lane >> 5;
    const float* a = A + h * lda + i0 + i;
    const float* b = B + h * ldb + j0 + i;
#pragma unroll 8
    for (int k = 0; k < 32; k += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[k * lda], b[k * ldb], acc, 0, 0, 0);
}

// row of accumulator register r for the lane half h (pwv_common.h)
__device__ __forceinline__ int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

__device__ __forceinline__ void acc_to_lds(const f32x16& acc, float* dst, int ld, int col0) {
    const int lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
#pragma unroll
    for (int r = 0; r < 16; ++r) dst[acc_row(r, h) * ld + col0 + j] = acc[r];
}

// a tile of a workgroup's partial: part[(i0 + i) * ld + j0 + j]
__device__ __forceinline__ void acc_to_part(const f32x16& acc, float* part, int ld, int i0, int j0) {
    const int lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
#pragma unroll
    for (int r = 0; r < 16; ++r) part[(size_t)(i0 + acc_row(r, h)) * ld + j0 + j] = acc[r];
}

__device__ __forceinline__ const float* t32_quad(const float* buf, int row, int q) {      // 64 channels
    return buf + (size_t)(row >> 5) * 2048 + q * 128 + (row & 31) * 4;
}

// 32 rows x 64 channels of an LDS array (columns col0 ..) -> block u of a tile32 buffer, 16 bytes per lane and store
__device__ __forceinline__ void lds_to_tile32(float* dst, int u, const float* src, int ld, int col0) {
    for (int idx = threadIdx.x; idx < 512; idx += kTrThreads) {
        const int q = idx >> 5, r = idx & 31;
        const float* s = src + r * ld + col0 + 4 * q;
        f32x4 v = {s[0], s[1], s[2], s[3]};
        *reinterpret_cast<f32x4*>(dst + (size_t)u * 2048 + q * 128 + r * 4) = v;
    }
}

// block u of a tile32 buffer -> LDS [32][ld] columns col0 ..; rows beyond the batch read as zeros
__device__ __forceinline__ void tile32_to_lds(float* dst, int ld, int col0, const float* src, int u, int rows) {
    for (int idx = threadIdx.x; idx < 512; idx += kTrThreads) {
        const int q = idx >> 5, r = idx & 31;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (32 * u + r < rows) v = *reinterpret_cast<const f32x4*>(src + (size_t)u * 2048 + q * 128 + r * 4);
        float* d = dst + r * ld + col0 + 4 * q;
        d[0] = v[0]; d[1] = v[1]; d[2] = v[2]; d[3] = v[3];
    }
}

__device__ __forceinline__ float sigmoid_f(float v) { return 1.f / (1.f + expf(-v)); }

// ------------------------------------------------------------------------------------------------------------------------------
// geometry policies: where row r of unit u (packed row `row` = 32 u + r < g.rows) lies in its utterance
//   t        its utterance-local sample          len      the samples of its utterance
//   frame    its P row                           first    the first packed row of P row f, which holds row r of this unit
// ------------------------------------------------------------------------------------------------------------------------------
struct UniformGeo {
    struct Loc {};
    __device__ static __forceinline__ void locate(Loc&, int, const Geom&, const PackedTables&) {}
    __device__ static __forceinline__ int t(const Loc&, int, int row, const Geom& g) { return row % g.T; }
    __device__ static __forceinline__ int len(const Loc&, int, const Geom& g) { return g.T; }
    __device__ static __forceinline__ int frame(const Loc&, int, int row, const Geom& g) {
        const int n = row / g.T, t = row - n * g.T;
        return n * g.frames + (t + g.off) / g.hop;
    }
    __device__ static __forceinline__ int slot(const Loc&, int, int f, int u, const Geom& g) {
        const int n = f / g.frames, fi = f - n * g.frames;
        int t0 = fi * g.hop - g.off;
        t0 = t0 < 0 ? 0 : t0;
        return u - ((n * g.T + t0) >> 5);
    }
};

struct PackedGeo {
    struct Loc {
        int t[33], len[33], fr[33], first[33];
    };
    // Threads 0 .. 32 find their row's utterance (the last i with cu_rows[i] <= row) and leave its place in LDS; a barrier publishes it.
    // Whatever the tables hold, 0 <= t <= row, row + (len - t) <= rows and 0 <= fr < prows: a look-back, a look-ahead and a P row
    // stay inside their buffers.  (The caller's loop ends on a barrier: nobody still reads the last unit's entries.)
    __device__ static __forceinline__ void locate(Loc& loc, int u, const Geom& g, const PackedTables& tab) {
        if (threadIdx.x < 33) {
            const int r = threadIdx.x, row = 32 * u + r;
            int t = 0, len = 0, fr = -1, first = 0;
            if (row < g.rows) {
                int lo = 0, hi = tab.n - 1;
                while (lo < hi) {
                    const int mid = (lo + hi + 1) >> 1;
                    if (tab.cu_rows[mid] <= row) lo = mid; else hi = mid - 1;
                }
                const int s = tab.cu_rows[lo], e = tab.cu_rows[lo + 1], f0 = tab.cu_frames[lo], f1 = tab.cu_frames[lo + 1];
                t = s < 0 ? row : (s > row ? 0 : row - s);
                int rest = e - row;                             // rows from this one to the utterance's end
                rest = rest < 1 ? 1 : (rest > g.rows - row ? g.rows - row : rest);
                len = t + rest;
                int fl = (t + g.off) / g.hop;                   // the frame within the utterance, at most its last
                fl = fl > f1 - f0 - 1 ? f1 - f0 - 1 : fl;
                fl = fl < 0 ? 0 : fl;
                fr = f0 + fl;
                fr = fr < 0 ? 0 : (fr > tab.prows - 1 ? tab.prows - 1 : fr);
                int t0 = fl * g.hop - g.off;
                t0 = t0 < 0 ? 0 : (t0 > t ? t : t0);
                first = row - t + t0;
            }
            loc.t[r] = t;
            loc.len[r] = len;
            loc.fr[r] = fr;
            loc.first[r] = first;
        }
        __syncthreads();
    }
    __device__ static __forceinline__ int t(const Loc& loc, int r, int, const Geom&) { return loc.t[r]; }
    __device__ static __forceinline__ int len(const Loc& loc, int r, const Geom&) { return loc.len[r]; }
    __device__ static __forceinline__ int frame(const Loc& loc, int r, int, const Geom&) { return loc.fr[r]; }
    __device__ static __forceinline__ int slot(const Loc& loc, int r, int, int u, const Geom& g) {
        const int k = u - (loc.first[r] >> 5);
        return k < 0 ? 0 : (k > g.kmax - 1 ? g.kmax - 1 : k);
    }
};

// the gradient that arrives for a layer's output, rows of unit u: U[t] + V[t + dnext] while t + dnext is inside the utterance
template <class Geo>
__device__ __forceinline__ void load_g(float* dst, int ld, const float* U, const float* V, int u, int nrows, const Geom& g,
                                       const typename Geo::Loc& loc) {
    for (int idx = threadIdx.x; idx < 16 * nrows; idx += kTrThreads) {
        const int q = idx / nrows, r = idx - q * nrows, row = 32 * u + r;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (row < g.rows) {
            v = *reinterpret_cast<const f32x4*>(t32_quad(U, row, q));
            const int t = Geo::t(loc, r, row, g);
            if (t + g.dnext < Geo::len(loc, r, g)) v += *reinterpret_cast<const f32x4*>(t32_quad(V, row + g.dnext, q));
        }
        float* d = dst + r * ld + 4 * q;
        d[0] = v[0]; d[1] = v[1]; d[2] = v[2]; d[3] = v[3];
    }
}

// a = [x[t - d] | x[t]] of unit u into LDS [32][kLdW]
template <class Geo>
__device__ __forceinline__ void load_a(float* a, const float* x, int u, const Geom& g, const typename Geo::Loc& loc) {
    for (int idx = threadIdx.x; idx < 1024; idx += kTrThreads) {
        const int q = idx >> 5, r = idx & 31, row = 32 * u + r;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (row < g.rows) {
            if (q >= 16) v = *reinterpret_cast<const f32x4*>(t32_quad(x, row, q - 16));
            else if (Geo::t(loc, r, row, g) >= g.d) v = *reinterpret_cast<const f32x4*>(t32_quad(x, row - g.d, q));
        }
        float* d = a + r * kLdW + 4 * q;
        d[0] = v[0]; d[1] = v[1]; d[2] = v[2]; d[3] = v[3];
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// skip policies: whether a layer feeds the net's skip sum S (tile32, 128 channels: block u = 4096 floats) and reads its gradient dS
//   Params      what the kernel takes beside the layer's parameters
//   Tile        the unit's dS rows in LDS (backward)             kPartFloats   what a workgroup's partial grows by: d skip [64][128]
// NoSkip is empty: a body instantiated with it is the text it was before the policy existed.
// ------------------------------------------------------------------------------------------------------------------------------
struct NoSkip {
    static constexpr bool kOn = false;
    static constexpr int kPartFloats = 0;
    struct Params {};
    struct Tile {};
};

struct SkipParams {
    const float *skip, *skip_bias;              // this layer's skip [64][128], skip_bias [128] or NULL
    float* sum;                                 // S (forward)
    const float* d_sum;                         // dS (backward)
    int accumulate;                             // forward: 0 = S is written (layer 0), 1 = S is added to
};

struct SumSkip {
    static constexpr bool kOn = true;
    static constexpr int kPartFloats = 64 * 128;
    using Params = SkipParams;
    struct Tile {
        float ds[32 * kLdW];
    };
};

// block u of a 128-channel tile32 buffer -> LDS [32][ld]; rows beyond the batch read as zeros.  RELU: max(v, 0)
template <bool RELU>
__device__ __forceinline__ void tile32w_to_lds(float* dst, int ld, const float* src, int u, int rows) {
    for (int idx = threadIdx.x; idx < 1024; idx += kTrThreads) {
        const int q = idx >> 5, r = idx & 31;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (32 * u + r < rows) v = *reinterpret_cast<const f32x4*>(src + (size_t)u * 4096 + q * 128 + r * 4);
        float* d = dst + r * ld + 4 * q;
#pragma unroll
        for (int e = 0; e < 4; ++e) d[e] = RELU ? fmaxf(v[e], 0.f) : v[e];
    }
}

// 32 rows x 128 channels of an LDS array -> block u of a 128-channel tile32 buffer, the rows of the batch alone (a padding row is
// neither read nor written); accumulate: dst + src, one rounding
__device__ __forceinline__ void lds_to_tile32w(float* dst, int u, const float* src, int ld, int rows, int accumulate) {
    for (int idx = threadIdx.x; idx < 1024; idx += kTrThreads) {
        const int q = idx >> 5, r = idx & 31;
        if (32 * u + r >= rows) continue;
        const float* s = src + r * ld + 4 * q;
        f32x4 v = {s[0], s[1], s[2], s[3]};
        f32x4* d = reinterpret_cast<f32x4*>(dst + (size_t)u * 4096 + q * 128 + r * 4);
        if (accumulate) v = *d + v;
        *d = v;
    }
}

struct LayerFwdParams {
    const float *x, *proj, *filter, *gate, *dense, *dense_bias;
    float* x_out;
    Geom g;
    int last;
    PackedTables tab;
};

struct LayerBwdParams {
    const float *x, *proj, *filter, *gate, *dense;
    const float *u_next, *v_next, *d_o;
    float *u, *v, *d_proj, *part;
    Geom g;
    PackedTables tab;
};

// ------------------------------------------------------------------------------------------------------------------------------
// conditioning policies: how the condition enters FG of a unit and how its gradient leaves
//   Params      what the kernel takes beside the layer's parameters
//   Tile        what `stage` leaves in LDS for the unit (a barrier of the body publishes it)
//   Acc         accumulators that live in registers over a workgroup's units and leave in `flush`
//   stage       fill the tile of unit u                  fg           FG = a Wfg + the conditioning term
//   unit_grad   the unit's share of the condition's gradient, from dFG in LDS
//   part_floats the floats of a workgroup's partial      flush        write what lies behind its first kLayerPart floats
// ProjCond: the condition is a row of the frame-rate projection P (Geom: hop, off, pstride, dpstride, kmax); SampleCond, a condition
// row per sample, is csrc/pwv_train_cond.hip's.  A hook holds its text itself: as a wrapper around a free function, one more level
// of inlining, `fg` cost the projection kernels registers ("One text for both conditionings").
// ------------------------------------------------------------------------------------------------------------------------------
struct ProjCond {
    static constexpr bool kProjected = true;
    struct Params {};
    struct Tile {
        int fr[32];                             // the P row of every row of the unit, -1 beyond the batch
    };
    struct Acc {};
    template <class Geo>
    __device__ static __forceinline__ void stage(Tile& tile, int u, const Geom& g, const typename Geo::Loc& loc, const Params&) {
        if (threadIdx.x < 32) {
            const int row = 32 * u + threadIdx.x;
            int f = -1;
            if (row < g.rows) f = Geo::frame(loc, threadIdx.x, row, g);
            tile.fr[threadIdx.x] = f;
        }
    }
    // FG = a Wfg + P into LDS fg [32][kLdW]: wave w owns columns 32 w .. 32 w + 31 (F: waves 0, 1; G: waves 2, 3)
    __device__ static __forceinline__ void fg(float* fg, const float* a, const Tile& tile, const float* filter, const float* gate, const float* proj,
                                              const Geom& g, const Params&) {
        const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
        f32x16 acc = zero16();
        gemm_xw<128>(acc, a, kLdW, (w < 2 ? filter : gate) + 32 * (w & 1), 64);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = acc_row(r, h), f = tile.fr[i];
            const float p = f >= 0 ? proj[(size_t)f * g.pstride + 32 * w + j] : 0.f;
            fg[i * kLdW + 32 * w + j] = acc[r] + p;
        }
    }
    // dP: threads 128 .. 255 sum column c of dFG over the rows of each frame, in row order, into the frame's slot of this unit
    template <class Geo>
    __device__ static __forceinline__ void unit_grad(Acc&, const Tile& tile, const float* fg, int u, const LayerBwdParams& p,
                                                     const typename Geo::Loc& loc, const Params&) {
        if (threadIdx.x >= 128) {
            const int c = threadIdx.x - 128;
            float s = 0.f;
            int cur = -1;
            for (int r = 0; r <= 32; ++r) {
                const int f = r < 32 ? tile.fr[r] : -1;
                if (f != cur) {
                    if (cur >= 0) {
                        const int k = Geo::slot(loc, r - 1, cur, u, p.g);
                        p.d_proj[((size_t)cur * p.g.kmax + k) * p.g.dpstride + c] = s;
                    }
                    cur = f;
                    s = 0.f;
                }
                if (f >= 0) s += fg[r * kLdW + c];
            }
        }
    }
    __host__ __device__ static __forceinline__ int part_floats(const Params&) { return kLayerPart; }
    __device__ static __forceinline__ void flush(const Acc&, float*, const Params&) {}
};

// ------------------------------------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------------------------------------
struct FrontFwdParams {
    const float *in, *cf;
    float* x0;
    Geom g;
    PackedTables tab;
};

// x_0[t] = in[t - 1] cf[0] + in[t] cf[1], in[-1] = 0 at every utterance's first sample; one unit per workgroup
template <class Geo>
__device__ __forceinline__ void front_fwd_body(const FrontFwdParams& p) {
    __shared__ typename Geo::Loc loc;
    const int u = blockIdx.x;
    Geo::locate(loc, u, p.g, p.tab);
    for (int idx = threadIdx.x; idx < 512; idx += kTrThreads) {
        const int q = idx >> 5, r = idx & 31, row = 32 * u + r;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (row < p.g.rows) {
            const float cur = p.in[row], prev = Geo::t(loc, r, row, p.g) > 0 ? p.in[row - 1] : 0.f;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = prev * p.cf[4 * q + e] + cur * p.cf[64 + 4 * q + e];
        }
        *reinterpret_cast<f32x4*>(p.x0 + (size_t)u * 2048 + q * 128 + r * 4) = v;
    }
}

template <class Geo, class Cond, class Skip = NoSkip>
__device__ __forceinline__ void layer_fwd_body(const LayerFwdParams& p, const typename Cond::Params& cp, const typename Skip::Params& sp = {}) {
    __shared__ float a[32 * kLdW];
    __shared__ float fg[32 * kLdW];
    __shared__ float o[32 * kLdH];
    __shared__ typename Cond::Tile tile;
    __shared__ typename Geo::Loc loc;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
    const int units = (p.g.rows + 31) / 32;
    for (int u = blockIdx.x; u < units; u += gridDim.x) {
        Geo::locate(loc, u, p.g, p.tab);
        load_a<Geo>(a, p.x, u, p.g, loc);
        Cond::template stage<Geo>(tile, u, p.g, loc, cp);
        __syncthreads();
        Cond::fg(fg, a, tile, p.filter, p.gate, p.proj, p.g, cp);
        __syncthreads();
        for (int idx = threadIdx.x; idx < 2048; idx += kTrThreads) {
            const int r = idx >> 6, c = idx & 63;
            o[r * kLdH + c] = tanhf(fg[r * kLdW + c]) * sigmoid_f(fg[r * kLdW + 64 + c]);
        }
        __syncthreads();
        if constexpr (Skip::kOn) {
            // o skip + skip_bias, columns 32 w .., into fg (FG is spent); x + o dense + dense_bias into columns 0 .. 63 of a (the tap at
            // t - d is spent, and wave w reads and writes its own columns): no barrier between the two
            {
                f32x16 acc = zero16();
                gemm_xw<64>(acc, o, kLdH, sp.skip + 32 * w, 128);
                const float b = sp.skip_bias ? sp.skip_bias[32 * w + j] : 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) fg[acc_row(r, h) * kLdW + 32 * w + j] = acc[r] + b;
            }
            if (!p.last && w < 2) {
                f32x16 acc = zero16();
                gemm_xw<64>(acc, o, kLdH, p.dense + 32 * w, 64);
                const float b = p.dense_bias ? p.dense_bias[32 * w + j] : 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int i = acc_row(r, h);
                    a[i * kLdW + 32 * w + j] = a[i * kLdW + 64 + 32 * w + j] + acc[r] + b;
                }
            }
            __syncthreads();
            lds_to_tile32w(sp.sum, u, fg, kLdW, p.g.rows, sp.accumulate);
            if (!p.last) lds_to_tile32(p.x_out, u, a, kLdW, 0);
        } else if (p.last) {
            lds_to_tile32(p.x_out, u, o, kLdH, 0);
        } else {
            if (w < 2) {        // x + o dense + dense_bias, columns 32 w ..
                f32x16 acc = zero16();
                gemm_xw<64>(acc, o, kLdH, p.dense + 32 * w, 64);
                const float b = p.dense_bias ? p.dense_bias[32 * w + j] : 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int i = acc_row(r, h);
                    fg[i * kLdW + 32 * w + j] = a[i * kLdW + 64 + 32 * w + j] + acc[r] + b;
                }
            }
            __syncthreads();
            lds_to_tile32(p.x_out, u, fg, kLdW, 0);
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// backward
// ------------------------------------------------------------------------------------------------------------------------------
template <class Geo, class Cond, bool LAST, class Skip = NoSkip>
__device__ __forceinline__ void layer_bwd_body(const LayerBwdParams& p, const typename Cond::Params& cp, const typename Skip::Params& sp = {}) {
    __shared__ float a[32 * kLdW];              // [x[t - d] | x[t]], then [V | U]
    __shared__ float fg[32 * kLdW];             // FG, then dFG
    __shared__ float od[32 * kLdH];             // d o, then o: the gating pass replaces element by element ("LDS: aliasing")
    __shared__ float gin[32 * kLdH];            // g
    __shared__ typename Cond::Tile tile;
    __shared__ typename Skip::Tile stile;       // dS
    __shared__ typename Geo::Loc loc;
    const int w = threadIdx.x >> 6;
    const int units = (p.g.rows + 31) / 32;
    f32x16 g_wfg[4], g_dense = zero16(), g_skip[2];
#pragma unroll
    for (int b = 0; b < 4; ++b) g_wfg[b] = zero16();
    g_skip[0] = zero16();
    g_skip[1] = zero16();
    float g_db = 0.f;                           // thread c < 64: d dense_bias[c]
    typename Cond::Acc g_cond;
    for (int u = blockIdx.x; u < units; u += gridDim.x) {
        Geo::locate(loc, u, p.g, p.tab);
        load_a<Geo>(a, p.x, u, p.g, loc);
        Cond::template stage<Geo>(tile, u, p.g, loc, cp);
        if constexpr (Skip::kOn) tile32w_to_lds<false>(stile.ds, kLdW, sp.d_sum, u, p.g.rows);
        if (LAST && !Skip::kOn) tile32_to_lds(od, kLdH, 0, p.d_o, u, p.g.rows);
        if (!LAST) load_g<Geo>(gin, kLdH, p.u_next, p.v_next, u, 32, p.g, loc);
        __syncthreads();
        Cond::fg(fg, a, tile, p.filter, p.gate, p.proj, p.g, cp);
        if ((!LAST || Skip::kOn) && w < 2) {    // d o = g dense^T (+ dS skip^T), columns 32 w ..
            f32x16 acc = zero16();
            if (!LAST) gemm_xwt<64>(acc, gin, kLdH, p.dense + (size_t)32 * w * 64, 64);
            if constexpr (Skip::kOn) gemm_xwt<128>(acc, stile.ds, kLdW, sp.skip + (size_t)32 * w * 128, 128);
            acc_to_lds(acc, od, kLdH, 32 * w);
        }
        __syncthreads();
        for (int idx = threadIdx.x; idx < 2048; idx += kTrThreads) {
            const int r = idx >> 6, c = idx & 63;
            const float th = tanhf(fg[r * kLdW + c]), sg = sigmoid_f(fg[r * kLdW + 64 + c]), d = od[r * kLdH + c];
            od[r * kLdH + c] = th * sg;
            fg[r * kLdW + c] = d * sg * (1.f - th * th);
            fg[r * kLdW + 64 + c] = d * th * sg * (1.f - sg);
        }
        __syncthreads();
        for (int b = 0; b < 4; ++b) gemm_tn(g_wfg[b], a, kLdW, 32 * b, fg, kLdW, 32 * w);         // dWfg += a^T dFG
        if (!LAST) {
            gemm_tn(g_dense, od, kLdH, 32 * (w >> 1), gin, kLdH, 32 * (w & 1));                   // d dense += o^T g
            if (threadIdx.x < 64)
                for (int r = 0; r < 32; ++r) g_db += gin[r * kLdH + threadIdx.x];
        }
        if constexpr (Skip::kOn)
            for (int b = 0; b < 2; ++b) gemm_tn(g_skip[b], od, kLdH, 32 * b, stile.ds, kLdW, 32 * w);   // d skip += o^T dS
        Cond::template unit_grad<Geo>(g_cond, tile, fg, u, p, loc, cp);
        // [V | U] = dFG Wfg^T: wave w owns input channels 32 w .. of the 128 (0..63: the tap at t - d, 64..127: the tap at t)
        f32x16 acc = zero16();
        gemm_xwt<64>(acc, fg, kLdW, p.filter + (size_t)32 * w * 64, 64);
        gemm_xwt<64>(acc, fg + 64, kLdW, p.gate + (size_t)32 * w * 64, 64);
        __syncthreads();                        // every wave has read a
        acc_to_lds(acc, a, kLdW, 32 * w);
        __syncthreads();
        if (!LAST) {
            for (int idx = threadIdx.x; idx < 2048; idx += kTrThreads) {
                const int r = idx >> 6, c = idx & 63;
                a[r * kLdW + 64 + c] += gin[r * kLdH + c];
            }
            __syncthreads();
        }
        lds_to_tile32(p.v, u, a, kLdW, 0);
        lds_to_tile32(p.u, u, a, kLdW, 64);
        __syncthreads();
    }
    float* part = p.part + (size_t)blockIdx.x * (Cond::part_floats(cp) + Skip::kPartFloats);
    for (int b = 0; b < 4; ++b) acc_to_part(g_wfg[b], part, 128, 32 * b, 32 * w);
    if (!LAST) {
        acc_to_part(g_dense, part + 128 * 128, 64, 32 * (w >> 1), 32 * (w & 1));
        if (threadIdx.x < 64) part[128 * 128 + 64 * 64 + threadIdx.x] = g_db;
    }
    Cond::flush(g_cond, part + kLayerPart, cp);
    if constexpr (Skip::kOn)
        for (int b = 0; b < 2; ++b) acc_to_part(g_skip[b], part + Cond::part_floats(cp), 128, 32 * b, 32 * w);
}

struct FrontBwdParams {
    const float *in, *cf, *u_next, *v_next, *d_out, *scale;
    float *d_in, *part;
    Geom g;
    int accumulate;
    PackedTables tab;
};

template <class Geo>
__device__ __forceinline__ void front_bwd_body(const FrontBwdParams& p) {
    __shared__ float g0[33 * kLdH];             // the gradient for x_0, rows of the unit and the first row behind it
    __shared__ float s_in[34];                  // in[32 u - 1 .. 32 u + 32]
    __shared__ float s_a[33], s_b[33];          // g0 . cf[1], g0 . cf[0]
    __shared__ typename Geo::Loc loc;
    const int units = (p.g.rows + 31) / 32;
    float g_cf0 = 0.f, g_cf1 = 0.f;             // thread c < 64
    for (int u = blockIdx.x; u < units; u += gridDim.x) {
        Geo::locate(loc, u, p.g, p.tab);
        load_g<Geo>(g0, kLdH, p.u_next, p.v_next, u, 33, p.g, loc);
        if (threadIdx.x < 34) {
            const int row = 32 * u - 1 + threadIdx.x;
            s_in[threadIdx.x] = row >= 0 && row < p.g.rows ? p.in[row] : 0.f;
        }
        __syncthreads();
        if (threadIdx.x < 64) {
            const int c = threadIdx.x;
            for (int r = 0; r < 32; ++r) {
                const int row = 32 * u + r;
                if (row >= p.g.rows) break;
                const float gv = g0[r * kLdH + c];
                if (Geo::t(loc, r, row, p.g) > 0) g_cf0 += s_in[r] * gv;
                g_cf1 += s_in[r + 1] * gv;
            }
        } else if (threadIdx.x < 64 + 33) {
            const int r = threadIdx.x - 64;
            float sa = 0.f, sb = 0.f;
            for (int c = 0; c < 64; ++c) {
                const float gv = g0[r * kLdH + c];
                sb += gv * p.cf[c];
                sa += gv * p.cf[64 + c];
            }
            s_a[r] = sa;
            s_b[r] = sb;
        }
        __syncthreads();
        if (threadIdx.x < 32 && p.d_in) {
            const int r = threadIdx.x, row = 32 * u + r;
            if (row < p.g.rows) {
                float v = p.accumulate ? p.d_in[row] : (p.d_out && p.scale ? p.d_out[row] * p.scale[row] : 0.f);
                v += s_a[r];
                if (Geo::t(loc, r, row, p.g) + 1 < Geo::len(loc, r, p.g)) v += s_b[r + 1];
                p.d_in[row] = v;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x < 64) {
        float* part = p.part + (size_t)blockIdx.x * kFrontPart;
        part[threadIdx.x] = g_cf0;
        part[64 + threadIdx.x] = g_cf1;
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// host: stage two of every weight gradient (train_reduce_kernel, csrc/pwv_train.hip) and the entry points every ABI struct shares
// ------------------------------------------------------------------------------------------------------------------------------
struct ReduceSeg {
    int begin, end;                             // elements [begin, end) of a partial
    float* dst;                                 // NULL: not wanted
    float* dst2;                                // begin == 0 of a layer: d_gate (the segment is dWfg [128][128] = [k][filter | gate])
};
struct ReduceParams {
    const float* part;
    int n_part, stride, total, n_seg;
    ReduceSeg seg[6];
};

int train_reduce(const ReduceParams& rp, hipStream_t st);
int train_grid_size(int max_workgroups, int units);
// what every uniform entry point checks first: the struct (`field` of size `size` = sizeof(`name`)), N, T, N T and max_workgroups
int train_check_batch(const pwv_train_args* a, const char* who, const char* field, size_t size, const char* name);

// The four entry-point kinds that depend on where an utterance begins, once for every ABI struct: pwv_train_args (also as the head of
// pwv_train_cond_args) and pwv_train_varlen_args share the names of the fields read here.  The caller has checked the struct and its
// geometry and filled `g`, `tab` and the condition's parameters; `launch` enqueues its kernel on its stream.
template <class Args>
int train_check_ws(const Args* a, const char* who, int grid, int part) {
    PWV_CHECK_ARG(a->workspace, "%s: workspace is a NULL pointer", who);
    PWV_CHECK_ARG(a->workspace_bytes >= (size_t)grid * part * sizeof(float), "%s: workspace_bytes %zu is short of %zu", who, a->workspace_bytes,
                  (size_t)grid * part * sizeof(float));
    return PWV_OK;
}

template <class Args, class Launch>
int train_front_fwd(const Args* a, const char* who, const Geom& g, const PackedTables& tab, Launch launch) {      // launch(grid, p)
    PWV_CHECK_ARG(a->in && a->causal_filter && a->x_out, "%s: in, causal_filter or x_out is a NULL pointer", who);
    FrontFwdParams p{};
    p.in = a->in; p.cf = a->causal_filter; p.x0 = a->x_out;
    p.g = g;
    p.tab = tab;
    launch((g.rows + 31) / 32, p);
    PWV_CHECK_HIP(hipGetLastError());
    return PWV_OK;
}

template <class Cond, class Args, class Launch>
int train_layer_fwd(const Args* a, const char* who, const Geom& g, const PackedTables& tab, Launch launch) {      // launch(grid, p)
    PWV_CHECK_ARG(a->form == PWV_TRAIN_RESIDUAL || a->form == PWV_TRAIN_LAST, "%s: form %d", who, a->form);
    PWV_CHECK_ARG(a->x && a->filter && a->gate && a->x_out, "%s: x, filter, gate or x_out is a NULL pointer", who);
    PWV_CHECK_ARG(!Cond::kProjected || a->proj, "%s: proj is a NULL pointer", who);
    PWV_CHECK_ARG(a->form == PWV_TRAIN_LAST || a->dense, "%s: dense is a NULL pointer", who);
    LayerFwdParams p{};
    p.x = a->x; p.proj = a->proj; p.filter = a->filter; p.gate = a->gate; p.dense = a->dense; p.dense_bias = a->dense_bias;
    p.x_out = a->x_out;
    p.g = g;
    p.last = a->form == PWV_TRAIN_LAST;
    p.tab = tab;
    launch(train_grid_size(a->max_workgroups, (g.rows + 31) / 32), p);
    PWV_CHECK_HIP(hipGetLastError());
    return PWV_OK;
}

// `extra`: the segments of the partial behind its first kLayerPart floats (Cond::flush), reduced with the layer's own
template <class Cond, class Args, class Launch>
int train_layer_bwd(const Args* a, const char* who, const Geom& g, const PackedTables& tab, const typename Cond::Params& cp, const ReduceSeg* extra,
                    int n_extra, hipStream_t st, Launch launch) {                                                 // launch(last, grid, p)
    PWV_CHECK_ARG(a->form == PWV_TRAIN_RESIDUAL || a->form == PWV_TRAIN_LAST, "%s: form %d", who, a->form);
    const bool last = a->form == PWV_TRAIN_LAST;
    PWV_CHECK_ARG(a->x && a->filter && a->gate, "%s: x, filter or gate is a NULL pointer", who);
    PWV_CHECK_ARG(a->u && a->v && a->d_filter && a->d_gate, "%s: u, v, d_filter or d_gate is a NULL pointer", who);
    if (Cond::kProjected) {
        PWV_CHECK_ARG(a->proj && a->d_proj, "%s: proj or d_proj is a NULL pointer", who);
        PWV_CHECK_ARG(a->d_proj_row_stride >= 128, "%s: d_proj_row_stride %d is below 128", who, a->d_proj_row_stride);
    }
    if (last) {
        PWV_CHECK_ARG(a->d_o, "%s: d_o is a NULL pointer", who);
    } else {
        PWV_CHECK_ARG(a->dense && a->u_next && a->v_next && a->d_dense, "%s: dense, u_next, v_next or d_dense is a NULL pointer", who);
        PWV_CHECK_ARG(a->next_dilation >= 1, "%s: next_dilation %d must be >= 1", who, a->next_dilation);
        PWV_CHECK_ARG(a->u != a->u_next && a->v != a->v_next && a->u != a->v_next && a->v != a->u_next, "%s: u / v alias u_next / v_next", who);
    }
    const int grid = train_grid_size(a->max_workgroups, (g.rows + 31) / 32), part = Cond::part_floats(cp);
    if (int e = train_check_ws(a, who, grid, part)) return e;
    LayerBwdParams p{};
    p.x = a->x; p.proj = a->proj; p.filter = a->filter; p.gate = a->gate; p.dense = a->dense;
    p.u_next = a->u_next; p.v_next = a->v_next; p.d_o = a->d_o;
    p.u = a->u; p.v = a->v; p.d_proj = a->d_proj; p.part = (float*)a->workspace;
    p.g = g;
    p.tab = tab;
    launch(last, grid, p);
    PWV_CHECK_HIP(hipGetLastError());
    // stage two: dWfg | d dense | d dense_bias | extra; a PWV_TRAIN_LAST layer has no dense, and what nobody wants at the end is not summed
    ReduceParams rp;
    rp.part = p.part; rp.n_part = grid; rp.stride = part;
    rp.seg[0] = ReduceSeg{0, 128 * 128, a->d_filter, a->d_gate};
    rp.seg[1] = ReduceSeg{128 * 128, 128 * 128 + 64 * 64, last ? nullptr : a->d_dense, nullptr};
    rp.seg[2] = ReduceSeg{128 * 128 + 64 * 64, kLayerPart, last ? nullptr : a->d_dense_bias, nullptr};
    PWV_CHECK_ARG(3 + n_extra <= (int)(sizeof(rp.seg) / sizeof(rp.seg[0])), "%s: %d segments behind the layer's own are more than a reduction holds", who, n_extra);
    for (int s = 0; s < n_extra; ++s) rp.seg[3 + s] = extra[s];
    rp.n_seg = 3 + n_extra;
    while (rp.n_seg > 1 && !rp.seg[rp.n_seg - 1].dst) --rp.n_seg;
    rp.total = rp.seg[rp.n_seg - 1].end;
    return train_reduce(rp, st);
}

template <class Args, class Launch>
int train_front_bwd(const Args* a, const char* who, const Geom& g, const PackedTables& tab, hipStream_t st, Launch launch) {  // launch(grid, p)
    PWV_CHECK_ARG(a->in && a->causal_filter && a->u_next && a->v_next && a->d_causal_filter,
                  "%s: in, causal_filter, u_next, v_next or d_causal_filter is a NULL pointer", who);
    PWV_CHECK_ARG(a->next_dilation >= 1, "%s: next_dilation %d must be >= 1", who, a->next_dilation);
    const int grid = train_grid_size(a->max_workgroups, (g.rows + 31) / 32);
    if (int e = train_check_ws(a, who, grid, kFrontPart)) return e;
    FrontBwdParams p{};
    p.in = a->in; p.cf = a->causal_filter; p.u_next = a->u_next; p.v_next = a->v_next; p.d_out = a->d_out; p.scale = a->scale;
    p.d_in = a->d_in; p.part = (float*)a->workspace; p.accumulate = a->accumulate;
    p.g = g;
    p.tab = tab;
    launch(grid, p);
    PWV_CHECK_HIP(hipGetLastError());
    ReduceParams rp;
    rp.part = p.part; rp.n_part = grid; rp.stride = kFrontPart; rp.total = kFrontPart; rp.n_seg = 1;
    rp.seg[0] = ReduceSeg{0, kFrontPart, a->d_causal_filter, nullptr};
    return train_reduce(rp, st);
}

}  // namespace pwv

#endif  // PWV_TRAIN_UNITS_H
