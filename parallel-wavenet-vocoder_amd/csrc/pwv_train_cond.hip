// Training with a per-sample condition (include/pwv_hip_train_cond.h; DESIGN.md section 9, "Training the transposed-conv
// conditioning"): the layer forward and backward of csrc/pwv_train.hip with the conditioning product c[t] Gc and its gradients inside
// the unit -- the condition of the transposed-conv upsampler changes every sample, so nothing of it can be hoisted to frame rate.
// Uniform [N, T] batches; the kernels are the layer bodies of pwv_train_units.h instantiated with the conditioning policy SampleCond
// below, so the unit scheme (32 rows, 256 threads = 4 waves, one 32 x 32 tile per wave and GEMM call), the partial-then-ordered-reduce
// of the weight gradients and the host text of the entry points are the ones every training layer has.  The condition tile of a unit
// lies in LDS as [32][97], columns C .. 95 zero: as the A operand of c Gc its K loop stops at C, as the A^T operand of c^T dFG its
// zero columns give zero tiles that are not written to the partial.
#include "pwv_common.h"
#include "pwv_hip_train_cond.h"
#include "pwv_train_head.h"

namespace pwv {

constexpr int kCondMax = PWV_TRAIN_COND_MAX;      // columns of the LDS tile
constexpr int kLdC = kCondMax + 1;

struct CondParams {
    const float *c, *gc_filter, *gc_gate, *filter_bias, *gate_bias;
    float* d_c;
    int C, stride, utt_rows, accumulate;
};

// where the condition row of packed row `row` begins, in floats
__device__ __forceinline__ size_t cond_row(int row, const Geom& g, const CondParams& cp) {
    const int n = row / g.T;
    return ((size_t)n * cp.utt_rows + (row - n * g.T)) * cp.stride;
}

// gemm_xwt over a weight of which only `valid` rows exist: acc[i][j] += sum_{k < K} A[i][k] * B[j][k] for j < valid, + 0 beyond.  A lane
// whose row does not exist loads row 0 instead and multiplies zeros.
template <int K>
__device__ __forceinline__ void gemm_xwt_rows(f32x16& acc, const float* A, int lda, const float* __restrict__ B, int sj, int valid) {
    const int lane = threadIdx.x & 63, i = lane & 31, h = lane >> 5;
    const bool ok = i < valid;
    const float* a = A + i * lda + 4 * h;
    const float* b = B + (size_t)(ok ? i : 0) * sj + 4 * h;
#pragma unroll 4
    for (int k = 0; k < K; k += 8) {
        const f32x4 bv = *reinterpret_cast<const f32x4*>(b + k);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[k + e], ok ? bv[e] : 0.f, acc, 0, 0, 0);
    }
}

constexpr int kCondBlocks = kCondMax / 32;      // 32-row blocks of d_gc

// the conditioning policy of a per-sample condition (pwv_train_units.h, "conditioning policies"); uniform batches only: cond_row
struct SampleCond {
    static constexpr bool kProjected = false;
    using Params = CondParams;
    struct Tile {
        float c[32 * kLdC];
    };
    struct Acc {
        f32x16 gc[kCondBlocks];                 // d_gc, 32 condition channels x this wave's 32 columns of FG each
        float b = 0.f;                          // thread 128 + col: d_b[col]
        __device__ __forceinline__ Acc() {
#pragma unroll
            for (int k = 0; k < kCondBlocks; ++k) gc[k] = zero16();
        }
    };
    // the condition rows of unit u into LDS [32][kLdC]; columns >= C and rows beyond the batch are zeros.  A wave takes a row at a time
    // (its place is wave-uniform arithmetic) and its lanes the row's columns lane and 64 + lane: 256 + 128 contiguous bytes
    template <class Geo>
    __device__ static __forceinline__ void stage(Tile& tile, int u, const Geom& g, const typename Geo::Loc&, const Params& cp) {
        const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
        static_assert(kCondMax <= 128, "two columns per lane");
        for (int r = w; r < 32; r += kTrThreads / 64) {
            const int row = 32 * u + r;
            const bool in = row < g.rows;
            const float* src = cp.c + (in ? cond_row(row, g, cp) : 0);
            tile.c[r * kLdC + lane] = in && lane < cp.C ? src[lane] : 0.f;
            if (lane < kCondMax - 64) tile.c[r * kLdC + 64 + lane] = in && 64 + lane < cp.C ? src[64 + lane] : 0.f;
        }
    }
    // FG = a Wfg + c Gc + b into LDS fg [32][kLdW]: wave w owns columns 32 w .. 32 w + 31 (F: waves 0, 1; G: waves 2, 3).  The K loop
    // of c Gc ends at C (even: the MFMA takes two values of k a step), so no row >= C of gc_filter / gc_gate is read.
    __device__ static __forceinline__ void fg(float* fg, const float* a, const Tile& tile, const float* filter, const float* gate, const float*,
                                              const Geom&, const Params& cp) {
        const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
        f32x16 acc = zero16();
        gemm_xw<128>(acc, a, kLdW, (w < 2 ? filter : gate) + 32 * (w & 1), 64);
        const float* ca = tile.c + j * kLdC + h;
        const float* gb = (w < 2 ? cp.gc_filter : cp.gc_gate) + 32 * (w & 1) + (size_t)h * 64 + j;
#pragma unroll 8
        for (int k = 0; k < cp.C; k += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ca[k], gb[(size_t)k * 64], acc, 0, 0, 0);
        const float* bias = w < 2 ? cp.filter_bias : cp.gate_bias;
        const float b = bias ? bias[32 * (w & 1) + j] : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) fg[acc_row(r, h) * kLdW + 32 * w + j] = acc[r] + b;
    }
    template <class Geo>
    __device__ static __forceinline__ void unit_grad(Acc& acc, const Tile& tile, const float* fg, int u, const LayerBwdParams& p,
                                                     const typename Geo::Loc&, const Params& cp) {
        const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
#pragma unroll
        for (int b = 0; b < kCondBlocks; ++b) gemm_tn(acc.gc[b], tile.c, kLdC, 32 * b, fg, kLdW, 32 * w);      // d_gc += c^T dFG
        if (threadIdx.x >= 128) {               // d_b: column col of dFG over the rows, in row order (rows beyond the batch hold zeros)
            const int col = threadIdx.x - 128;
            for (int r = 0; r < 32; ++r) acc.b += fg[r * kLdW + col];
        }
        // d_cond = dFG Gc^T: wave w owns condition channels 32 w .. while they exist; a row of d_cond belongs to this unit alone
        if (32 * w < cp.C) {
            f32x16 dc = zero16();
            gemm_xwt_rows<64>(dc, fg, kLdW, cp.gc_filter + (size_t)32 * w * 64, 64, cp.C - 32 * w);
            gemm_xwt_rows<64>(dc, fg + 64, kLdW, cp.gc_gate + (size_t)32 * w * 64, 64, cp.C - 32 * w);
            const int k = 32 * w + j;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = 32 * u + acc_row(r, h);
                if (row < p.g.rows && k < cp.C) {
                    float* dst = cp.d_c + cond_row(row, p.g, cp) + k;
                    *dst = cp.accumulate ? *dst + dc[r] : dc[r];
                }
            }
        }
    }
    // the partial: dWfg | d dense | d dense_bias | d_gc [C][128] | d_b [128]
    __host__ __device__ static __forceinline__ int part_floats(const Params& cp) { return kLayerPart + cp.C * 128 + 128; }
    __device__ static __forceinline__ void flush(const Acc& acc, float* gc, const Params& cp) {
        const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
#pragma unroll
        for (int b = 0; b < kCondBlocks; ++b) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int k = 32 * b + acc_row(r, h);
                if (k < cp.C) gc[(size_t)k * 128 + 32 * w + j] = acc.gc[b][r];
            }
        }
        if (threadIdx.x >= 128) gc[(size_t)cp.C * 128 + threadIdx.x - 128] = acc.b;
    }
};

__global__ __launch_bounds__(kTrThreads) void train_cond_layer_fwd_kernel(LayerFwdParams p, CondParams cp) {
    layer_fwd_body<UniformGeo, SampleCond>(p, cp);
}

// Eight accumulator tiles stay in registers over a workgroup's units (dWfg 4, d_gc 3, d dense 1); the second launch bound holds the
// kernel to the 256 registers per lane at which two workgroups share a compute unit, as the default grid of two per CU assumes
template <bool LAST>
__global__ __launch_bounds__(kTrThreads, 2) void train_cond_layer_bwd_kernel(LayerBwdParams p, CondParams cp) {
    layer_bwd_body<UniformGeo, SampleCond, LAST>(p, cp);
}

// what both entry points and the workspace size check; fills the geometry and the condition's parameters
static int cond_check(const pwv_train_cond_args* c, const char* who, bool sizes_only, Geom& g, CondParams& cp) {
    PWV_CHECK_ARG(c, "%s: args is NULL", who);
    const pwv_train_args* a = &c->train;
    if (int e = train_check_batch(a, who, "train.struct_size", sizeof(pwv_train_cond_args), "pwv_train_cond_args")) return e;
    PWV_CHECK_ARG(c->cond_channels >= 2 && c->cond_channels <= kCondMax && c->cond_channels % 2 == 0,
                  "%s: cond_channels %d must be even and in 2 .. %d", who, c->cond_channels, kCondMax);
    cp = CondParams{c->cond, c->gc_filter, c->gc_gate, c->filter_bias, c->gate_bias, c->d_cond,
                    c->cond_channels, c->cond_row_stride, c->cond_utt_rows, c->d_cond_accumulate != 0};
    if (sizes_only) return PWV_OK;
    PWV_CHECK_ARG(a->dilation >= 1, "%s: dilation %d must be >= 1", who, a->dilation);
    PWV_CHECK_ARG(c->cond, "%s: cond is a NULL pointer", who);
    PWV_CHECK_ARG(c->cond_row_stride >= c->cond_channels, "%s: cond_row_stride %d is below cond_channels %d", who, c->cond_row_stride,
                  c->cond_channels);
    PWV_CHECK_ARG(c->cond_utt_rows >= a->T, "%s: cond_utt_rows %d is below T = %d", who, c->cond_utt_rows, a->T);
    PWV_CHECK_ARG((long long)a->N * c->cond_utt_rows < (1ll << 31), "%s: N cond_utt_rows = %lld is beyond int32", who,
                  (long long)a->N * c->cond_utt_rows);
    PWV_CHECK_ARG(!a->proj && !a->d_proj, "%s: proj and d_proj must be NULL (the condition is per sample: there is no frame-rate projection)", who);
    PWV_CHECK_ARG(c->gc_filter && c->gc_gate, "%s: gc_filter or gc_gate is a NULL pointer", who);
    g = Geom{};                                 // (no frame-rate field is read)
    g.rows = a->N * a->T;
    g.T = a->T;
    g.d = a->dilation;
    g.dnext = a->next_dilation;
    return PWV_OK;
}

}  // namespace pwv

using namespace pwv;

extern "C" size_t pwv_train_cond_workspace_bytes(const pwv_train_cond_args* c) {
    Geom g;
    CondParams cp;
    if (cond_check(c, "pwv_train_cond_workspace_bytes", true, g, cp) != PWV_OK) return 0;
    const int units = (c->train.N * c->train.T + 31) / 32, part = SampleCond::part_floats(cp);
    return (size_t)train_grid_size(c->train.max_workgroups, units) * (part > kMaxPart ? part : kMaxPart) * sizeof(float);
}

extern "C" int pwv_train_cond_layer_fwd_f32(const pwv_train_cond_args* c, pwv_stream_t stream) {
    const char* who = "pwv_train_cond_layer_fwd_f32";
    Geom g;
    CondParams cp;
    if (int e = cond_check(c, who, false, g, cp)) return e;
    return train_layer_fwd<SampleCond>(&c->train, who, g, PackedTables{}, [&](int grid, const LayerFwdParams& p) {
        hipLaunchKernelGGL(train_cond_layer_fwd_kernel, dim3(grid), dim3(kTrThreads), 0, (hipStream_t)stream, p, cp);
    });
}

extern "C" int pwv_train_cond_layer_bwd_f32(const pwv_train_cond_args* c, pwv_stream_t stream) {
    const char* who = "pwv_train_cond_layer_bwd_f32";
    Geom g;
    CondParams cp;
    if (int e = cond_check(c, who, false, g, cp)) return e;
    PWV_CHECK_ARG(c->d_cond && c->d_gc_filter && c->d_gc_gate, "%s: d_cond, d_gc_filter or d_gc_gate is a NULL pointer", who);
    // stage two of d_gc [C][128] (its rows split into [C][64] | [C][64]) and of d_b [128], behind the layer's own segments
    const int at_b = kLayerPart + cp.C * 128;
    const ReduceSeg extra[3] = {{kLayerPart, at_b, c->d_gc_filter, c->d_gc_gate},
                                {at_b, at_b + 64, c->d_filter_bias, nullptr},
                                {at_b + 64, at_b + 128, c->d_gate_bias, nullptr}};
    return train_layer_bwd<SampleCond>(&c->train, who, g, PackedTables{}, cp, extra, 3, (hipStream_t)stream,
                                       [&](bool last, int grid, const LayerBwdParams& p) {
        if (last) hipLaunchKernelGGL(train_cond_layer_bwd_kernel<true>, dim3(grid), dim3(kTrThreads), 0, (hipStream_t)stream, p, cp);
        else hipLaunchKernelGGL(train_cond_layer_bwd_kernel<false>, dim3(grid), dim3(kTrThreads), 0, (hipStream_t)stream, p, cp);
    });
}
