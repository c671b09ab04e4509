// Training with a per-sample condition (include/pwv_hip_train_cond.h; DESIGN.md section 9, "Training the transposed-conv
// conditioning"): the layer forward and backward of csrc/pwv_train.hip with the conditioning product c[t] Gc and its gradients inside
// the unit -- the condition of the transposed-conv upsampler changes every sample, so nothing of it can be hoisted to frame rate.
// Uniform [N, T] batches; the helpers, the unit scheme (32 rows, 256 threads = 4 waves, one 32 x 32 tile per wave and GEMM call) and the
// partial-then-ordered-reduce of the weight gradients are those of pwv_train_units.h.  The condition tile of a unit lies in LDS as
// [32][97], columns C .. 95 zero: as the A operand of c Gc its K loop stops at C, as the A^T operand of c^T dFG its zero columns give
// zero tiles that are not written to the partial.
#include "pwv_common.h"
#include "pwv_hip_train_cond.h"
#include "pwv_train_units.h"

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

// the condition rows of unit u into LDS [32][kLdC]; columns >= C and rows beyond the batch are zeros.  A wave takes a row at a time (its
// place is wave-uniform arithmetic) and its lanes the row's columns lane and 64 + lane: 256 + 128 contiguous bytes
__device__ __forceinline__ void load_c(float* c, int u, const Geom& g, const CondParams& cp) {
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    static_assert(kCondMax <= 128, "two columns per lane");
    for (int r = w; r < 32; r += kTrThreads / 64) {
        const int row = 32 * u + r;
        const bool in = row < g.rows;
        const float* src = cp.c + (in ? cond_row(row, g, cp) : 0);
        c[r * kLdC + lane] = in && lane < cp.C ? src[lane] : 0.f;
        if (lane < kCondMax - 64) c[r * kLdC + 64 + lane] = in && 64 + lane < cp.C ? src[64 + lane] : 0.f;
    }
}

// FG = a Wfg + c Gc + b into LDS fg [32][kLdW]: wave w owns columns 32 w .. 32 w + 31 (F: waves 0, 1; G: waves 2, 3).  The K loop of
// c Gc ends at C (even: the MFMA takes two values of k a step), so no row >= C of gc_filter / gc_gate is read.
__device__ __forceinline__ void compute_fg_cond(float* fg, const float* a, const float* c, const float* filter, const float* gate,
                                                const CondParams& cp) {
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
    f32x16 acc = zero16();
    gemm_xw<128>(acc, a, kLdW, (w < 2 ? filter : gate) + 32 * (w & 1), 64);
    const float* ca = c + j * kLdC + h;
    const float* gb = (w < 2 ? cp.gc_filter : cp.gc_gate) + 32 * (w & 1) + (size_t)h * 64 + j;
#pragma unroll 8
    for (int k = 0; k < cp.C; k += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ca[k], gb[(size_t)k * 64], acc, 0, 0, 0);
    const float* bias = w < 2 ? cp.filter_bias : cp.gate_bias;
    const float b = bias ? bias[32 * (w & 1) + j] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) fg[acc_row(r, h) * kLdW + 32 * w + j] = acc[r] + b;
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

// ------------------------------------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kTrThreads) void train_cond_layer_fwd_kernel(LayerFwdParams p, CondParams cp) {
    __shared__ float a[32 * kLdW];
    __shared__ float fg[32 * kLdW];
    __shared__ float o[32 * kLdH];
    __shared__ float c[32 * kLdC];
    __shared__ int s_fr[32];                    // (load_a leaves the P row of a row here: not read)
    UniformGeo::Loc loc;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
    const int units = (p.g.rows + 31) / 32;
    for (int u = blockIdx.x; u < units; u += gridDim.x) {
        load_a<UniformGeo>(a, s_fr, p.x, u, p.g, loc);
        load_c(c, u, p.g, cp);
        __syncthreads();
        compute_fg_cond(fg, a, c, p.filter, p.gate, cp);
        __syncthreads();
        for (int idx = threadIdx.x; idx < 2048; idx += kTrThreads) {
            const int r = idx >> 6, col = idx & 63;
            o[r * kLdH + col] = tanhf(fg[r * kLdW + col]) * sigmoid_f(fg[r * kLdW + 64 + col]);
        }
        __syncthreads();
        if (p.last) {
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
constexpr int kCondBlocks = kCondMax / 32;      // 32-row blocks of d_gc

// Eight accumulator tiles stay in registers over a workgroup's units (dWfg 4, d_gc 3, d dense 1); the second launch bound holds the
// kernel to the 256 registers per lane at which two workgroups share a compute unit, as the default grid of two per CU assumes
template <bool LAST>
__global__ __launch_bounds__(kTrThreads, 2) void train_cond_layer_bwd_kernel(LayerBwdParams p, CondParams cp) {
    __shared__ float a[32 * kLdW];              // [x[t - d] | x[t]], then [V | U]
    __shared__ float fg[32 * kLdW];             // FG, then dFG
    __shared__ float od[32 * kLdH];             // d o, then o: the gating pass replaces element by element (include/pwv_hip_train_cond.h, LDS)
    __shared__ float gin[32 * kLdH];            // g
    __shared__ float c[32 * kLdC];
    __shared__ int s_fr[32];
    UniformGeo::Loc loc;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
    const int units = (p.g.rows + 31) / 32;
    f32x16 g_wfg[4], g_gc[kCondBlocks], g_dense = zero16();
#pragma unroll
    for (int b = 0; b < 4; ++b) g_wfg[b] = zero16();
#pragma unroll
    for (int b = 0; b < kCondBlocks; ++b) g_gc[b] = zero16();
    float g_db = 0.f;                           // thread col < 64: d dense_bias[col]
    float g_b = 0.f;                            // thread 128 + col: d_b[col]
    for (int u = blockIdx.x; u < units; u += gridDim.x) {
        load_a<UniformGeo>(a, s_fr, p.x, u, p.g, loc);
        load_c(c, u, p.g, cp);
        if (LAST) tile32_to_lds(od, kLdH, 0, p.d_o, u, p.g.rows);
        else load_g<UniformGeo>(gin, kLdH, p.u_next, p.v_next, u, 32, p.g, loc);
        __syncthreads();
        compute_fg_cond(fg, a, c, p.filter, p.gate, cp);
        if (!LAST && w < 2) {                   // d o = g dense^T, columns 32 w ..
            f32x16 acc = zero16();
            gemm_xwt<64>(acc, gin, kLdH, p.dense + (size_t)32 * w * 64, 64);
            acc_to_lds(acc, od, kLdH, 32 * w);
        }
        __syncthreads();
        for (int idx = threadIdx.x; idx < 2048; idx += kTrThreads) {
            const int r = idx >> 6, col = idx & 63;
            const float th = tanhf(fg[r * kLdW + col]), sg = sigmoid_f(fg[r * kLdW + 64 + col]), d = od[r * kLdH + col];
            od[r * kLdH + col] = th * sg;
            fg[r * kLdW + col] = d * sg * (1.f - th * th);
            fg[r * kLdW + 64 + col] = d * th * sg * (1.f - sg);
        }
        __syncthreads();
        for (int b = 0; b < 4; ++b) gemm_tn(g_wfg[b], a, kLdW, 32 * b, fg, kLdW, 32 * w);         // dWfg += a^T dFG
#pragma unroll
        for (int b = 0; b < kCondBlocks; ++b) gemm_tn(g_gc[b], c, kLdC, 32 * b, fg, kLdW, 32 * w);      // d_gc += c^T dFG
        if (!LAST) {
            gemm_tn(g_dense, od, kLdH, 32 * (w >> 1), gin, kLdH, 32 * (w & 1));                   // d dense += o^T g
            if (threadIdx.x < 64)
                for (int r = 0; r < 32; ++r) g_db += gin[r * kLdH + threadIdx.x];
        }
        if (threadIdx.x >= 128) {               // d_b: column col of dFG over the rows, in row order (rows beyond the batch hold zeros)
            const int col = threadIdx.x - 128;
            for (int r = 0; r < 32; ++r) g_b += fg[r * kLdW + col];
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
        // [V | U] = dFG Wfg^T: wave w owns input channels 32 w .. of the 128 (0..63: the tap at t - d, 64..127: the tap at t)
        f32x16 acc = zero16();
        gemm_xwt<64>(acc, fg, kLdW, p.filter + (size_t)32 * w * 64, 64);
        gemm_xwt<64>(acc, fg + 64, kLdW, p.gate + (size_t)32 * w * 64, 64);
        __syncthreads();                        // every wave has read a
        acc_to_lds(acc, a, kLdW, 32 * w);
        __syncthreads();
        if (!LAST) {
            for (int idx = threadIdx.x; idx < 2048; idx += kTrThreads) {
                const int r = idx >> 6, col = idx & 63;
                a[r * kLdW + 64 + col] += gin[r * kLdH + col];
            }
            __syncthreads();
        }
        lds_to_tile32(p.v, u, a, kLdW, 0);
        lds_to_tile32(p.u, u, a, kLdW, 64);
        __syncthreads();
    }
    // the partial: dWfg | d dense | d dense_bias | d_gc [C][128] | d_b [128]
    float* part = p.part + (size_t)blockIdx.x * (kLayerPart + cp.C * 128 + 128);
    for (int b = 0; b < 4; ++b) acc_to_part(g_wfg[b], part, 128, 32 * b, 32 * w);
    if (!LAST) {
        acc_to_part(g_dense, part + 128 * 128, 64, 32 * (w >> 1), 32 * (w & 1));
        if (threadIdx.x < 64) part[128 * 128 + 64 * 64 + threadIdx.x] = g_db;
    }
    float* gc = part + kLayerPart;
#pragma unroll
    for (int b = 0; b < kCondBlocks; ++b) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int k = 32 * b + acc_row(r, h);
            if (k < cp.C) gc[(size_t)k * 128 + 32 * w + j] = g_gc[b][r];
        }
    }
    if (threadIdx.x >= 128) gc[(size_t)cp.C * 128 + threadIdx.x - 128] = g_b;
}

static int cond_part(int C) { return kLayerPart + C * 128 + 128; }

// what both entry points and the workspace size check; fills the geometry and the condition's parameters
static int cond_check(const pwv_train_cond_args* c, const char* who, bool sizes_only, Geom& g, CondParams& cp) {
    PWV_CHECK_ARG(c, "%s: args is NULL", who);
    const pwv_train_args* a = &c->train;
    PWV_CHECK_ARG(a->struct_size == sizeof(pwv_train_cond_args), "%s: train.struct_size %zu is not sizeof(pwv_train_cond_args) = %zu", who,
                  a->struct_size, sizeof(pwv_train_cond_args));
    PWV_CHECK_ARG(a->N >= 1 && a->T >= 1, "%s: N = %d, T = %d must be >= 1", who, a->N, a->T);
    PWV_CHECK_ARG((long long)a->N * a->T < (1ll << 31) - 64, "%s: N T = %lld is beyond int32", who, (long long)a->N * a->T);
    PWV_CHECK_ARG(a->max_workgroups >= 0, "%s: max_workgroups %d is negative", who, a->max_workgroups);
    PWV_CHECK_ARG(c->cond_channels >= 2 && c->cond_channels <= kCondMax && c->cond_channels % 2 == 0,
                  "%s: cond_channels %d must be even and in 2 .. %d", who, c->cond_channels, kCondMax);
    if (sizes_only) return PWV_OK;
    PWV_CHECK_ARG(a->dilation >= 1, "%s: dilation %d must be >= 1", who, a->dilation);
    PWV_CHECK_ARG(a->form == PWV_TRAIN_RESIDUAL || a->form == PWV_TRAIN_LAST, "%s: form %d", who, a->form);
    PWV_CHECK_ARG(c->cond, "%s: cond is a NULL pointer", who);
    PWV_CHECK_ARG(c->cond_row_stride >= c->cond_channels, "%s: cond_row_stride %d is below cond_channels %d", who, c->cond_row_stride,
                  c->cond_channels);
    PWV_CHECK_ARG(c->cond_utt_rows >= a->T, "%s: cond_utt_rows %d is below T = %d", who, c->cond_utt_rows, a->T);
    PWV_CHECK_ARG((long long)a->N * c->cond_utt_rows < (1ll << 31), "%s: N cond_utt_rows = %lld is beyond int32", who,
                  (long long)a->N * c->cond_utt_rows);
    PWV_CHECK_ARG(!a->proj && !a->d_proj, "%s: proj and d_proj must be NULL (the condition is per sample: there is no frame-rate projection)", who);
    PWV_CHECK_ARG(a->x && a->filter && a->gate && c->gc_filter && c->gc_gate, "%s: x, filter, gate, gc_filter or gc_gate is a NULL pointer", who);
    g.rows = a->N * a->T;
    g.T = a->T;
    g.d = a->dilation;
    g.dnext = a->next_dilation;
    g.hop = 1;                                  // (the P row load_a works out is not read)
    g.off = 0;
    g.frames = a->T;
    g.pstride = g.dpstride = g.kmax = 0;
    cp.c = c->cond; cp.gc_filter = c->gc_filter; cp.gc_gate = c->gc_gate; cp.filter_bias = c->filter_bias; cp.gate_bias = c->gate_bias;
    cp.d_c = c->d_cond;
    cp.C = c->cond_channels; cp.stride = c->cond_row_stride; cp.utt_rows = c->cond_utt_rows; cp.accumulate = c->d_cond_accumulate != 0;
    return PWV_OK;
}

}  // namespace pwv

using namespace pwv;

extern "C" size_t pwv_train_cond_workspace_bytes(const pwv_train_cond_args* c) {
    Geom g;
    CondParams cp;
    if (cond_check(c, "pwv_train_cond_workspace_bytes", true, g, cp) != PWV_OK) return 0;
    const int units = (c->train.N * c->train.T + 31) / 32, part = cond_part(c->cond_channels);
    return (size_t)train_grid_size(c->train.max_workgroups, units) * (part > kMaxPart ? part : kMaxPart) * sizeof(float);
}

extern "C" int pwv_train_cond_layer_fwd_f32(const pwv_train_cond_args* c, pwv_stream_t stream) {
    const char* who = "pwv_train_cond_layer_fwd_f32";
    LayerFwdParams p{};
    CondParams cp{};
    if (int e = cond_check(c, who, false, p.g, cp)) return e;
    const pwv_train_args* a = &c->train;
    PWV_CHECK_ARG(a->x_out, "%s: x_out is a NULL pointer", who);
    PWV_CHECK_ARG(a->form == PWV_TRAIN_LAST || a->dense, "%s: dense is a NULL pointer", who);
    p.x = a->x; p.filter = a->filter; p.gate = a->gate; p.dense = a->dense; p.dense_bias = a->dense_bias;
    p.x_out = a->x_out;
    p.last = a->form == PWV_TRAIN_LAST;
    hipLaunchKernelGGL(train_cond_layer_fwd_kernel, dim3(train_grid_size(a->max_workgroups, (p.g.rows + 31) / 32)), dim3(kTrThreads), 0,
                       (hipStream_t)stream, p, cp);
    PWV_CHECK_HIP(hipGetLastError());
    return PWV_OK;
}

extern "C" int pwv_train_cond_layer_bwd_f32(const pwv_train_cond_args* c, pwv_stream_t stream) {
    const char* who = "pwv_train_cond_layer_bwd_f32";
    LayerBwdParams p{};
    CondParams cp{};
    if (int e = cond_check(c, who, false, p.g, cp)) return e;
    const pwv_train_args* a = &c->train;
    const bool last = a->form == PWV_TRAIN_LAST;
    PWV_CHECK_ARG(a->u && a->v && a->d_filter && a->d_gate, "%s: u, v, d_filter or d_gate is a NULL pointer", who);
    PWV_CHECK_ARG(c->d_cond && c->d_gc_filter && c->d_gc_gate, "%s: d_cond, d_gc_filter or d_gc_gate is a NULL pointer", who);
    if (last) {
        PWV_CHECK_ARG(a->d_o, "%s: d_o is a NULL pointer", who);
    } else {
        PWV_CHECK_ARG(a->dense && a->u_next && a->v_next && a->d_dense, "%s: dense, u_next, v_next or d_dense is a NULL pointer", who);
        PWV_CHECK_ARG(a->next_dilation >= 1, "%s: next_dilation %d must be >= 1", who, a->next_dilation);
        PWV_CHECK_ARG(a->u != a->u_next && a->v != a->v_next && a->u != a->v_next && a->v != a->u_next, "%s: u / v alias u_next / v_next", who);
    }
    const int grid = train_grid_size(a->max_workgroups, (p.g.rows + 31) / 32), part = cond_part(cp.C);
    PWV_CHECK_ARG(a->workspace, "%s: workspace is a NULL pointer", who);
    PWV_CHECK_ARG(a->workspace_bytes >= (size_t)grid * part * sizeof(float), "%s: workspace_bytes %zu is short of %zu", who, a->workspace_bytes,
                  (size_t)grid * part * sizeof(float));
    p.x = a->x; p.filter = a->filter; p.gate = a->gate; p.dense = a->dense;
    p.u_next = a->u_next; p.v_next = a->v_next; p.d_o = a->d_o;
    p.u = a->u; p.v = a->v; p.part = (float*)a->workspace;
    if (last) hipLaunchKernelGGL(train_cond_layer_bwd_kernel<true>, dim3(grid), dim3(kTrThreads), 0, (hipStream_t)stream, p, cp);
    else hipLaunchKernelGGL(train_cond_layer_bwd_kernel<false>, dim3(grid), dim3(kTrThreads), 0, (hipStream_t)stream, p, cp);
    PWV_CHECK_HIP(hipGetLastError());
    // stage two (train_reduce_kernel, csrc/pwv_train.hip): the segments of the partial to their TF layouts; a [k][128] segment with two
    // destinations splits its rows into [k][64] | [k][64]
    ReduceParams rp;
    rp.part = p.part; rp.n_part = grid; rp.stride = part; rp.total = part; rp.n_seg = 6;
    const int at_dense = 128 * 128, at_db = at_dense + 64 * 64, at_gc = kLayerPart, at_b = at_gc + cp.C * 128;
    const int begin[7] = {0, at_dense, at_db, at_gc, at_b, at_b + 64, part};
    float* dst[6] = {a->d_filter, last ? nullptr : a->d_dense, last ? nullptr : a->d_dense_bias, c->d_gc_filter, c->d_filter_bias, c->d_gate_bias};
    float* dst2[6] = {a->d_gate, nullptr, nullptr, c->d_gc_gate, nullptr, nullptr};
    for (int s = 0; s < 6; ++s) {
        rp.seg[s].begin = begin[s]; rp.seg[s].end = begin[s + 1]; rp.seg[s].dst = dst[s]; rp.seg[s].dst2 = dst2[s];
    }
    return train_reduce(rp, (hipStream_t)stream);
}
