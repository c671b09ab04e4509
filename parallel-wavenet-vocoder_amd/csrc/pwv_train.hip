// Training (include/pwv_hip_train.h; DESIGN.md section 9, "Training"): the forward with saved activations and the backward pass of the
// default architecture, one net per launch, exact-fp32 MFMA (v_mfma_f32_32x32x2_f32).
// Every kernel works on UNITS of 32 rows (one tile32 block) with 256 threads = 4 waves.  The operands of a unit's GEMMs are staged in LDS
// as plain row-major [32][odd stride] arrays; a wave computes one 32 x 32 tile per GEMM call:
//   activations x weights    A[i = row][k] from LDS, B[k][j] from the TF-layout weight in global memory (strides pick W or W^T)
//   weight gradients         A[i][k = row] and B[k = row][j] both from LDS: the 32 rows of the unit are the K dimension, the tile stays in
//                            the wave's accumulators over all units of the workgroup and leaves once, as the workgroup's partial.
// A second launch (train_reduce_kernel) adds the partials in a fixed order and scatters them to the TF layouts.  No atomics.
// The unit bodies that depend on where an utterance begins and ends live in pwv_train_units.h, written over a geometry and a
// conditioning policy, with the host text of their entry points; the kernels here are their uniform [N, T] instances on the
// frame-rate projection (csrc/pwv_train_varlen.hip holds the packed ones, csrc/pwv_train_cond.hip those of a per-sample condition),
// next to the one-output instance of the head (csrc/pwv_train_head.h), which is row-independent, and the reduction.
#include "pwv_common.h"
#include "pwv_hip_train.h"
#include "pwv_train_head.h"

namespace pwv {

// ------------------------------------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kTrThreads) void train_front_fwd_kernel(FrontFwdParams p) { front_fwd_body<UniformGeo>(p); }

__global__ __launch_bounds__(kTrThreads) void train_layer_fwd_kernel(LayerFwdParams p) { layer_fwd_body<UniformGeo, ProjCond>(p, {}); }

__global__ __launch_bounds__(kTrThreads) void train_head_fwd_kernel(HeadParams p) { head_fwd_body<GatedIn, 1>(p); }

// ------------------------------------------------------------------------------------------------------------------------------
// backward
// ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kTrThreads) void train_head_bwd_kernel(HeadParams p) { head_bwd_body<GatedIn, 1>(p); }

template <bool LAST>
__global__ __launch_bounds__(kTrThreads) void train_layer_bwd_kernel(LayerBwdParams p) {
    layer_bwd_body<UniformGeo, ProjCond, LAST>(p, {});
}

__global__ __launch_bounds__(kTrThreads) void train_front_bwd_kernel(FrontBwdParams p) { front_bwd_body<UniformGeo>(p); }

// stage two: element e of the result = the sum over the partials in a fixed order, scattered to the TF layouts (ReduceParams:
// pwv_train_units.h).
// A workgroup owns 32 consecutive elements; its 8 groups of 32 lanes each add a contiguous eighth of the partials in index order (eight
// loads in flight at a time), and lane group 0 adds the eight sums in order: an order that depends on the indices alone.
constexpr int kReduceElems = 32, kReduceGroups = kTrThreads / kReduceElems;

__global__ __launch_bounds__(kTrThreads) void train_reduce_kernel(ReduceParams p) {
    __shared__ float s_sum[kReduceGroups][kReduceElems];
    const int el = threadIdx.x & (kReduceElems - 1), grp = threadIdx.x / kReduceElems;
    const int e = blockIdx.x * kReduceElems + el;
    const int chunk = (p.n_part + kReduceGroups - 1) / kReduceGroups;
    const int lo = grp * chunk, hi = min(lo + chunk, p.n_part);
    float sum = 0.f;
    if (e < p.total) {
        const float* src = p.part + e;
        int i = lo;
        for (; i + 8 <= hi; i += 8) {
            float v[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = src[(size_t)(i + q) * p.stride];
#pragma unroll
            for (int q = 0; q < 8; ++q) sum += v[q];
        }
        for (; i < hi; ++i) sum += src[(size_t)i * p.stride];
    }
    s_sum[grp][el] = sum;
    __syncthreads();
    if (grp != 0 || e >= p.total) return;
    sum = s_sum[0][el];
#pragma unroll
    for (int q = 1; q < kReduceGroups; ++q) sum += s_sum[q][el];
    int s = 0;
    while (s + 1 < p.n_seg && e >= p.seg[s].end) ++s;
    if (e < p.seg[s].begin || e >= p.seg[s].end || !p.seg[s].dst) return;
    const int l = e - p.seg[s].begin;
    if (p.seg[s].dst2) {
        const int k = l >> 7, c = l & 127;
        (c < 64 ? p.seg[s].dst : p.seg[s].dst2)[k * 64 + (c & 63)] = sum;
    } else {
        p.seg[s].dst[l] = sum;
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------------------------------------
int train_grid_size(int max_workgroups, int units) {
    // two per compute unit by default: at most 62 KB of LDS (the per-sample layer backward) and <= 256 registers let two share a CU,
    // and one hides the other's operand loads
    int cap = max_workgroups > 0 ? max_workgroups : 2 * device_cus();
    if (cap < 1) cap = 1;
    return units < cap ? units : cap;
}

static int train_grid(const pwv_train_args* a, int units) { return train_grid_size(a->max_workgroups, units); }

int train_check_batch(const pwv_train_args* a, const char* who, const char* field, size_t size, const char* name) {
    PWV_CHECK_ARG(a, "%s: args is NULL", who);
    PWV_CHECK_ARG(a->struct_size == size, "%s: %s %zu is not sizeof(%s) = %zu", who, field, a->struct_size, name, size);
    PWV_CHECK_ARG(a->N >= 1 && a->T >= 1, "%s: N = %d, T = %d must be >= 1", who, a->N, a->T);
    PWV_CHECK_ARG((long long)a->N * a->T < (1ll << 31) - 64, "%s: N T = %lld is beyond int32", who, (long long)a->N * a->T);
    PWV_CHECK_ARG(a->max_workgroups >= 0, "%s: max_workgroups %d is negative", who, a->max_workgroups);
    return PWV_OK;
}

static int train_check(const pwv_train_args* a, const char* who) {
    return train_check_batch(a, who, "struct_size", sizeof(pwv_train_args), "pwv_train_args");
}

static int train_geom(const pwv_train_args* a, const char* who, Geom& g, bool layer) {
    g.rows = a->N * a->T;
    g.T = a->T;
    g.d = a->dilation;
    g.dnext = a->next_dilation;
    g.hop = a->cond_hop;
    g.off = a->cond_offset;
    g.frames = a->cond_frames;
    g.pstride = a->proj_row_stride;
    g.dpstride = a->d_proj_row_stride;
    g.kmax = layer ? (a->cond_hop + 30) / 32 + 1 : 0;
    if (layer) {
        PWV_CHECK_ARG(a->dilation >= 1, "%s: dilation %d must be >= 1", who, a->dilation);
        PWV_CHECK_ARG(a->cond_hop >= 1 && a->cond_offset >= 0 && a->cond_frames >= 1, "%s: cond_hop %d, cond_offset %d, cond_frames %d", who,
                      a->cond_hop, a->cond_offset, a->cond_frames);
        PWV_CHECK_ARG((a->T - 1 + a->cond_offset) / a->cond_hop < a->cond_frames, "%s: cond_frames %d is short of the frames T = %d needs", who,
                      a->cond_frames, a->T);
        PWV_CHECK_ARG(a->proj_row_stride >= 128, "%s: proj_row_stride %d is below 128", who, a->proj_row_stride);
    }
    return PWV_OK;
}

int train_reduce(const ReduceParams& rp, hipStream_t st) {
    hipLaunchKernelGGL(train_reduce_kernel, dim3((rp.total + kReduceElems - 1) / kReduceElems), dim3(kTrThreads), 0, st, rp);
    PWV_CHECK_HIP(hipGetLastError());
    return PWV_OK;
}

}  // namespace pwv

using namespace pwv;

extern "C" size_t pwv_train_workspace_bytes(const pwv_train_args* a) {
    if (train_check(a, "pwv_train_workspace_bytes") != PWV_OK) return 0;
    const int units = (a->N * a->T + 31) / 32;
    return (size_t)train_grid(a, units) * kMaxPart * sizeof(float);
}

extern "C" int pwv_train_front_fwd_f32(const pwv_train_args* a, pwv_stream_t stream) {
    const char* who = "pwv_train_front_fwd_f32";
    if (int e = train_check(a, who)) return e;
    Geom g;
    if (int e = train_geom(a, who, g, false)) return e;
    return train_front_fwd(a, who, g, PackedTables{}, [&](int grid, const FrontFwdParams& p) {
        hipLaunchKernelGGL(train_front_fwd_kernel, dim3(grid), dim3(kTrThreads), 0, (hipStream_t)stream, p);
    });
}

extern "C" int pwv_train_layer_fwd_f32(const pwv_train_args* a, pwv_stream_t stream) {
    const char* who = "pwv_train_layer_fwd_f32";
    if (int e = train_check(a, who)) return e;
    Geom g;
    if (int e = train_geom(a, who, g, true)) return e;
    return train_layer_fwd<ProjCond>(a, who, g, PackedTables{}, [&](int grid, const LayerFwdParams& p) {
        hipLaunchKernelGGL(train_layer_fwd_kernel, dim3(grid), dim3(kTrThreads), 0, (hipStream_t)stream, p);
    });
}

static int head_check(const pwv_train_args* a, const char* who) {
    if (int e = train_check(a, who)) return e;
    PWV_CHECK_ARG(a->x && a->skip && a->post1 && a->post2, "%s: x, skip, post1 or post2 is a NULL pointer", who);
    return PWV_OK;
}

extern "C" int pwv_train_head_fwd_f32(const pwv_train_args* a, pwv_stream_t stream) {
    const char* who = "pwv_train_head_fwd_f32";
    if (int e = head_check(a, who)) return e;
    PWV_CHECK_ARG(a->y, "%s: y is a NULL pointer", who);
    const HeadParams p = head_params(a, a->N * a->T);
    return head_fwd_launch(train_head_fwd_kernel, p, train_grid(a, (p.rows + 31) / 32), (hipStream_t)stream);
}

extern "C" int pwv_train_head_bwd_f32(const pwv_train_args* a, pwv_stream_t stream) {
    const char* who = "pwv_train_head_bwd_f32";
    if (int e = head_check(a, who)) return e;
    PWV_CHECK_ARG(a->d_out && a->d_o_out, "%s: d_out or d_o_out is a NULL pointer", who);
    const HeadParams p = head_params(a, a->N * a->T);
    const int grid = train_grid(a, (p.rows + 31) / 32);
    if (int e = train_check_ws(a, who, grid, head_part<GatedIn, 1>())) return e;
    return head_bwd_launch_and_reduce<GatedIn, 1>(train_head_bwd_kernel, p, grid, a, a->d_skip_bias, (hipStream_t)stream);
}

extern "C" int pwv_train_layer_bwd_f32(const pwv_train_args* a, pwv_stream_t stream) {
    const char* who = "pwv_train_layer_bwd_f32";
    if (int e = train_check(a, who)) return e;
    Geom g;
    if (int e = train_geom(a, who, g, true)) return e;
    return train_layer_bwd<ProjCond>(a, who, g, PackedTables{}, {}, nullptr, 0, (hipStream_t)stream, [&](bool last, int grid, const LayerBwdParams& p) {
        if (last) hipLaunchKernelGGL(train_layer_bwd_kernel<true>, dim3(grid), dim3(kTrThreads), 0, (hipStream_t)stream, p);
        else hipLaunchKernelGGL(train_layer_bwd_kernel<false>, dim3(grid), dim3(kTrThreads), 0, (hipStream_t)stream, p);
    });
}

extern "C" int pwv_train_front_bwd_f32(const pwv_train_args* a, pwv_stream_t stream) {
    const char* who = "pwv_train_front_bwd_f32";
    if (int e = train_check(a, who)) return e;
    Geom g;
    if (int e = train_geom(a, who, g, false)) return e;
    return train_front_bwd(a, who, g, PackedTables{}, (hipStream_t)stream, [&](int grid, const FrontBwdParams& p) {
        hipLaunchKernelGGL(train_front_bwd_kernel, dim3(grid), dim3(kTrThreads), 0, (hipStream_t)stream, p);
    });
}
