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
// next to the head, which is row-independent, and the reduction.
#include "pwv_common.h"
#include "pwv_hip_train.h"
#include "pwv_train_units.h"

namespace pwv {

// ------------------------------------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kTrThreads) void train_front_fwd_kernel(FrontFwdParams p) { front_fwd_body<UniformGeo>(p); }

__global__ __launch_bounds__(kTrThreads) void train_layer_fwd_kernel(LayerFwdParams p) { layer_fwd_body<UniformGeo, ProjCond>(p, {}); }

struct HeadParams {
    const float *o, *skip, *skip_bias, *post1, *post1_bias, *post2, *post2_bias;
    float* y;                                   // forward
    const float *d_out, *d_mul;                 // backward
    float* d_o;
    float* part;
    int rows;
};

// h1 = relu(o skip + sb), h2 = relu(h1 post1 + b1) of one unit; o is in LDS
__device__ __forceinline__ void head_hidden(float* h1, float* h2, const float* o, const HeadParams& p) {
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
    {
        f32x16 acc = zero16();
        gemm_xw<64>(acc, o, kLdH, p.skip + 32 * w, 128);
        const float b = p.skip_bias ? p.skip_bias[32 * w + j] : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) h1[acc_row(r, h) * kLdW + 32 * w + j] = fmaxf(acc[r] + b, 0.f);
    }
    __syncthreads();
    {
        f32x16 acc = zero16();
        gemm_xw<128>(acc, h1, kLdW, p.post1 + 32 * w, 128);
        const float b = p.post1_bias ? p.post1_bias[32 * w + j] : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) h2[acc_row(r, h) * kLdW + 32 * w + j] = fmaxf(acc[r] + b, 0.f);
    }
    __syncthreads();
}

__global__ __launch_bounds__(kTrThreads) void train_head_fwd_kernel(HeadParams p) {
    __shared__ float o[32 * kLdH];
    __shared__ float h1[32 * kLdW];
    __shared__ float h2[32 * kLdW];
    const int units = (p.rows + 31) / 32;
    for (int u = blockIdx.x; u < units; u += gridDim.x) {
        tile32_to_lds(o, kLdH, 0, p.o, u, p.rows);
        __syncthreads();
        head_hidden(h1, h2, o, p);
        // y[r] = h2[r] . post2 + b2: 8 lanes per row, 16 columns each, then a fixed tree over the 8
        const int r = threadIdx.x >> 3, part = threadIdx.x & 7;
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < 16; ++e) s += h2[r * kLdW + 16 * part + e] * p.post2[16 * part + e];
        s += __shfl_xor(s, 1);
        s += __shfl_xor(s, 2);
        s += __shfl_xor(s, 4);
        if (part == 0 && 32 * u + r < p.rows) p.y[32 * u + r] = s + (p.post2_bias ? p.post2_bias[0] : 0.f);
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// backward
// ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kTrThreads) void train_head_bwd_kernel(HeadParams p) {
    __shared__ float o[32 * kLdH];
    __shared__ float h1[32 * kLdW];             // h1, then dz1
    __shared__ float h2[32 * kLdW];             // h2, then dz2
    __shared__ float dy[32];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
    const int units = (p.rows + 31) / 32;
    f32x16 g_post1[4], g_skip[2];
#pragma unroll
    for (int b = 0; b < 4; ++b) g_post1[b] = zero16();
    g_skip[0] = zero16();
    g_skip[1] = zero16();
    float g_p2 = 0.f, g_b1 = 0.f, g_sb = 0.f, g_b2 = 0.f;      // thread c < 128: column c; g_b2: thread 128
    for (int u = blockIdx.x; u < units; u += gridDim.x) {
        tile32_to_lds(o, kLdH, 0, p.o, u, p.rows);
        if (threadIdx.x < 32) {
            const int row = 32 * u + threadIdx.x;
            dy[threadIdx.x] = row < p.rows ? p.d_out[row] * (p.d_mul ? p.d_mul[row] : 1.f) : 0.f;
        }
        __syncthreads();
        head_hidden(h1, h2, o, p);
        if (threadIdx.x < 128) {                // d post2, dz2 = dy post2^T where h2 > 0, d b1
            const int c = threadIdx.x;
            const float w2 = p.post2[c];
            for (int r = 0; r < 32; ++r) {
                const float v = h2[r * kLdW + c], z = v > 0.f ? dy[r] * w2 : 0.f;
                g_p2 += v * dy[r];
                g_b1 += z;
                h2[r * kLdW + c] = z;
            }
        } else if (threadIdx.x == 128) {
            for (int r = 0; r < 32; ++r) g_b2 += dy[r];
        }
        __syncthreads();
        for (int b = 0; b < 4; ++b) gemm_tn(g_post1[b], h1, kLdW, 32 * b, h2, kLdW, 32 * w);      // d post1 += h1^T dz2
        f32x16 acc = zero16();                  // dh1 = dz2 post1^T, columns 32 w ..
        gemm_xwt<128>(acc, h2, kLdW, p.post1 + (size_t)32 * w * 128, 128);
        __syncthreads();                        // every wave has read h1 as an operand
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float* e = h1 + acc_row(r, h) * kLdW + 32 * w + j;
            *e = *e > 0.f ? acc[r] : 0.f;       // dz1
        }
        __syncthreads();
        if (threadIdx.x < 128) {
            const int c = threadIdx.x;
            for (int r = 0; r < 32; ++r) g_sb += h1[r * kLdW + c];
        }
        for (int b = 0; b < 2; ++b) gemm_tn(g_skip[b], o, kLdH, 32 * b, h1, kLdW, 32 * w);        // d skip += o^T dz1
        f32x16 d_o_acc = zero16();
        if (w < 2) gemm_xwt<128>(d_o_acc, h1, kLdW, p.skip + (size_t)32 * w * 128, 128);             // d o = dz1 skip^T, columns 32 w ..
        __syncthreads();                        // every wave has read o
        if (w < 2) acc_to_lds(d_o_acc, o, kLdH, 32 * w);
        __syncthreads();
        lds_to_tile32(p.d_o, u, o, kLdH, 0);
        __syncthreads();
    }
    float* part = p.part + (size_t)blockIdx.x * kHeadPart;
    for (int b = 0; b < 2; ++b) acc_to_part(g_skip[b], part, 128, 32 * b, 32 * w);
    for (int b = 0; b < 4; ++b) acc_to_part(g_post1[b], part + 64 * 128 + 128, 128, 32 * b, 32 * w);
    if (threadIdx.x < 128) {
        part[64 * 128 + threadIdx.x] = g_sb;
        part[64 * 128 + 128 + 128 * 128 + threadIdx.x] = g_b1;
        part[64 * 128 + 128 + 128 * 128 + 128 + threadIdx.x] = g_p2;
    } else if (threadIdx.x == 128) {
        part[kHeadPart - 1] = g_b2;
    }
}

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

static int head_params(const pwv_train_args* a, const char* who, HeadParams& p) {
    PWV_CHECK_ARG(a->x && a->skip && a->post1 && a->post2, "%s: x, skip, post1 or post2 is a NULL pointer", who);
    p.o = a->x; p.skip = a->skip; p.skip_bias = a->skip_bias; p.post1 = a->post1; p.post1_bias = a->post1_bias;
    p.post2 = a->post2; p.post2_bias = a->post2_bias;
    p.y = a->y; p.d_out = a->d_out; p.d_mul = a->d_mul; p.d_o = a->d_o_out; p.part = (float*)a->workspace;
    p.rows = a->N * a->T;
    return PWV_OK;
}

extern "C" int pwv_train_head_fwd_f32(const pwv_train_args* a, pwv_stream_t stream) {
    const char* who = "pwv_train_head_fwd_f32";
    if (int e = train_check(a, who)) return e;
    HeadParams p;
    if (int e = head_params(a, who, p)) return e;
    PWV_CHECK_ARG(a->y, "%s: y is a NULL pointer", who);
    hipLaunchKernelGGL(train_head_fwd_kernel, dim3(train_grid(a, (p.rows + 31) / 32)), dim3(kTrThreads), 0, (hipStream_t)stream, p);
    PWV_CHECK_HIP(hipGetLastError());
    return PWV_OK;
}

extern "C" int pwv_train_head_bwd_f32(const pwv_train_args* a, pwv_stream_t stream) {
    const char* who = "pwv_train_head_bwd_f32";
    if (int e = train_check(a, who)) return e;
    HeadParams p;
    if (int e = head_params(a, who, p)) return e;
    PWV_CHECK_ARG(a->d_out && a->d_o_out, "%s: d_out or d_o_out is a NULL pointer", who);
    const int grid = train_grid(a, (p.rows + 31) / 32);
    if (int e = train_check_ws(a, who, grid, kHeadPart)) return e;
    hipLaunchKernelGGL(train_head_bwd_kernel, dim3(grid), dim3(kTrThreads), 0, (hipStream_t)stream, p);
    PWV_CHECK_HIP(hipGetLastError());
    ReduceParams rp;
    rp.part = p.part; rp.n_part = grid; rp.stride = kHeadPart; rp.total = kHeadPart; rp.n_seg = 6;
    int at = 0;
    const int len[6] = {64 * 128, 128, 128 * 128, 128, 128, 1};
    float* dst[6] = {a->d_skip, a->d_skip_bias, a->d_post1, a->d_post1_bias, a->d_post2, a->d_post2_bias};
    for (int s = 0; s < 6; ++s) {
        rp.seg[s].begin = at; rp.seg[s].end = at + len[s]; rp.seg[s].dst = dst[s]; rp.seg[s].dst2 = nullptr;
        at += len[s];
    }
    return train_reduce(rp, (hipStream_t)stream);
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
