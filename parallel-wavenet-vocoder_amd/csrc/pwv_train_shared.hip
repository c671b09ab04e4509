// Training the shared-net architecture (include/pwv_hip_train_shared.h; DESIGN.md section 9, "Training the shared-net architecture"):
// one net per flow with two output channels, y_0 the scale and y_1 the shift.  Only the head knows the output width, so this file is
// the Q = 2 head, forward and backward, written ONCE over an INPUT POLICY: GatedIn begins at the last layer's o and forms
// relu(o skip + skip_bias) itself (the head of csrc/pwv_train.hip), SumIn begins at the skip sum S (the head of
// csrc/pwv_train_skip.hip).  Behind h1 the two are one text: h2, the two dots with post2's columns, dz2 from both dy planes, d post1,
// dh1; the policy then takes dz1 back to (d skip, d skip_bias, d o) or leaves it as dS with its column sums.  The plan is the other
// training kernels': 256 threads per 32-row unit, workgroup b takes units u = b (mod grid), operands in LDS at the odd strides kLdH /
// kLdW, weights in their TensorFlow layouts, weight gradients in accumulators over all units of the workgroup, ONE partial per
// workgroup, train_reduce_kernel's fixed order behind it.  No floating-point atomics.
#include "pwv_common.h"
#include "pwv_hip_train_shared.h"
#include "pwv_train_units.h"

namespace pwv {

struct SharedHeadParams {
    const float *o, *s, *skip, *skip_bias, *post1, *post1_bias, *post2, *post2_bias;
    float *y0, *y1;                             // forward: the scale and the shift plane
    const float *d_out, *d_mul;                 // backward
    float *d_o, *d_s;
    float* part;
    int rows;
};

// ------------------------------------------------------------------------------------------------------------------------------
// input policies: what stands in front of h1 and what dz1 becomes
//   kFront   floats of a partial in front of d post1: GatedIn d skip [64][128] | d skip_bias [128]; SumIn the column sums of dS [128]
// ------------------------------------------------------------------------------------------------------------------------------
struct GatedIn {
    static constexpr bool kGated = true;
    static constexpr int kFront = 64 * 128 + 128;
    struct Tile {
        float o[32 * kLdH];
    };
};

struct SumIn {
    static constexpr bool kGated = false;
    static constexpr int kFront = 128;
    struct Tile {};
};

template <class In>
constexpr int shared_part() {                   // front | d post1 | d b1 | d post2 [128][2] as it lies in TF's layout | d b2 [2]
    return In::kFront + 128 * 128 + 128 + 256 + 2;
}
constexpr int kSharedMaxPart = shared_part<GatedIn>() > kMaxPart ? shared_part<GatedIn>() : kMaxPart;

// h1 and h2 = relu(h1 post1 + b1) of unit u; GatedIn leaves the unit's o in tl.o
template <class In>
__device__ __forceinline__ void shared_hidden(typename In::Tile& tl, float* h1, float* h2, int u, const SharedHeadParams& p) {
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
    if constexpr (In::kGated) {
        tile32_to_lds(tl.o, kLdH, 0, p.o, u, p.rows);
        __syncthreads();
        f32x16 acc = zero16();
        gemm_xw<64>(acc, tl.o, kLdH, p.skip + 32 * w, 128);
        const float b = p.skip_bias ? p.skip_bias[32 * w + j] : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) h1[acc_row(r, h) * kLdW + 32 * w + j] = fmaxf(acc[r] + b, 0.f);
    } else {
        tile32w_to_lds<true>(h1, kLdW, p.s, u, p.rows);
    }
    __syncthreads();
    f32x16 acc = zero16();
    gemm_xw<128>(acc, h1, kLdW, p.post1 + 32 * w, 128);
    const float b = p.post1_bias ? p.post1_bias[32 * w + j] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) h2[acc_row(r, h) * kLdW + 32 * w + j] = fmaxf(acc[r] + b, 0.f);
    __syncthreads();
}

template <class In>
__device__ __forceinline__ void shared_head_fwd_body(const SharedHeadParams& p) {
    __shared__ typename In::Tile tl;
    __shared__ float h1[32 * kLdW];
    __shared__ float h2[32 * kLdW];
    const int units = (p.rows + 31) / 32;
    for (int u = blockIdx.x; u < units; u += gridDim.x) {
        shared_hidden<In>(tl, h1, h2, u, p);
        // y_q[r] = h2[r] . post2[:, q] + b2[q]: 8 lanes per row, 16 columns each, then a fixed tree over the 8, for both columns
        const int r = threadIdx.x >> 3, part = threadIdx.x & 7;
        float s0 = 0.f, s1 = 0.f;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const float v = h2[r * kLdW + 16 * part + e];
            s0 += v * p.post2[2 * (16 * part + e)];
            s1 += v * p.post2[2 * (16 * part + e) + 1];
        }
        s0 += __shfl_xor(s0, 1);
        s1 += __shfl_xor(s1, 1);
        s0 += __shfl_xor(s0, 2);
        s1 += __shfl_xor(s1, 2);
        s0 += __shfl_xor(s0, 4);
        s1 += __shfl_xor(s1, 4);
        if (part == 0 && 32 * u + r < p.rows) {
            p.y0[32 * u + r] = s0 + (p.post2_bias ? p.post2_bias[0] : 0.f);
            p.y1[32 * u + r] = s1 + (p.post2_bias ? p.post2_bias[1] : 0.f);
        }
        __syncthreads();
    }
}

// 32 rows x 64 channels of an LDS array -> block u of a tile32 buffer, the rows of the batch alone
__device__ __forceinline__ void lds_to_tile32_rows(float* dst, int u, const float* src, int ld, int rows) {
    for (int idx = threadIdx.x; idx < 512; idx += kTrThreads) {
        const int q = idx >> 5, r = idx & 31;
        if (32 * u + r >= rows) continue;
        const float* s = src + r * ld + 4 * q;
        f32x4 v = {s[0], s[1], s[2], s[3]};
        *reinterpret_cast<f32x4*>(dst + (size_t)u * 2048 + q * 128 + r * 4) = v;
    }
}

template <class In>
__device__ __forceinline__ void shared_head_bwd_body(const SharedHeadParams& p) {
    __shared__ typename In::Tile tl;
    __shared__ float h1[32 * kLdW];             // h1, then dz1 (SumIn: = dS)
    __shared__ float h2[32 * kLdW];             // h2, then dz2
    __shared__ float dy[2][32];                 // dy_0 = d_out d_mul, dy_1 = d_out; zeros beyond the batch
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
    const int units = (p.rows + 31) / 32;
    f32x16 g_post1[4];
    f32x16 g_skip[In::kGated ? 2 : 1];
#pragma unroll
    for (int b = 0; b < 4; ++b) g_post1[b] = zero16();
    if constexpr (In::kGated) {
        g_skip[0] = zero16();
        g_skip[1] = zero16();
    }
    // thread c < 128: column c of d post2 (both q), d b1 and the policy's column sums; threads 128, 129: d b2[0], d b2[1]
    float g_p20 = 0.f, g_p21 = 0.f, g_b1 = 0.f, g_col = 0.f, g_b2 = 0.f;
    for (int u = blockIdx.x; u < units; u += gridDim.x) {
        if (threadIdx.x < 32) {
            const int row = 32 * u + threadIdx.x;
            const float d = row < p.rows ? p.d_out[row] : 0.f;
            dy[0][threadIdx.x] = row < p.rows ? d * (p.d_mul ? p.d_mul[row] : 1.f) : 0.f;
            dy[1][threadIdx.x] = d;
        }
        shared_hidden<In>(tl, h1, h2, u, p);    // (its barriers publish dy)
        if (threadIdx.x < 128) {                // d post2, dz2 = (dy_0 post2[:, 0] + dy_1 post2[:, 1]) where h2 > 0, d b1
            const int c = threadIdx.x;
            const float w20 = p.post2[2 * c], w21 = p.post2[2 * c + 1];
#pragma unroll 4                                // (unrolled whole, the 32 rows' loads in flight cost 78 more registers: beyond 256)
            for (int r = 0; r < 32; ++r) {
                const float v = h2[r * kLdW + c], z = v > 0.f ? dy[0][r] * w20 + dy[1][r] * w21 : 0.f;
                g_p20 += v * dy[0][r];
                g_p21 += v * dy[1][r];
                g_b1 += z;
                h2[r * kLdW + c] = z;
            }
        } else if (threadIdx.x < 130) {
            const int q = threadIdx.x - 128;
            for (int r = 0; r < 32; ++r) g_b2 += dy[q][r];
        }
        __syncthreads();
        for (int b = 0; b < 4; ++b) gemm_tn(g_post1[b], h1, kLdW, 32 * b, h2, kLdW, 32 * w);      // d post1 += h1^T dz2
        f32x16 acc = zero16();                  // dh1 = dz2 post1^T, columns 32 w ..
        gemm_xwt<128>(acc, h2, kLdW, p.post1 + (size_t)32 * w * 128, 128);
        __syncthreads();                        // every wave has read h1 as an operand
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float* e = h1 + acc_row(r, h) * kLdW + 32 * w + j;
            *e = *e > 0.f ? acc[r] : 0.f;       // dz1 = dh1 where h1 > 0 (SumIn: where S > 0)
        }
        __syncthreads();
        if (threadIdx.x < 128) {                // d skip_bias (SumIn: of every layer)
            const int c = threadIdx.x;
            for (int r = 0; r < 32; ++r) g_col += h1[r * kLdW + c];
        }
        if constexpr (In::kGated) {
            for (int b = 0; b < 2; ++b) gemm_tn(g_skip[b], tl.o, kLdH, 32 * b, h1, kLdW, 32 * w);    // d skip += o^T dz1
            f32x16 d_o_acc = zero16();
            if (w < 2) gemm_xwt<128>(d_o_acc, h1, kLdW, p.skip + (size_t)32 * w * 128, 128);         // d o = dz1 skip^T, columns 32 w ..
            __syncthreads();                    // every wave has read o
            if (w < 2) acc_to_lds(d_o_acc, tl.o, kLdH, 32 * w);
            __syncthreads();
            lds_to_tile32_rows(p.d_o, u, tl.o, kLdH, p.rows);
        } else {
            lds_to_tile32w(p.d_s, u, h1, kLdW, p.rows, 0);
        }
        __syncthreads();
    }
    float* part = p.part + (size_t)blockIdx.x * shared_part<In>();
    if constexpr (In::kGated) {
        for (int b = 0; b < 2; ++b) acc_to_part(g_skip[b], part, 128, 32 * b, 32 * w);
    }
    float* behind = part + In::kFront;
    for (int b = 0; b < 4; ++b) acc_to_part(g_post1[b], behind, 128, 32 * b, 32 * w);
    if (threadIdx.x < 128) {
        part[In::kFront - 128 + threadIdx.x] = g_col;
        behind[128 * 128 + threadIdx.x] = g_b1;
        behind[128 * 128 + 128 + 2 * threadIdx.x] = g_p20;            // (c, q) at 2 c + q: the reduction writes TF's layout as it lies
        behind[128 * 128 + 128 + 2 * threadIdx.x + 1] = g_p21;
    } else if (threadIdx.x < 130) {
        behind[128 * 128 + 128 + 256 + threadIdx.x - 128] = g_b2;
    }
}

template <class In>
__global__ __launch_bounds__(kTrThreads) void train_shared_head_fwd_kernel(SharedHeadParams p) {
    shared_head_fwd_body<In>(p);
}

// six accumulator tiles (GatedIn) stay in registers over a workgroup's units
template <class In>
__global__ __launch_bounds__(kTrThreads) void train_shared_head_bwd_kernel(SharedHeadParams p) {
    shared_head_bwd_body<In>(p);
}

// ------------------------------------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------------------------------------
static int shared_check(const pwv_train_shared_args* s, const char* who) {
    PWV_CHECK_ARG(s, "%s: args is NULL", who);
    if (int e = train_check_batch(&s->train, who, "train.struct_size", sizeof(pwv_train_shared_args), "pwv_train_shared_args")) return e;
    PWV_CHECK_ARG(s->head_in == PWV_TRAIN_HEAD_IN_GATED || s->head_in == PWV_TRAIN_HEAD_IN_SKIPSUM,
                  "%s: head_in %d is neither PWV_TRAIN_HEAD_IN_GATED (0) nor PWV_TRAIN_HEAD_IN_SKIPSUM (1)", who, s->head_in);
    return PWV_OK;
}

static int shared_head_params(const pwv_train_shared_args* s, const char* who, SharedHeadParams& p) {
    const pwv_train_args* a = &s->train;
    if (s->head_in == PWV_TRAIN_HEAD_IN_GATED) {
        PWV_CHECK_ARG(a->x, "%s: train.x is a NULL pointer (head_in GATED reads the last layer's o)", who);
        PWV_CHECK_ARG(a->skip, "%s: train.skip is a NULL pointer (head_in GATED)", who);
    } else {
        PWV_CHECK_ARG(s->skip_sum, "%s: skip_sum is a NULL pointer (head_in SKIPSUM)", who);
    }
    PWV_CHECK_ARG(a->post1 && a->post2, "%s: post1 or post2 is a NULL pointer", who);
    p = SharedHeadParams{};
    p.o = a->x; p.s = s->skip_sum; p.skip = a->skip; p.skip_bias = a->skip_bias; p.post1 = a->post1; p.post1_bias = a->post1_bias;
    p.post2 = a->post2; p.post2_bias = a->post2_bias;
    p.y0 = a->y; p.y1 = s->y_shift; p.d_out = a->d_out; p.d_mul = a->d_mul; p.d_o = a->d_o_out; p.d_s = s->d_skip_sum_out;
    p.part = (float*)a->workspace;
    p.rows = a->N * a->T;
    return PWV_OK;
}

}  // namespace pwv

using namespace pwv;

extern "C" size_t pwv_train_shared_workspace_bytes(const pwv_train_shared_args* s) {
    if (shared_check(s, "pwv_train_shared_workspace_bytes") != PWV_OK) return 0;
    const int units = (s->train.N * s->train.T + 31) / 32;
    return (size_t)train_grid_size(s->train.max_workgroups, units) * kSharedMaxPart * sizeof(float);
}

extern "C" int pwv_train_shared_head_fwd_f32(const pwv_train_shared_args* s, pwv_stream_t stream) {
    const char* who = "pwv_train_shared_head_fwd_f32";
    if (int e = shared_check(s, who)) return e;
    SharedHeadParams p;
    if (int e = shared_head_params(s, who, p)) return e;
    PWV_CHECK_ARG(p.y0, "%s: train.y is a NULL pointer", who);
    PWV_CHECK_ARG(p.y1, "%s: y_shift is a NULL pointer", who);
    const dim3 grid(train_grid_size(s->train.max_workgroups, (p.rows + 31) / 32)), blk(kTrThreads);
    if (s->head_in == PWV_TRAIN_HEAD_IN_GATED) hipLaunchKernelGGL(train_shared_head_fwd_kernel<GatedIn>, grid, blk, 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(train_shared_head_fwd_kernel<SumIn>, grid, blk, 0, (hipStream_t)stream, p);
    PWV_CHECK_HIP(hipGetLastError());
    return PWV_OK;
}

extern "C" int pwv_train_shared_head_bwd_f32(const pwv_train_shared_args* s, pwv_stream_t stream) {
    const char* who = "pwv_train_shared_head_bwd_f32";
    if (int e = shared_check(s, who)) return e;
    SharedHeadParams p;
    if (int e = shared_head_params(s, who, p)) return e;
    const pwv_train_args* a = &s->train;
    const bool gated = s->head_in == PWV_TRAIN_HEAD_IN_GATED;
    PWV_CHECK_ARG(a->d_out, "%s: train.d_out is a NULL pointer", who);
    if (gated) PWV_CHECK_ARG(a->d_o_out, "%s: train.d_o_out is a NULL pointer (head_in GATED)", who);
    else PWV_CHECK_ARG(s->d_skip_sum_out, "%s: d_skip_sum_out is a NULL pointer (head_in SKIPSUM)", who);
    const int grid = train_grid_size(a->max_workgroups, (p.rows + 31) / 32);
    PWV_CHECK_ARG(a->workspace, "%s: workspace is a NULL pointer", who);
    PWV_CHECK_ARG(a->workspace_bytes >= (size_t)grid * kSharedMaxPart * sizeof(float),
                  "%s: workspace_bytes %zu is short of the %zu pwv_train_shared_workspace_bytes gives", who, a->workspace_bytes,
                  (size_t)grid * kSharedMaxPart * sizeof(float));
    const dim3 grd(grid), blk(kTrThreads);
    if (gated) hipLaunchKernelGGL(train_shared_head_bwd_kernel<GatedIn>, grd, blk, 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(train_shared_head_bwd_kernel<SumIn>, grd, blk, 0, (hipStream_t)stream, p);
    PWV_CHECK_HIP(hipGetLastError());
    // stage two: (d skip |) column sums | d post1 | d b1 | d post2 | d b2
    const int total = gated ? shared_part<GatedIn>() : shared_part<SumIn>();
    ReduceParams rp;
    rp.part = p.part; rp.n_part = grid; rp.stride = total; rp.total = total; rp.n_seg = 0;
    int at = 0;
    auto seg = [&](int len, float* dst) {
        rp.seg[rp.n_seg++] = ReduceSeg{at, at + len, dst, nullptr};
        at += len;
    };
    if (gated) seg(64 * 128, a->d_skip);
    seg(128, a->d_skip_bias);
    seg(128 * 128, a->d_post1);
    seg(128, a->d_post1_bias);
    seg(256, a->d_post2);
    seg(2, a->d_post2_bias);
    return train_reduce(rp, (hipStream_t)stream);
}
