// The head of a training net ("The training head and the net driver written once"), forward and backward,
// written ONCE over an INPUT POLICY and the OUTPUT WIDTH Q:
//   GatedIn   begins at the last layer's o and forms h1 = relu(o skip + skip_bias) itself; dz1 goes back to d skip, d skip_bias, d o
//   SumIn     begins at the skip sum S, h1 = relu(S); dz1 is dS and its column sums are every layer's d skip_bias
//   Q         1: one output y (a net per flow and statistic); 2: y_0 the scale and y_1 the shift of a shared net
// Behind h1 there is one text: h2, the Q dots with post2's columns, dz2 from the Q dy planes, d post1, dh1.  The plan is the other
// training kernels' (csrc/pwv_train_units.h): 256 threads per 32-row unit, workgroup b takes units u = b (mod grid), operands in LDS at
// the odd strides kLdH / kLdW, weights in their TensorFlow layouts, weight gradients in accumulators over all units of the workgroup,
// ONE partial per workgroup, train_reduce_kernel's fixed order behind it.  No floating-point atomics.
// The kernels are one-line instances under the names of their headers: <GatedIn, 1> in csrc/pwv_train.hip, <SumIn, 1> in
// csrc/pwv_train_skip.hip, <In, 2> in csrc/pwv_train_shared.hip, each beside the entry points that check its ABI struct.
#ifndef PWV_TRAIN_HEAD_H
#define PWV_TRAIN_HEAD_H

#include "pwv_train_units.h"

namespace pwv {

struct HeadParams {
    const float *o, *s, *skip, *skip_bias, *post1, *post1_bias, *post2, *post2_bias;
    float* y[2];                                // forward: y (Q = 2: the scale and the shift plane)
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

template <class In, int Q>
constexpr int head_part() {                     // front | d post1 | d b1 | d post2 [128][Q] as it lies in TF's layout | d b2 [Q]
    return In::kFront + 128 * 128 + 128 + 128 * Q + Q;
}
constexpr int kMaxPart = head_part<GatedIn, 1>();           // the largest partial of the default architecture's kernels

// h1 and h2 = relu(h1 post1 + b1) of unit u; GatedIn leaves the unit's o in tl.o
template <class In>
__device__ __forceinline__ void head_hidden(typename In::Tile& tl, float* h1, float* h2, int u, const HeadParams& p) {
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

template <class In, int Q>
__device__ __forceinline__ void head_fwd_body(const HeadParams& p) {
    __shared__ typename In::Tile tl;
    __shared__ float h1[32 * kLdW];
    __shared__ float h2[32 * kLdW];
    const int units = (p.rows + 31) / 32;
    for (int u = blockIdx.x; u < units; u += gridDim.x) {
        head_hidden<In>(tl, h1, h2, u, p);
        // y_q[r] = h2[r] . post2[:, q] + b2[q]: 8 lanes per row, 16 columns each, then a fixed tree over the 8, for every column
        const int r = threadIdx.x >> 3, part = threadIdx.x & 7;
        float s[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) s[q] = 0.f;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const float v = h2[r * kLdW + 16 * part + e];
#pragma unroll
            for (int q = 0; q < Q; ++q) s[q] += v * p.post2[Q * (16 * part + e) + q];
        }
#pragma unroll
        for (int m = 1; m < 8; m *= 2) {
#pragma unroll
            for (int q = 0; q < Q; ++q) s[q] += __shfl_xor(s[q], m);
        }
        if (part == 0 && 32 * u + r < p.rows) {
#pragma unroll
            for (int q = 0; q < Q; ++q) p.y[q][32 * u + r] = s[q] + (p.post2_bias ? p.post2_bias[q] : 0.f);
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

// six accumulator tiles (GatedIn) stay in registers over a workgroup's units
template <class In, int Q>
__device__ __forceinline__ void head_bwd_body(const HeadParams& p) {
    __shared__ typename In::Tile tl;
    __shared__ float h1[32 * kLdW];             // h1, then dz1 (SumIn: = dS)
    __shared__ float h2[32 * kLdW];             // h2, then dz2
    __shared__ float dy[Q][32];                 // dy_0 = d_out d_mul, (Q = 2) dy_1 = d_out; zeros beyond the batch
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
    // thread c < 128: column c of d post2 (every q), d b1 and the policy's column sums; threads 128 .. 128 + Q - 1: d b2[q]
    float g_p20 = 0.f, g_p21 = 0.f, g_b1 = 0.f, g_col = 0.f, g_b2 = 0.f;
    for (int u = blockIdx.x; u < units; u += gridDim.x) {
        if (threadIdx.x < 32) {
            const int row = 32 * u + threadIdx.x;
            if constexpr (Q == 1) {
                dy[0][threadIdx.x] = row < p.rows ? p.d_out[row] * (p.d_mul ? p.d_mul[row] : 1.f) : 0.f;
            } else {
                const float d = row < p.rows ? p.d_out[row] : 0.f;
                dy[0][threadIdx.x] = row < p.rows ? d * (p.d_mul ? p.d_mul[row] : 1.f) : 0.f;
                dy[1][threadIdx.x] = d;
            }
        }
        head_hidden<In>(tl, h1, h2, u, p);      // (its barriers publish dy)
        if (threadIdx.x < 128) {                // d post2, dz2 = (sum_q dy_q post2[:, q]) where h2 > 0, d b1
            const int c = threadIdx.x;
            if constexpr (Q == 1) {
                const float w2 = p.post2[c];
                for (int r = 0; r < 32; ++r) {
                    const float v = h2[r * kLdW + c], z = v > 0.f ? dy[0][r] * w2 : 0.f;
                    g_p20 += v * dy[0][r];
                    g_b1 += z;
                    h2[r * kLdW + c] = z;
                }
            } else {
                const float w20 = p.post2[2 * c], w21 = p.post2[2 * c + 1];
#pragma unroll 4                                // (unrolled whole, the 32 rows' loads in flight cost 78 more registers: beyond 256)
                for (int r = 0; r < 32; ++r) {
                    const float v = h2[r * kLdW + c], z = v > 0.f ? dy[0][r] * w20 + dy[1][r] * w21 : 0.f;
                    g_p20 += v * dy[0][r];
                    g_p21 += v * dy[1][r];
                    g_b1 += z;
                    h2[r * kLdW + c] = z;
                }
            }
        } else if (threadIdx.x < 128 + Q) {
            const int q = Q == 1 ? 0 : threadIdx.x - 128;
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
            // the one-output head writes all 32 rows of the last block, the two-output head the rows of the batch alone
            if constexpr (Q == 1) lds_to_tile32(p.d_o, u, tl.o, kLdH, 0);
            else lds_to_tile32_rows(p.d_o, u, tl.o, kLdH, p.rows);
        } else {
            lds_to_tile32w(p.d_s, u, h1, kLdW, p.rows, 0);
        }
        __syncthreads();
    }
    float* part = p.part + (size_t)blockIdx.x * head_part<In, Q>();
    if constexpr (In::kGated) {
        for (int b = 0; b < 2; ++b) acc_to_part(g_skip[b], part, 128, 32 * b, 32 * w);
    }
    float* behind = part + In::kFront;
    for (int b = 0; b < 4; ++b) acc_to_part(g_post1[b], behind, 128, 32 * b, 32 * w);
    if (threadIdx.x < 128) {
        part[In::kFront - 128 + threadIdx.x] = g_col;
        behind[128 * 128 + threadIdx.x] = g_b1;
        behind[128 * 128 + 128 + Q * threadIdx.x] = g_p20;   // (c, q) at Q c + q: the reduction writes TF's layout as it lies
        if constexpr (Q == 2) behind[128 * 128 + 128 + Q * threadIdx.x + 1] = g_p21;
    } else if (threadIdx.x < 128 + Q) {
        behind[128 * 128 + 128 + 128 * Q + threadIdx.x - 128] = g_b2;
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// host: what the entry points share behind their own struct checks
// ------------------------------------------------------------------------------------------------------------------------------
// the optional fields are those of the larger structs: S and dS of the skip architecture, the shift plane of a shared net
inline HeadParams head_params(const pwv_train_args* a, int rows, const float* skip_sum = nullptr, float* d_skip_sum_out = nullptr,
                              float* y_shift = nullptr) {
    HeadParams p{};
    p.o = a->x; p.s = skip_sum; p.skip = a->skip; p.skip_bias = a->skip_bias; p.post1 = a->post1; p.post1_bias = a->post1_bias;
    p.post2 = a->post2; p.post2_bias = a->post2_bias;
    p.y[0] = a->y; p.y[1] = y_shift; p.d_out = a->d_out; p.d_mul = a->d_mul; p.d_o = a->d_o_out; p.d_s = d_skip_sum_out;
    p.part = (float*)a->workspace;
    p.rows = rows;
    return p;
}

inline int head_fwd_launch(void (*kernel)(HeadParams), const HeadParams& p, int grid, hipStream_t st) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kTrThreads), 0, st, p);
    PWV_CHECK_HIP(hipGetLastError());
    return PWV_OK;
}

// the backward launch and stage two of its partials, head_part<In, Q>() floats each: (d skip |) column sums | d post1 | d b1 |
// d post2 | d b2.  d_col: where the column sums go (GatedIn: d skip_bias; SumIn: every layer's d skip_bias)
template <class In, int Q>
int head_bwd_launch_and_reduce(void (*kernel)(HeadParams), const HeadParams& p, int grid, const pwv_train_args* a, float* d_col,
                               hipStream_t st) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kTrThreads), 0, st, p);
    PWV_CHECK_HIP(hipGetLastError());
    ReduceParams rp;
    rp.part = p.part; rp.n_part = grid; rp.stride = head_part<In, Q>(); rp.total = head_part<In, Q>(); rp.n_seg = 0;
    int at = 0;
    auto seg = [&](int len, float* dst) {
        rp.seg[rp.n_seg++] = ReduceSeg{at, at + len, dst, nullptr};
        at += len;
    };
    if (In::kGated) seg(64 * 128, a->d_skip);
    seg(128, d_col);
    seg(128 * 128, a->d_post1);
    seg(128, a->d_post1_bias);
    seg(128 * Q, a->d_post2);
    seg(Q, a->d_post2_bias);
    return train_reduce(rp, st);
}

}  // namespace pwv

#endif
