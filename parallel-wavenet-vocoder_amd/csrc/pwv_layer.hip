// Fused gated-residual WaveNet layer and post-processing head for gfx950 (MI355X).
//
// Replaces, per layer, the ~15 TensorFlow ops of WaveNet._create_dilation_layer
// (/root/reference/modules.py:185-259) and, per net, the post-processing of
// WaveNet.__call__ (modules.py:145-165).
//
// Design (measured history in HISTORY.md section 4):
//   * GEMM orientation: MFMA rows = output channels, MFMA columns = time.  A wave owns 32
//     consecutive samples; lane (t = lane&31, h = lane>>5) owns, of every 64-channel row, the
//     16-byte chunks at float offsets 8g + 4h -- which is exactly the v_mfma 32x32 C/D layout
//     (pwv::chan_of).  Hence x[t], x[t-d] are loaded straight from HBM into the B operand,
//     the gated output o stays in the registers it was accumulated in and IS the B operand of
//     the dense / skip GEMMs, and the residual add is a register add.  No LDS round trip and
//     no transposes for activations.
//   * Weights are the A operand, pre-packed (pwv_pack_*) so each lane reads 4 consecutive
//     k-steps with one conflict-free ds_read_b128; a workgroup loads one layer's weights
//     (80-152 KB of the 160 KB LDS) once and walks many time tiles (persistent over tiles).
//   * The conditioning term and the filter/gate biases enter as the accumulator's initial
//     value (frame-rate projection P), so the hoisted 'repeat' conditioning costs no FLOPs
//     in this kernel; per-sample conditioning (transposed-conv upsampling) adds 40 k-steps.
//   * fp32 arithmetic: v_mfma_f32_32x32x2_f32 (exact fp32 fma chains, 157 TFLOP/s peak).
#include "pwv_layer_common.h"
#include "pwv_layer_f32_tile.h"

#include <cstddef>
#include <cstdlib>
#include <cstring>

namespace pwv {

// Work is handed out in 32-row units (one MFMA column tile = one wave's worth of samples).
// 8 waves, two per SIMD (<= 256 registers each).  Waves pull units from a per-workgroup
// LDS counter and waves 4..7 (the second wave of each SIMD) run at raised priority, so
// the two waves of a SIMD drift out of phase: one wave's MFMAs cover the other's loads,
// gating, address arithmetic and stores (identical streams at equal priority stay in
// lockstep and hit their VALU sections together, leaving the matrix pipe idle).
// FIRST (layer 0 of a scalar-input net): the causal layer's output is not read but rebuilt from the flow input
//   with the front kernel's own two fp32 operations per channel (bit-identical to pwv_iaf_front_f32 + this kernel).
// HEAD  (plain gated last layer): head_f32_kernel<true>'s arithmetic runs behind the gate on the registers the
//   gated output was accumulated in; LDS holds exactly filter|gate + skip + postprocess1 = 160 KB, so the small vectors
//   come from global memory and units are handed out statically (no room for the counter).
// FOLD (with FIRST): layer 0's filter|gate convolution on the four scalars x[t-d-1], x[t-d], x[t-1], x[t] themselves
//   (pwv_pack_first_fold_f32; see layer_f16x3_kernel): two fp32 MFMA k-steps per row tile instead of 64.
// STREAM: see layer_f16x3_kernel (pwv_layer_f16.hip) -- history look-back instead of zeros, the chunk's last rows stored as the
//   next history.  The body is text included into both kernels (pwv_layer_f32_body.inc): the non-streaming instantiations keep
//   their names and their instruction streams.
template <bool SKIP, bool COND, bool GATED, bool FIRST = false, bool HEAD = false, bool FOLD = false>
__global__ __launch_bounds__(512) void layer_f32_kernel(const LayerParams p) {
    constexpr bool STREAM = false;
    const StreamParams st{};      // (not read)
#include "pwv_layer_f32_body.inc"
}

// the streaming forms: layer 0 folded (FIRST), the last layer + head (HEAD), else a plain residual layer
template <bool FIRST, bool HEAD>
__global__ __launch_bounds__(512) void layer_f32_stream_kernel(const LayerParams p, const StreamParams st) {
    constexpr bool STREAM = true, SKIP = false, COND = false, GATED = HEAD, FOLD = FIRST;
#include "pwv_layer_f32_body.inc"
}

// pwv_stream_carry_f32: the rows of the read blocks that a chunk of T rows does not push out, moved to the written blocks
// (new[k] = old[k + T], k < len - T), for every history of the model in one launch: block (entry, utterance); `tab` holds
// {float offset in a block, rows, floats per row (64: tile32 rows, 1: scalars), 0} per entry.
__global__ __launch_bounds__(256) void stream_carry_kernel(const StreamParams st, const int* __restrict__ tab, int T) {
    const int e = blockIdx.x, n = blockIdx.y;
    const int off = tab[4 * e], len = tab[4 * e + 1], width = tab[4 * e + 2];
    const int keep = len - T;
    if (keep <= 0) return;
    const int2 blk = reinterpret_cast<const int2*>(st.slot_tab)[n];
    const float* src = st.hist_rd + (long long)blk.x * st.block_stride + off;
    float* dst = st.hist_wr + (long long)blk.y * st.block_stride + off;
    if (width == 1) {
        for (int k = threadIdx.x; k < keep; k += blockDim.x) dst[k] = src[k + T];
        return;
    }
    // 32 consecutive rows of one channel quad per 32 threads: 512 B contiguous on the written side
    const int total = ((keep + 31) >> 5) * 512;
    for (int i = threadIdx.x; i < total; i += blockDim.x) {
        const int k = (i >> 9) * 32 + (i & 31), q = (i >> 5) & 15;
        if (k < keep) *reinterpret_cast<f32x4*>(dst + tile_off(k, q, 64)) = *reinterpret_cast<const f32x4*>(src + tile_off(k + T, q, 64));
    }
}

// --------------------------------------------------------------------------------------
// Head: (o @ skip + b | skip_sum) -> relu -> post1 -> relu -> post2     modules.py:145-165
// --------------------------------------------------------------------------------------
template <bool FROM_GATED>
__global__ __launch_bounds__(256) void head_f32_kernel(const HeadParams p) {
    constexpr int kLds = head_floats(kMaxQ);
    __shared__ __attribute__((aligned(16))) float lds[kLds];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = lane >> 5;
    const int net = blockIdx.x % p.G;
    const int wg = blockIdx.x / p.G;
    const int nwg = gridDim.x / p.G;
    const int Q = p.Q;
    fill_lds<head_floats(kMaxQ) / 4, 256>(lds, p.packed[net], tid);   // buffers are sized for kMaxQ
    __syncthreads();

    auto no_extra = [](int) {};
    const int rows = p.N * p.T;
    const int ntiles = (rows + 127) / 128;
    for (int tile = wg; tile < ntiles; tile += nwg) {
        const int row = tile * 128 + wave * 32 + (lane & 31);
        const bool valid = row < rows;
        f32x16 accs[4];
        f32x4 a[4];
        if constexpr (FROM_GATED) {
            float o[32];
            load_tiled<8, 64>(p.in[net], valid ? row : rows - 1, h, true, o);
#pragma unroll
            for (int it = 0; it < 4; ++it)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const f32x4 bs = *reinterpret_cast<const f32x4*>(&lds[kHBS + h * 64 + it * 16 + q * 4]);
#pragma unroll
                    for (int e = 0; e < 4; ++e) accs[it][q * 4 + e] = bs[e];
                }
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = frag(lds, kHAS, i, 8, 0, lane);
            gemm_groups<8, 4, 0, 1>(lds, kHAS, lane, accs, a, [&](int ks) -> float { return o[ks]; }, no_extra,
                                    [&](f32x4(&n)[4]) {
#pragma unroll
                                        for (int i = 0; i < 4; ++i) n[i] = frag(lds, kHA1, i, 16, 0, lane);
                                    });
        } else {
            const float* srow = p.in[net] + tile_off(valid ? row : rows - 1, h, 128);
#pragma unroll
            for (int it = 0; it < 4; ++it)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(srow + (8 * it + 2 * q) * 128);
#pragma unroll
                    for (int e = 0; e < 4; ++e) accs[it][q * 4 + e] = v[e];
                }
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = frag(lds, kHA1, i, 16, 0, lane);
        }
        // relu -> post1 (128 -> 128)
        f32x16 acc1[4];
#pragma unroll
        for (int it = 0; it < 4; ++it)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f32x4 b1 = *reinterpret_cast<const f32x4*>(&lds[kHB1 + h * 64 + it * 16 + q * 4]);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc1[it][q * 4 + e] = b1[e];
            }
        gemm_groups<16, 4, 0, 1>(
            lds, kHA1, lane, acc1, a, [&](int ks) -> float { return fmaxf(accs[ks >> 4][ks & 15], 0.f); }, no_extra,
            [](f32x4(&)[4]) {});
        // relu -> post2 (128 -> Q): per-lane partial dot over its 64 channels, then add the halves
        for (int q = 0; q < Q; ++q) {
            float part = 0.f;
            const float* w2 = &lds[kHW2 + (h * Q + q) * 64];
#pragma unroll
            for (int i4 = 0; i4 < 16; ++i4) {
                const f32x4 w = *reinterpret_cast<const f32x4*>(w2 + 4 * i4);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int i = 4 * i4 + e;
                    part = fmaf(fmaxf(acc1[i >> 4][i & 15], 0.f), w[e], part);
                }
            }
            part += __shfl_xor(part, 32);
            part += lds[kHW2 + 2 * Q * 64 + q];
            if (valid && h == 0) p.out[net][(size_t)row * Q + q] = part;
        }
    }
}

// --------------------------------------------------------------------------------------
// weight packing (device-side gathers from TensorFlow layouts)
// --------------------------------------------------------------------------------------
// pwv_pack_first_fold_f32 (see pack_first_fold_f16_kernel): [4 row tiles][64 lanes] f32x4 = {M[oc][h], M[oc][2 + h], 0, 0},
// the A values of the two fp32 MFMA k-steps (k = h and k = 2 + h) of lane (i, h), oc = 32 it + i
__global__ void pack_first_fold_f32_kernel(const float* __restrict__ cf, const float* __restrict__ filter, const float* __restrict__ gate,
                                           f32x4* __restrict__ out) {
    const int u = threadIdx.x;      // (it, lane)
    const int it = u >> 6, lane = u & 63, h = lane >> 5, oc = 32 * it + (lane & 31);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    for (int e = 0; e < 2; ++e) {
        const int k = 2 * e + h, tap = k >> 1, c = k & 1;
        double acc = 0.0;
        for (int cin = 0; cin < 64; ++cin) {
            const float wv = oc < 64 ? filter[(tap * 64 + cin) * 64 + oc] : gate[(tap * 64 + cin) * 64 + oc - 64];
            acc += (double)cf[c * 64 + cin] * (double)wv;
        }
        v[e] = (float)((double)(oc < 64 ? kFScale : kGScale) * acc);
    }
    out[u] = v;
}

__global__ void pack_layer_kernel(const float* filter, const float* gate, const float* dense,
                                  const float* dense_bias, const float* skip, const float* skip_bias,
                                  const float* gc_filter, const float* gc_gate, int with_skip, int cond_c,
                                  float* out, int total) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    float v = 0.f;
    int i = idx;
    if (i < kA1Size) {
        const int e = i & 3, lane = (i >> 2) & 63, ks4 = (i >> 8) & 15, it = i >> 12;
        const int ks = ks4 * 4 + e, tap = ks >> 5, r = ks & 31, h = lane >> 5;
        const int cin = 8 * (r >> 2) + 4 * h + (r & 3);
        const int oc = 32 * it + (lane & 31);
        v = oc < 64 ? kFScale * filter[(tap * 64 + cin) * 64 + oc] : kGScale * gate[(tap * 64 + cin) * 64 + oc - 64];
    } else if ((i -= kA1Size) < kA2Size) {
        const int e = i & 3, lane = (i >> 2) & 63, ks4 = (i >> 8) & 7, it = i >> 11;
        const int ks = ks4 * 4 + e, h = lane >> 5;
        const int c = chan_of(ks >> 4, ks & 15, h);
        v = dense[c * 64 + 32 * it + (lane & 31)];
    } else if ((i -= kA2Size) < kBDSize) {
        const int h = i >> 5, it = (i >> 4) & 1, r = i & 15;
        v = dense_bias ? dense_bias[chan_of(it, r, h)] : 0.f;
    } else {
        i -= kBDSize;
        bool done = false;
        if (with_skip) {
            if (i < kASSize) {
                const int e = i & 3, lane = (i >> 2) & 63, ks4 = (i >> 8) & 7, it = i >> 11;
                const int ks = ks4 * 4 + e, h = lane >> 5;
                const int c = chan_of(ks >> 4, ks & 15, h);
                v = skip[c * 128 + 32 * it + (lane & 31)];
                done = true;
            } else if ((i -= kASSize) < kBSSize) {
                const int h = i >> 6, it = (i >> 4) & 3, r = i & 15;
                v = skip_bias ? skip_bias[chan_of(it, r, h)] : 0.f;
                done = true;
            } else {
                i -= kBSSize;
            }
        }
        if (!done && cond_c > 0) {
            const int nc8 = cond_c / 8;
            const int e = i & 3, lane = (i >> 2) & 63;
            const int rest = i >> 8;  // it * nc8 + ks4
            const int ks4 = rest % nc8, it = rest / nc8;
            const int r = ks4 * 4 + e, h = lane >> 5;
            const int ci = 8 * (r >> 2) + 4 * h + (r & 3);
            const int oc = 32 * it + (lane & 31);
            v = oc < 64 ? kFScale * gc_filter[ci * 64 + oc] : kGScale * gc_gate[ci * 64 + oc - 64];
        }
    }
    out[idx] = v;
}

__global__ void pack_head_kernel(const float* skip, const float* skip_bias, const float* post1,
                                 const float* post1_bias, const float* post2, const float* post2_bias, int Q,
                                 float* out, int total) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    float v = 0.f;
    int i = idx;
    if (i < kASSize) {
        const int e = i & 3, lane = (i >> 2) & 63, ks4 = (i >> 8) & 7, it = i >> 11;
        const int ks = ks4 * 4 + e, h = lane >> 5;
        v = skip ? skip[chan_of(ks >> 4, ks & 15, h) * 128 + 32 * it + (lane & 31)] : 0.f;
    } else if ((i -= kASSize) < kBSSize) {
        const int h = i >> 6, it = (i >> 4) & 3, r = i & 15;
        v = skip_bias ? skip_bias[chan_of(it, r, h)] : 0.f;
    } else if ((i -= kBSSize) < kHA1Size) {
        const int e = i & 3, lane = (i >> 2) & 63, ks4 = (i >> 8) & 15, it = i >> 12;
        const int ks = ks4 * 4 + e, h = lane >> 5;
        v = post1[chan_of(ks >> 4, ks & 15, h) * 128 + 32 * it + (lane & 31)];
    } else if ((i -= kHA1Size) < 128) {
        const int h = i >> 6, it = (i >> 4) & 3, r = i & 15;
        v = post1_bias ? post1_bias[chan_of(it, r, h)] : 0.f;
    } else if ((i -= 128) < 2 * Q * 64) {
        const int j = i & 63, hq = i >> 6;
        const int q = hq % Q, h = hq / Q;
        v = post2[chan_of(j >> 4, j & 15, h) * Q + q];
    } else {
        i -= 2 * Q * 64;
        v = (i < Q && post2_bias) ? post2_bias[i] : 0.f;
    }
    out[idx] = v;
}

template <bool SKIP, bool COND, bool GATED, bool FIRST = false, bool HEAD = false, bool FOLD = false>
static int launch_layer(const LayerParams& lp, int per_net, hipStream_t s) {
    hipLaunchKernelGGL((layer_f32_kernel<SKIP, COND, GATED, FIRST, HEAD, FOLD>), dim3(per_net * lp.G), dim3(512), 0, s, lp);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(PWV_EHIP, "layer kernel launch failed: %s", hipGetErrorString(e));
    return PWV_OK;
}

}  // namespace pwv

using namespace pwv;

extern "C" {

size_t pwv_layer_packed_floats(int with_skip, int cond_channels) {
    return (size_t)layer_floats(with_skip != 0, cond_channels > 0);
}

size_t pwv_head_packed_floats(int Q) {
    (void)Q;   // one size for every Q <= kMaxQ: the kernels copy a fixed-size block into LDS
    return (size_t)head_floats(kMaxQ);
}

int pwv_proj_column_map(int* map128) {
    if (!map128) return set_error(PWV_EINVAL, "map128 is NULL");
    for (int h = 0; h < 2; ++h)
        for (int it = 0; it < 4; ++it)
            for (int r = 0; r < 16; ++r) map128[h * 64 + it * 16 + r] = chan_of(it, r, h);
    return PWV_OK;
}

int pwv_pack_layer_f32(const float* filter, const float* gate, const float* dense, const float* dense_bias,
                       const float* skip, const float* skip_bias, const float* gc_filter, const float* gc_gate,
                       int with_skip, int cond_channels, int precision, float* packed, pwv_stream_t stream) {
    PWV_CHECK_ARG(filter && gate && dense && packed, "pwv_pack_layer_f32: NULL weight pointer");
    PWV_CHECK_ARG(!with_skip || skip, "pwv_pack_layer_f32: with_skip needs skip weights");
    PWV_CHECK_ARG(cond_channels == 0 || cond_channels == kCondC,
                  "pwv_pack_layer_f32: per-sample conditioning supports %d channels, got %d", kCondC, cond_channels);
    PWV_CHECK_ARG(cond_channels == 0 || (gc_filter && gc_gate), "pwv_pack_layer_f32: gc weights missing");
    PWV_CHECK_ARG(precision >= PWV_PREC_F32 && precision <= PWV_PREC_F16, "pwv_pack_layer_f32: unsupported precision %d", precision);
    PWV_CHECK_ARG(precision != PWV_PREC_F16 || !with_skip, "pwv_pack_layer_f32: PWV_PREC_F16 does not support skip accumulation");
    if (precision != PWV_PREC_F32)   // the fp16 mode reads the `hi` halves of the split-fp16 layout
        return launch_pack_layer_f16x3(filter, gate, dense, dense_bias, skip, skip_bias, gc_filter, gc_gate, with_skip,
                                       cond_channels, packed, (hipStream_t)stream);
    const int total = layer_floats(with_skip != 0, cond_channels > 0);
    hipLaunchKernelGGL(pack_layer_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, filter, gate,
                       dense, dense_bias, skip, skip_bias, gc_filter, gc_gate, with_skip, cond_channels, packed, total);
    PWV_CHECK_HIP(hipGetLastError());
    return PWV_OK;
}

int pwv_pack_first_fold_f32(const float* causal_filter, const float* filter, const float* gate, float* folded, pwv_stream_t stream) {
    PWV_CHECK_ARG(causal_filter && filter && gate && folded, "pwv_pack_first_fold_f32: NULL pointer");
    hipLaunchKernelGGL(pack_first_fold_f32_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, causal_filter, filter, gate,
                       reinterpret_cast<f32x4*>(folded));
    PWV_CHECK_HIP(hipGetLastError());
    return PWV_OK;
}

int pwv_pack_first_fold_f16x3(const float* causal_filter, const float* filter, const float* gate, float* folded, pwv_stream_t stream) {
    PWV_CHECK_ARG(causal_filter && filter && gate && folded, "pwv_pack_first_fold_f16x3: NULL pointer");
    return launch_pack_first_fold_f16x3(causal_filter, filter, gate, folded, (hipStream_t)stream);
}

int pwv_pack_head_f32(const float* skip, const float* skip_bias, const float* post1, const float* post1_bias,
                      const float* post2, const float* post2_bias, int Q, int precision, float* packed,
                      pwv_stream_t stream) {
    PWV_CHECK_ARG(post1 && post2 && packed, "pwv_pack_head_f32: NULL weight pointer");
    PWV_CHECK_ARG(Q >= 1 && Q <= kMaxQ, "pwv_pack_head_f32: Q must be in [1,%d], got %d", kMaxQ, Q);
    PWV_CHECK_ARG(precision >= PWV_PREC_F32 && precision <= PWV_PREC_F16, "pwv_pack_head_f32: unsupported precision %d", precision);
    if (precision != PWV_PREC_F32)
        return launch_pack_head_f16x3(skip, skip_bias, post1, post1_bias, post2, post2_bias, Q, packed, (hipStream_t)stream);
    const int total = head_floats(Q);
    hipLaunchKernelGGL(pack_head_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, skip, skip_bias,
                       post1, post1_bias, post2, post2_bias, Q, packed, total);
    PWV_CHECK_HIP(hipGetLastError());
    return PWV_OK;
}

}  // extern "C"

// pwv_wavenet_layer_f32 (st == NULL) and pwv_wavenet_layer_stream_f32: checks, kernel parameters, grid, instantiation
static int layer_call(const pwv_layer_args* a, const StreamParams* st, pwv_stream_t stream) {
    PWV_CHECK_ARG(a, "pwv_wavenet_layer_f32: args is NULL");
    PWV_CHECK_ARG(a->G >= 1 && a->G <= PWV_MAX_NETS, "pwv_wavenet_layer_f32: G=%d out of range", a->G);
    PWV_CHECK_ARG(a->N >= 1 && a->T >= 1 && a->dilation >= 1, "pwv_wavenet_layer_f32: bad N/T/dilation");
    PWV_CHECK_ARG((long long)a->N * a->T < (1ll << 31) - 256, "pwv_wavenet_layer_f32: N*T too large");
    PWV_CHECK_ARG(a->precision >= PWV_PREC_F32 && a->precision <= PWV_PREC_F16, "pwv_wavenet_layer_f32: unsupported precision %d", a->precision);
    PWV_CHECK_ARG(a->cond_channels == 0 || a->cond_channels == kCondC,
                  "pwv_wavenet_layer_f32: per-sample conditioning supports %d channels", kCondC);
    PWV_CHECK_ARG((a->cond_channels > 0) == (a->cond != nullptr), "pwv_wavenet_layer_f32: cond / cond_channels mismatch");
    PWV_CHECK_ARG(a->proj_row_stride % 4 == 0, "pwv_wavenet_layer_f32: proj_row_stride must be a multiple of 4");
    PWV_CHECK_ARG(a->cond_hop >= 0, "pwv_wavenet_layer_f32: cond_hop < 0");
    LayerParams lp{};
    bool any_skip = false;
    for (int g = 0; g < a->G; ++g) {
        PWV_CHECK_ARG((a->x_in[g] || a->x_first) && (a->x_out[g] || a->head_packed[g]) && a->packed[g] && a->proj[g],
                      "pwv_wavenet_layer_f32: NULL buffer for net %d", g);
        PWV_CHECK_ARG(!a->head_packed[0] == !a->head_packed[g] && (!a->head_packed[g] || a->head_out[g]),
                      "pwv_wavenet_layer_f32: head_packed / head_out must be set for all nets or none");
        lp.packed_head[g] = a->head_packed[g];
        lp.head_out[g] = a->head_out[g];
        PWV_CHECK_ARG(!a->x_first || a->causal_filter[g], "pwv_wavenet_layer_f32: x_first needs causal_filter for net %d", g);
        lp.cfilt[g] = a->causal_filter[g];
        lp.fold0[g] = a->x_first ? a->first_fold[g] : nullptr;
        PWV_CHECK_ARG((lp.fold0[g] == nullptr) == (lp.fold0[0] == nullptr), "pwv_wavenet_layer_f32: first_fold must be set for all nets or for none");
        PWV_CHECK_ARG(a->x_in[g] != a->x_out[g], "pwv_wavenet_layer_f32: in-place layers are not supported (x[t-d] halo)");
        lp.x_in[g] = a->x_in[g];
        lp.x_out[g] = a->x_out[g];
        lp.packed[g] = a->packed[g];
        lp.proj[g] = a->proj[g];
        lp.skip[g] = a->skip[g];
        any_skip = any_skip || a->skip[g];
    }
    for (int g = 0; g < a->G; ++g)
        PWV_CHECK_ARG(!any_skip || a->skip[g], "pwv_wavenet_layer_f32: skip must be set for all nets or none");
    const bool half16 = a->precision == PWV_PREC_F16;      // (its fused head has room for the per-sample condition weights)
    PWV_CHECK_ARG(!a->x_first || !any_skip, "pwv_wavenet_layer_f32: x_first does not support skip accumulation");
    PWV_CHECK_ARG(!a->head_packed[0] || (a->out_mode == PWV_OUT_GATED && !any_skip && (!a->cond || half16) && !a->x_first && a->head_q >= 1 && a->head_q <= kMaxQ),
                  "pwv_wavenet_layer_f32: a fused head needs out_mode PWV_OUT_GATED, no skip accumulation, no per-sample condition (PWV_PREC_F16: "
                  "allowed) and head_q in [1,%d]", kMaxQ);
    lp.head_q = a->head_q;
    lp.x_first = a->x_first;
    lp.x_limit = a->x_limit;
    lp.range_flag = a->x_first ? a->range_flag : nullptr;
    lp.cond = a->cond;
    lp.proj_row_stride = a->proj_row_stride;
    lp.G = a->G;
    lp.N = a->N;
    lp.T = a->T;
    lp.dilation = a->dilation;
    lp.cond_hop = a->cond_hop;
    lp.cond_offset = a->cond_offset;
    lp.cond_frames = a->cond_frames;
    lp.skip_init = a->skip_init;
    make_magic((unsigned)a->T, lp.T_magic, lp.T_shift);
    make_magic((unsigned)(a->cond_hop > 0 ? a->cond_hop : 1), lp.hop_magic, lp.hop_shift);
    lp.trace = nullptr;
#ifdef PWV_TRACE
    { const char* e = getenv("PWV_TRACE_PTR"); if (e) lp.trace = (long long*)strtoull(e, nullptr, 0); }
#endif

    const int cus = device_cus();
    if (cus <= 0) return set_error(PWV_EHIP, "no HIP device");
    const long long rows = (long long)a->N * a->T;
    int per_net = (a->max_workgroups > 0 ? a->max_workgroups : cus) / a->G;
    if (per_net < 1) per_net = 1;
    const int nt4 = (int)((rows + 127) / 128), nt8 = (int)((rows + 255) / 256);   // >= 1 unit per wave
    const int g8 = per_net < nt8 ? per_net : nt8;
    // the write-through stores address a workgroup's own units with 32-bit byte offsets (units_rsrc / units_off): 16 KB per
    // unit of the widest buffer (skip accumulators) must stay below 2 GB per workgroup
    PWV_CHECK_ARG(((rows + 31) / 32 + g8 - 1) / g8 < (1 << 17),
                  "pwv_wavenet_layer_f32: %lld rows on %d workgroups per net: more than 131071 units per workgroup (raise max_workgroups)",
                  rows, g8);
    hipStream_t s = (hipStream_t)stream;
    const bool cond = a->cond != nullptr, gated = a->out_mode == PWV_OUT_GATED;
    PWV_CHECK_ARG(a->out_mode == PWV_OUT_GATED || a->out_mode == PWV_OUT_RESIDUAL, "pwv_wavenet_layer_f32: bad out_mode");
    if (st) {      // (pwv_wavenet_layer_stream_f32 has checked that the layer is one of the three streaming forms)
        if (cond) return launch_layer_stream_cond(lp, *st, a->precision == PWV_PREC_F16X3, gated, g8, s);      // (pwv_wavenet_layer_stream_cond_f32 has)
        if (any_skip) return launch_layer_stream_skip(lp, *st, a->precision == PWV_PREC_F16X3, gated, g8, s);      // (pwv_wavenet_layer_stream_skip_f32 has)
        if (a->precision == PWV_PREC_F16X3) return launch_layer_f16x3_stream(lp, *st, g8, s);
        const dim3 grid(g8 * lp.G);
        if (lp.packed_head[0]) hipLaunchKernelGGL((layer_f32_stream_kernel<false, true>), grid, dim3(512), 0, s, lp, *st);
        else if (lp.x_first) hipLaunchKernelGGL((layer_f32_stream_kernel<true, false>), grid, dim3(512), 0, s, lp, *st);
        else hipLaunchKernelGGL((layer_f32_stream_kernel<false, false>), grid, dim3(512), 0, s, lp, *st);
        PWV_CHECK_HIP(hipGetLastError());
        return PWV_OK;
    }
    if (a->precision == PWV_PREC_F16X3) return launch_layer_f16x3(lp, any_skip, cond, gated, g8, s);
    if (a->precision == PWV_PREC_F16) {
        PWV_CHECK_ARG(!any_skip, "pwv_wavenet_layer_f32: PWV_PREC_F16 does not support skip accumulation");
        // 4-wave workgroups with 40 KB (60 KB with cond) of LDS: several per CU
        if (lp.packed_head[0]) return launch_layer_h16(lp, cond, gated, g8, s);      // fused head: one 8-wave workgroup per CU
        const int want = per_net * (cond ? 2 : 3);
        return launch_layer_h16(lp, cond, gated, want < nt4 ? want : nt4, s);
    }
    if (lp.packed_head[0]) return launch_layer<false, false, true, false, true>(lp, g8, s);
    if (lp.x_first && lp.fold0[0]) {
        if (cond) return gated ? launch_layer<false, true, true, true, false, true>(lp, g8, s) : launch_layer<false, true, false, true, false, true>(lp, g8, s);
        return gated ? launch_layer<false, false, true, true, false, true>(lp, g8, s) : launch_layer<false, false, false, true, false, true>(lp, g8, s);
    }
    if (lp.x_first) {
        if (cond) return gated ? launch_layer<false, true, true, true>(lp, g8, s) : launch_layer<false, true, false, true>(lp, g8, s);
        return gated ? launch_layer<false, false, true, true>(lp, g8, s) : launch_layer<false, false, false, true>(lp, g8, s);
    }
    if (any_skip) {
        if (cond) return gated ? launch_layer<true, true, true>(lp, g8, s) : launch_layer<true, true, false>(lp, g8, s);
        return gated ? launch_layer<true, false, true>(lp, g8, s) : launch_layer<true, false, false>(lp, g8, s);
    }
    if (cond) return gated ? launch_layer<false, true, true>(lp, g8, s) : launch_layer<false, true, false>(lp, g8, s);
    return gated ? launch_layer<false, false, true>(lp, g8, s) : launch_layer<false, false, false>(lp, g8, s);
}

// pwv_stream_args as far as the caller's struct_size reaches (the rest zero) and the kernels' view of it; returns why not, or NULL
static const char* stream_args(const pwv_stream_args* sa, pwv_stream_args& out, StreamParams& st) {
    if (!sa) return "args is NULL";
    if (sa->struct_size < offsetof(pwv_stream_args, carry_tab) || sa->struct_size > 4096) return "struct_size does not cover the history fields";
    out = pwv_stream_args{};
    memcpy(&out, sa, sa->struct_size < sizeof(out) ? sa->struct_size : sizeof(out));
    if (!out.hist_rd || !out.hist_wr || !out.slot_tab) return "NULL history / slot table";
    if (out.block_stride == 0 || out.block_stride % 4) return "block_stride must be a positive multiple of 4 floats";
    st.hist_rd = out.hist_rd;
    st.hist_wr = out.hist_wr;
    st.slot_tab = out.slot_tab;
    st.block_stride = (long long)out.block_stride;
    for (int g = 0; g < PWV_MAX_NETS; ++g) st.row_off[g] = (long long)out.row_off[g];
    st.scalar_off = (long long)out.scalar_off;
    return nullptr;
}

namespace pwv {
const char* stream_args_view(const pwv_stream_args* sa, pwv_stream_args& out, StreamParams& st) { return stream_args(sa, out, st); }
int layer_call_stream(const pwv_layer_args* a, const StreamParams& st, pwv_stream_t stream) { return layer_call(a, &st, stream); }
}  // namespace pwv

extern "C" {

int pwv_wavenet_layer_f32(const pwv_layer_args* a, pwv_stream_t stream) { return layer_call(a, nullptr, stream); }

int pwv_wavenet_layer_stream_f32(const pwv_layer_args* a, const pwv_stream_args* sa, pwv_stream_t stream) {
    PWV_CHECK_ARG(a, "pwv_wavenet_layer_stream_f32: args is NULL");
    pwv_stream_args v;
    StreamParams st{};
    const char* why = stream_args(sa, v, st);
    PWV_CHECK_ARG(!why, "pwv_wavenet_layer_stream_f32: %s", why);
    PWV_CHECK_ARG(!v.cu_rows, "pwv_wavenet_layer_stream_f32: hist->cu_rows is set: the per-layer kernels have no packed form (the persistent launch has)");
    PWV_CHECK_ARG(a->precision == PWV_PREC_F32 || a->precision == PWV_PREC_F16X3,
                  "pwv_wavenet_layer_stream_f32: PWV_PREC_F32 / PWV_PREC_F16X3 only (the fp16 storage mode has no streaming form)");
    PWV_CHECK_ARG(a->G >= 1 && a->G <= PWV_MAX_NETS && a->dilation >= 1 && a->T >= 1, "pwv_wavenet_layer_stream_f32: bad G / dilation / T");
    PWV_CHECK_ARG(!a->cond && a->cond_channels == 0, "pwv_wavenet_layer_stream_f32: per-sample conditioning has no streaming form");
    const long long hist_rows = ((long long)a->dilation + 31) / 32 * 32;
    for (int g = 0; g < a->G; ++g) {
        PWV_CHECK_ARG(!a->skip[g], "pwv_wavenet_layer_stream_f32: skip accumulation has no streaming form");
        PWV_CHECK_ARG(!a->x_first || a->first_fold[g], "pwv_wavenet_layer_stream_f32: layer 0 streams in its folded form only (first_fold)");
        PWV_CHECK_ARG(a->x_first || (v.row_off[g] % 4 == 0 && v.row_off[g] + (size_t)hist_rows * 64 <= v.block_stride),
                      "pwv_wavenet_layer_stream_f32: row_off[%d] + round32(dilation) rows leave the history block", g);
        for (int o = 0; o < g && !a->x_first; ++o)
            PWV_CHECK_ARG(v.row_off[o] + (size_t)hist_rows * 64 <= v.row_off[g] || v.row_off[g] + (size_t)hist_rows * 64 <= v.row_off[o],
                          "pwv_wavenet_layer_stream_f32: the nets' row histories overlap");
    }
    PWV_CHECK_ARG(!a->x_first || v.scalar_off + (size_t)a->dilation + 1 <= v.block_stride,
                  "pwv_wavenet_layer_stream_f32: scalar_off + dilation + 1 scalars leave the history block");
    if (a->head_packed[0]) PWV_CHECK_ARG(a->out_mode == PWV_OUT_GATED && !a->x_first, "pwv_wavenet_layer_stream_f32: a fused head needs out_mode PWV_OUT_GATED");
    else PWV_CHECK_ARG(a->out_mode == PWV_OUT_RESIDUAL, "pwv_wavenet_layer_stream_f32: without a fused head the streaming layer is out_mode PWV_OUT_RESIDUAL");
    return layer_call(a, &st, stream);
}

int pwv_stream_carry_f32(const pwv_stream_args* sa, int N, int T, pwv_stream_t stream) {
    pwv_stream_args v;
    StreamParams st{};
    const char* why = stream_args(sa, v, st);
    PWV_CHECK_ARG(!why, "pwv_stream_carry_f32: %s", why);
    PWV_CHECK_ARG(sa->struct_size >= offsetof(pwv_stream_args, n_carry) + sizeof(int32_t) && v.carry_tab && v.n_carry >= 1 && v.n_carry <= 65535,
                  "pwv_stream_carry_f32: carry_tab / n_carry missing");
    PWV_CHECK_ARG(N >= 1 && N <= 65535 && (v.cu_rows || T >= 1), "pwv_stream_carry_f32: bad N / T");
    if (v.cu_rows)      // the packed form: T is not read, session n's own T_n = cu_rows[n+1] - cu_rows[n]
        return launch_stream_carry_ragged(st, v.carry_tab, v.n_carry, v.cu_rows, N, (hipStream_t)stream);      // (pwv_stack_persist.hip, next to the ragged flow kernel)
    else
        hipLaunchKernelGGL(stream_carry_kernel, dim3(v.n_carry, N), dim3(256), 0, (hipStream_t)stream, st, v.carry_tab, T);
    PWV_CHECK_HIP(hipGetLastError());
    return PWV_OK;
}

int pwv_wavenet_head_f32(const pwv_head_args* a, pwv_stream_t stream) {
    PWV_CHECK_ARG(a, "pwv_wavenet_head_f32: args is NULL");
    PWV_CHECK_ARG(a->G >= 1 && a->G <= PWV_MAX_NETS, "pwv_wavenet_head_f32: G=%d out of range", a->G);
    PWV_CHECK_ARG(a->N >= 1 && a->T >= 1, "pwv_wavenet_head_f32: bad N/T");
    PWV_CHECK_ARG((long long)a->N * a->T < (1ll << 31) - 256, "pwv_wavenet_head_f32: N*T too large");
    PWV_CHECK_ARG(a->Q >= 1 && a->Q <= kMaxQ, "pwv_wavenet_head_f32: Q must be in [1,%d]", kMaxQ);
    PWV_CHECK_ARG(a->precision >= PWV_PREC_F32 && a->precision <= PWV_PREC_F16, "pwv_wavenet_head_f32: unsupported precision %d", a->precision);
    PWV_CHECK_ARG(a->in_mode == PWV_HEAD_IN_GATED || a->in_mode == PWV_HEAD_IN_SKIPSUM, "pwv_wavenet_head_f32: bad in_mode");
    HeadParams hp{};
    for (int g = 0; g < a->G; ++g) {
        PWV_CHECK_ARG(a->in[g] && a->packed[g] && a->out[g], "pwv_wavenet_head_f32: NULL buffer for net %d", g);
        hp.in[g] = a->in[g];
        hp.packed[g] = a->packed[g];
        hp.out[g] = a->out[g];
    }
    hp.G = a->G;
    hp.N = a->N;
    hp.T = a->T;
    hp.Q = a->Q;
    const int cus = device_cus();
    if (cus <= 0) return set_error(PWV_EHIP, "no HIP device");
    const long long rows = (long long)a->N * a->T;
    int ntiles = (int)((rows + 127) / 128);
    int per_net = (a->max_workgroups > 0 ? a->max_workgroups : cus) / a->G;
    if (per_net < 1) per_net = 1;
    if (a->precision == PWV_PREC_F16X3) ntiles = (int)((rows + 255) / 256);   // 8-wave workgroups: >= 1 unit per wave
    if (a->precision == PWV_PREC_F16) {
        PWV_CHECK_ARG(a->in_mode == PWV_HEAD_IN_GATED, "pwv_wavenet_head_f32: PWV_PREC_F16 needs in_mode PWV_HEAD_IN_GATED");
        per_net *= 3;
        if (per_net > ntiles) per_net = ntiles;
        return launch_head_h16(hp, per_net * a->G, (hipStream_t)stream);
    }
    if (per_net > ntiles) per_net = ntiles;
    const int grid = per_net * a->G;
    if (a->precision == PWV_PREC_F16X3)
        return launch_head_f16x3(hp, a->in_mode == PWV_HEAD_IN_GATED, grid, (hipStream_t)stream);
    if (a->in_mode == PWV_HEAD_IN_GATED)
        hipLaunchKernelGGL((head_f32_kernel<true>), dim3(grid), dim3(256), 0, (hipStream_t)stream, hp);
    else
        hipLaunchKernelGGL((head_f32_kernel<false>), dim3(grid), dim3(256), 0, (hipStream_t)stream, hp);
    PWV_CHECK_HIP(hipGetLastError());
    return PWV_OK;
}

int pwv_wavenet_stack_f32(const pwv_stack_args* a, pwv_stream_t const* streams) {
    PWV_CHECK_ARG(a && streams, "pwv_wavenet_stack_f32: NULL args / stream array");   // streams[0] may be the NULL (default) stream
    PWV_CHECK_ARG(a->G >= 1 && a->G <= PWV_MAX_NETS, "pwv_wavenet_stack_f32: G=%d out of range", a->G);
    PWV_CHECK_ARG(a->n_layers >= 1 && a->dilations, "pwv_wavenet_stack_f32: no layers");
    const bool two = a->G == 2 && streams[1] != nullptr;
    const int groups = two ? 2 : 1;           // launch groups per layer
    const int per_group = two ? 1 : a->G;     // nets per launch
    int wgs = a->max_workgroups;
    if (two && wgs == 0) {
        const int cus = device_cus();
        if (cus <= 0) return set_error(PWV_EHIP, "no HIP device");
        wgs = cus / 2 > 0 ? cus / 2 : 1;
    }
    const bool use_skip = a->skip[0] != nullptr;
    // split-fp16 and fp32 paths, plain last layer: the head runs inside the last layer's launch (pwv_layer_args.head_packed)
    const bool fuse_head = !a->separate_head && !use_skip && (!a->cond || a->precision == PWV_PREC_F16) && a->n_layers >= 2;
    int cur = 0;
    for (int j = 0; j < a->n_layers; ++j) {
        const bool last = j == a->n_layers - 1;
        for (int grp = 0; grp < groups; ++grp) {
            pwv_layer_args la{};
            la.G = per_group;
            for (int i = 0; i < per_group; ++i) {
                const int g = two ? grp : i;
                la.x_in[i] = cur ? a->buf1[g] : a->buf0[g];
                la.x_out[i] = cur ? a->buf0[g] : a->buf1[g];
                la.packed[i] = a->packed_layers[g] + (size_t)j * a->packed_layer_stride;
                la.proj[i] = a->proj[g] + (size_t)128 * j;
                la.skip[i] = use_skip ? a->skip[g] : nullptr;
            }
            la.proj_row_stride = a->proj_row_stride;
            la.cond = a->cond;
            la.cond_channels = a->cond_channels;
            la.skip_init = j == 0;
            la.N = a->N;
            la.T = a->T;
            la.dilation = a->dilations[j];
            la.cond_hop = a->cond_hop;
            la.cond_offset = a->cond_offset;
            la.cond_frames = a->cond_frames;
            la.out_mode = last ? PWV_OUT_GATED : PWV_OUT_RESIDUAL;
            la.precision = a->precision;
            la.max_workgroups = wgs;
            if (last && fuse_head) {
                for (int i = 0; i < per_group; ++i) {
                    const int g = two ? grp : i;
                    la.head_packed[i] = a->packed_head[g];
                    la.head_out[i] = a->out[g];
                }
                la.head_q = a->Q;
            }
            if (j == 0 && a->x_first) {
                la.x_first = a->x_first;
                la.x_limit = a->x_limit;
                la.range_flag = a->range_flag;
                for (int i = 0; i < per_group; ++i) {
                    la.causal_filter[i] = a->causal_filter[two ? grp : i];
                    la.first_fold[i] = a->first_fold[two ? grp : i];
                }
            }
            if (j == 0 && a->ev_begin[grp]) PWV_CHECK_HIP(hipEventRecord((hipEvent_t)a->ev_begin[grp], (hipStream_t)streams[grp]));
            const int rc = pwv_wavenet_layer_f32(&la, streams[grp]);
            if (rc != PWV_OK) return rc;
            if (j == a->n_layers - 2 && a->ev_end[grp]) PWV_CHECK_HIP(hipEventRecord((hipEvent_t)a->ev_end[grp], (hipStream_t)streams[grp]));
        }
        cur ^= 1;
    }
    for (int grp = 0; grp < groups && !fuse_head; ++grp) {
        pwv_head_args ha{};
        ha.G = per_group;
        for (int i = 0; i < per_group; ++i) {
            const int g = two ? grp : i;
            ha.in[i] = use_skip ? a->skip[g] : (cur ? a->buf1[g] : a->buf0[g]);
            ha.packed[i] = a->packed_head[g];
            ha.out[i] = a->out[g];
        }
        ha.N = a->N;
        ha.T = a->T;
        ha.Q = a->Q;
        ha.in_mode = use_skip ? PWV_HEAD_IN_SKIPSUM : PWV_HEAD_IN_GATED;
        ha.precision = a->precision;
        ha.max_workgroups = wgs;
        const int rc = pwv_wavenet_head_f32(&ha, streams[grp]);
        if (rc != PWV_OK) return rc;
    }
    return PWV_OK;
}

}  // extern "C"
