// Split-fp16 ("f16x3") variants of the fused layer / head kernels for gfx950.
//
// Same math, layouts in HBM, register ownership and launch structure as pwv_layer.hip (the
// reference call sites are /root/reference/modules.py:185-259 and :145-165), but the GEMMs run on
// v_mfma_f32_32x32x16_f16 (16x the fp32 MFMA rate) with error compensation:
//
//     w*x  ~=  w_hi*x_hi + w_hi*x_lo + w_lo*x_hi,     v_hi = fp16(v),  v_lo = fp16(v - v_hi)
//
// accumulated in fp32.  fp16 products are exact in the fp32 accumulator; the dropped term w_lo*x_lo
// is ~2^-22 |w x|, and each operand is represented to max(2^-22 |v|, 2^-25) (gfx950 keeps fp16
// subnormals in MFMA inputs and conversions -- tools/probes/f16_denorm.hip -- so no rescaling of the
// low parts is needed).  Activations stay fp32 in HBM; the split happens in registers.
// Per 32-sample unit: 120 MFMAs x 32 cycles = 3,840 matrix cycles instead of 320 x 64 = 20,480.
#include "pwv_f16x3.h"

namespace pwv {

// --------------------------------------------------------------------------------------
// fused gated-residual layer, split-fp16 arithmetic (8 waves, dynamic 32-sample units)
// --------------------------------------------------------------------------------------
// FIRST: layer 0 of a scalar-input net WITHOUT a materialised causal layer.  h[t] = x[t-1] w0 + x[t] w1
// (modules.py:179-180) is a rank-2 function of two scalars per row, so instead of writing [rows, 64] floats in a
// front kernel and reading them back twice (x[t], x[t-d]), the lane rebuilds its 32 channels of both rows from four
// scalars with the same two fp32 operations per channel the front kernel uses (bit-identical): 4 B instead of 768 B of
// traffic per sample for this layer, and no front launch.
//
// HEAD: the LAST layer with the post-processing head (modules.py:145-165) fused behind it.  The gated output o never
// leaves the registers it was accumulated in -- it is the B operand of the skip GEMM -- so the [rows, 64] round trip
// through HBM between the last layer and the head (512 B per sample and net) and the head launch disappear.  LDS holds
// exactly the three weight matrices (filter|gate 64 KB + skip 32 KB + postprocess1 64 KB = all 160 KB of the CU): the
// small vectors (skip / postprocess1 biases, postprocess2) are read from global memory per unit like P, and units are
// handed out statically (no room for a counter).
//
// FOLD (with FIRST): h[t] = x[t-1] w0 + x[t] w1 makes the filter|gate convolution of layer 0 a [4 -> 128] map of the scalars
// x[t-d-1], x[t-d], x[t-1], x[t] (pwv_pack_first_fold_f16x3): ONE MFMA k-step (4 of its 16 k values used) instead of eight,
// no LDS fragment reads and no operand splits for it.  The same function, rounded differently; the persistent kernel's
// folded layer 0 (pwv_stack_persist.hip) performs exactly these operations, so the two stay bit-identical.
//
// STREAM (pwv_wavenet_layer_stream_f32; layer_f16x3_stream_kernel below): the chunk continues a session.  The look-back of a row with
// t < d comes from the session's history of this layer's input (StreamParams, pwv_layer_common.h) instead of zeros -- a fresh
// session's history IS zeros, the one-shot left edge -- and the rows the next chunk will look back at (t >= T - d: the unit's own
// rows, in registers) are stored to the session's next history.  Everything else is the same instructions in the same order, so
// the chunks of a stream concatenate to the one-shot forward bit for bit.  The body is text included into both kernels
// (pwv_layer_f16x3_body.inc): the non-streaming instantiations keep their names and their instruction streams.

template <bool SKIP, bool COND, bool GATED, bool FIRST = false, bool HEAD = false, bool FOLD = false>
__global__ __launch_bounds__(512) void layer_f16x3_kernel(const LayerParams p) {
    constexpr bool STREAM = false;
    const StreamParams st{};      // (not read)
#include "pwv_layer_f16x3_body.inc"
}

// the streaming forms: layer 0 folded (FIRST), the last layer + head (HEAD), else a plain residual layer
template <bool FIRST, bool HEAD>
__global__ __launch_bounds__(512) void layer_f16x3_stream_kernel(const LayerParams p, const StreamParams st) {
    constexpr bool STREAM = true, SKIP = false, COND = false, GATED = HEAD, FOLD = FIRST;
#include "pwv_layer_f16x3_body.inc"
}

// --------------------------------------------------------------------------------------
// head, split-fp16 arithmetic (8 waves = 2 per SIMD, dynamic 32-row units out of a contiguous per-workgroup
// range like the layer kernel; post2 stays an fp32 VALU dot)
// --------------------------------------------------------------------------------------
template <bool FROM_GATED>
__global__ __launch_bounds__(512) void head_f16x3_kernel(const HeadParams p) {
    constexpr int WAVES = 8;
    constexpr int kLds = head_floats(kMaxQ);
    __shared__ __attribute__((aligned(16))) float lds[kLds + 4];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = lane >> 5;
    const int net = blockIdx.x % p.G;
    const int wg = blockIdx.x / p.G;
    const int nwg = gridDim.x / p.G;
    const int Q = p.Q;
    int* unit_counter = reinterpret_cast<int*>(&lds[kLds]);
    if (tid == 0) *unit_counter = WAVES;
    fill_lds<head_floats(kMaxQ) / 4, 64 * WAVES>(lds, p.packed[net], tid);   // buffers are sized for kMaxQ
    __syncthreads();
    const f16x8* HAS = reinterpret_cast<const f16x8*>(&lds[kHAS]);
    const f16x8* HA1 = reinterpret_cast<const f16x8*>(&lds[kHA1]);
    auto no_extra = [](int) {};
    const int rows = p.N * p.T;
    const int units = (rows + 31) / 32;
    const int per_wg = (units + nwg - 1) / nwg;
    const int u_begin = wg * per_wg;
    const int u_end = (u_begin + per_wg < units) ? u_begin + per_wg : units;
    auto grab = [&]() -> int {
        int v = 0;
        if (lane == 0) v = __hip_atomic_fetch_add(unit_counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        return u_begin + __builtin_amdgcn_readfirstlane(v);
    };
    if (wave >= WAVES / 2) __builtin_amdgcn_s_setprio(1);
    for (int unit = u_begin + wave; unit < u_end; unit = grab()) {
        const int row = unit * 32 + (lane & 31);
        const bool valid = row < rows;
        const int rc = valid ? row : rows - 1;
        f32x16 accs[4];
        f16x8 ah[4], al[4];
        if constexpr (FROM_GATED) {
            f16x8 oh[4], ol[4];
            {
                float o[32];
                load_tiled<8, 64>(p.in[net], rc, h, true, o);
                split8<0>(o, oh[0], ol[0]);
                split8<8>(o, oh[1], ol[1]);
                split8<16>(o, oh[2], ol[2]);
                split8<24>(o, oh[3], ol[3]);
            }
#pragma unroll
            for (int it = 0; it < 4; ++it)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const f32x4 bs = *reinterpret_cast<const f32x4*>(&lds[kHBS + h * 64 + it * 16 + q * 4]);
#pragma unroll
                    for (int e = 0; e < 4; ++e) accs[it][q * 4 + e] = bs[e];
                }
            first_frags<4, 4, 0, 1, 4>(HAS, lane, ah, al);
            gemm16<4, 4, 0, 1, 4>(HAS, lane, accs, ah, al, [&](int s) -> f16x8 { return oh[s]; },
                                  [&](int s) -> f16x8 { return ol[s]; }, no_extra,
                                  [&](f16x8(&nh)[4], f16x8(&nl)[4]) { first_frags<8, 4, 0, 1, 4>(HA1, lane, nh, nl); });
        } else {
            const float* srow = p.in[net] + tile_off(rc, h, 128);
#pragma unroll
            for (int it = 0; it < 4; ++it)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(srow + (8 * it + 2 * q) * 128);
#pragma unroll
                    for (int e = 0; e < 4; ++e) accs[it][q * 4 + e] = v[e];
                }
            first_frags<8, 4, 0, 1, 4>(HA1, lane, ah, al);
        }
        // relu -> split -> post1 (128 -> 128)
        f16x8 sh[8], sl[8];
        {
            float r[64];
#pragma unroll
            for (int i = 0; i < 64; ++i) r[i] = fmaxf(accs[i >> 4][i & 15], 0.f);
            split8<0>(r, sh[0], sl[0]);
            split8<8>(r, sh[1], sl[1]);
            split8<16>(r, sh[2], sl[2]);
            split8<24>(r, sh[3], sl[3]);
            split8<32>(r, sh[4], sl[4]);
            split8<40>(r, sh[5], sl[5]);
            split8<48>(r, sh[6], sl[6]);
            split8<56>(r, sh[7], sl[7]);
        }
        f32x16 acc1[4];
#pragma unroll
        for (int it = 0; it < 4; ++it)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f32x4 b1 = *reinterpret_cast<const f32x4*>(&lds[kHB1 + h * 64 + it * 16 + q * 4]);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc1[it][q * 4 + e] = b1[e];
            }
        gemm16<8, 4, 0, 1, 4>(HA1, lane, acc1, ah, al, [&](int s) -> f16x8 { return sh[s]; },
                              [&](int s) -> f16x8 { return sl[s]; }, no_extra, [](f16x8(&)[4], f16x8(&)[4]) {});
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
// packing: TF layouts -> hi/lo fp16 A fragments (+ fp32 bias sections, same offsets as fp32 layout)
// --------------------------------------------------------------------------------------
__device__ __forceinline__ void put_split(f16x8* dst, int comp, const float (&w)[8]) {
    f16x8 v;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const _Float16 hi = (_Float16)w[q];
        v[q] = comp == 0 ? hi : (_Float16)(w[q] - (float)hi);
    }
    *dst = v;
}

// decode unit index within a [comp][NITTOT][NS][64] section
#define PWV_DECODE(u, NITTOT, NS)                                                     \
    const int lane = (u) & 63, s = ((u) >> 6) % (NS), it = ((u) >> 6) / (NS) % (NITTOT), \
              comp = ((u) >> 6) / ((NS) * (NITTOT));                                   \
    const int h = lane >> 5, i = lane & 31;                                          \
    (void)h; (void)i; (void)s; (void)it; (void)comp;

__global__ void pack_layer_f16_kernel(const float* filter, const float* gate, const float* dense, const float* dense_bias,
                                      const float* skip, const float* skip_bias, const float* gc_filter,
                                      const float* gc_gate, int with_skip, int cond_c, float* out, int total_units) {
    int u = blockIdx.x * blockDim.x + threadIdx.x;   // 16-byte units
    if (u >= total_units) return;
    f16x8* o16 = reinterpret_cast<f16x8*>(out);
    f32x4* o32 = reinterpret_cast<f32x4*>(out);
    float w[8];
    const int base = u;
    if (u < kA1Size / 4) {
        PWV_DECODE(u, 4, 8)
        const int tap = 1 - (s >> 2), oc = 32 * it + i;      // k-steps 0..3 = x[t] (tap 1), 4..7 = x[t-d] (tap 0): see the B operands
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int cin = 16 * (s & 3) + 8 * (q >> 2) + 4 * h + (q & 3);
            w[q] = oc < 64 ? kFScale * filter[(tap * 64 + cin) * 64 + oc] : kGScale * gate[(tap * 64 + cin) * 64 + oc - 64];
        }
        put_split(&o16[base], comp, w);
        return;
    }
    u -= kA1Size / 4;
    if (u < kA2Size / 4) {
        PWV_DECODE(u, 2, 4)
#pragma unroll
        for (int q = 0; q < 8; ++q) w[q] = dense[chan_of(s >> 1, 8 * (s & 1) + q, h) * 64 + 32 * it + i];
        put_split(&o16[base], comp, w);
        return;
    }
    u -= kA2Size / 4;
    if (u < kBDSize / 4) {
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = u * 4 + e, hh = j >> 5, it = (j >> 4) & 1, r = j & 15;
            v[e] = dense_bias ? dense_bias[chan_of(it, r, hh)] : 0.f;
        }
        o32[base] = v;
        return;
    }
    u -= kBDSize / 4;
    if (with_skip) {
        if (u < kASSize / 4) {
            PWV_DECODE(u, 4, 4)
#pragma unroll
            for (int q = 0; q < 8; ++q) w[q] = skip[chan_of(s >> 1, 8 * (s & 1) + q, h) * 128 + 32 * it + i];
            put_split(&o16[base], comp, w);
            return;
        }
        u -= kASSize / 4;
        if (u < kBSSize / 4) {
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int j = u * 4 + e, hh = j >> 6, it = (j >> 4) & 3, r = j & 15;
                v[e] = skip_bias ? skip_bias[chan_of(it, r, hh)] : 0.f;
            }
            o32[base] = v;
            return;
        }
        u -= kBSSize / 4;
    }
    if (cond_c > 0) {
        PWV_DECODE(u, 4, 5)
        const int oc = 32 * it + i;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int ci = 16 * s + 8 * (q >> 2) + 4 * h + (q & 3);
            w[q] = oc < 64 ? kFScale * gc_filter[ci * 64 + oc] : kGScale * gc_gate[ci * 64 + oc - 64];
        }
        put_split(&o16[base], comp, w);
    }
}

// pwv_pack_first_fold_f16x3: layer 0 of a scalar-input net, filter|gate folded onto the causal layer (modules.py:174-183 into
// :216-222).  h[t] = x[t-1] w0 + x[t] w1, so F|G(h[t-d], h[t]) = M [x[t-d-1], x[t-d], x[t-1], x[t]]^T with the [128, 4] matrix
// M[oc][2 tap + c] = sum_cin cf[c][cin] W[tap][cin][oc] (accumulated in fp64).  Output: the A fragments of ONE k-step,
// [hi | lo][4 row tiles][64 lanes] f16x8, k values 0..3 used (lanes with h = 0), the rest zero.
__global__ void pack_first_fold_f16_kernel(const float* __restrict__ cf, const float* __restrict__ filter, const float* __restrict__ gate,
                                           f16x8* __restrict__ out) {
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= 2 * 4 * 64) return;
    const int comp = u >> 8, it = (u >> 6) & 3, lane = u & 63, h = lane >> 5, i = lane & 31;
    const int oc = 32 * it + i;
    float w[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (h == 0) {
        for (int q = 0; q < 4; ++q) {
            const int tap = q >> 1, c = q & 1;
            double acc = 0.0;
            for (int cin = 0; cin < 64; ++cin) {
                const float wv = oc < 64 ? filter[(tap * 64 + cin) * 64 + oc] : gate[(tap * 64 + cin) * 64 + oc - 64];
                acc += (double)cf[c * 64 + cin] * (double)wv;
            }
            w[q] = (float)((double)(oc < 64 ? kFScale : kGScale) * acc);
        }
    }
    put_split(&out[u], comp, w);
}

__global__ void pack_head_f16_kernel(const float* skip, const float* skip_bias, const float* post1,
                                     const float* post1_bias, const float* post2, const float* post2_bias, int Q,
                                     float* out, int total_floats) {
    // units of 16 bytes up to kHW2, then plain floats (post2 / its bias)
    int u = blockIdx.x * blockDim.x + threadIdx.x;
    f16x8* o16 = reinterpret_cast<f16x8*>(out);
    f32x4* o32 = reinterpret_cast<f32x4*>(out);
    const int base = u;
    float w[8];
    if (u < kASSize / 4) {
        PWV_DECODE(u, 4, 4)
#pragma unroll
        for (int q = 0; q < 8; ++q) w[q] = skip ? skip[chan_of(s >> 1, 8 * (s & 1) + q, h) * 128 + 32 * it + i] : 0.f;
        put_split(&o16[base], comp, w);
        return;
    }
    u -= kASSize / 4;
    if (u < kBSSize / 4) {
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = u * 4 + e, hh = j >> 6, it = (j >> 4) & 3, r = j & 15;
            v[e] = skip_bias ? skip_bias[chan_of(it, r, hh)] : 0.f;
        }
        o32[base] = v;
        return;
    }
    u -= kBSSize / 4;
    if (u < kHA1Size / 4) {
        PWV_DECODE(u, 4, 8)
#pragma unroll
        for (int q = 0; q < 8; ++q) w[q] = post1[chan_of(s >> 1, 8 * (s & 1) + q, h) * 128 + 32 * it + i];
        put_split(&o16[base], comp, w);
        return;
    }
    u -= kHA1Size / 4;
    if (u < 128 / 4) {
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = u * 4 + e, hh = j >> 6, it = (j >> 4) & 3, r = j & 15;
            v[e] = post1_bias ? post1_bias[chan_of(it, r, hh)] : 0.f;
        }
        o32[base] = v;
        return;
    }
    u -= 128 / 4;
    // post2 [2 h][Q][64] floats then bias (padded to 4)
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int j = u * 4 + e;
        float x = 0.f;
        if (j < 2 * Q * 64) {
            const int c = j & 63, hq = j >> 6, q = hq % Q, hh = hq / Q;
            x = post2[chan_of(c >> 4, c & 15, hh) * Q + q];
        } else if (j - 2 * Q * 64 < Q && post2_bias) {
            x = post2_bias[j - 2 * Q * 64];
        }
        v[e] = x;
    }
    if (base * 4 < total_floats) o32[base] = v;
}

template <bool SKIP, bool COND, bool GATED, bool FIRST = false, bool HEAD = false, bool FOLD = false>
static int launch16(const LayerParams& lp, int grid, hipStream_t s) {
    hipLaunchKernelGGL((layer_f16x3_kernel<SKIP, COND, GATED, FIRST, HEAD, FOLD>), dim3(grid), dim3(512), 0, s, lp);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(PWV_EHIP, "f16x3 layer kernel launch failed: %s", hipGetErrorString(e));
    return PWV_OK;
}

int launch_layer_f16x3(const LayerParams& lp, bool skip, bool cond, bool gated, int per_net, hipStream_t s) {
    const int grid = per_net * lp.G;
    if (lp.packed_head[0]) {
        if (skip || cond || !gated || lp.x_first)
            return set_error(PWV_EINVAL, "fused head: plain last layer only (no skip accumulation, no per-sample condition, not layer 0)");
        return launch16<false, false, true, false, true>(lp, grid, s);
    }
    if (lp.x_first) {
        if (skip) return set_error(PWV_EINVAL, "x_first (layer 0 without a materialised causal layer) does not support skip accumulation");
        if (lp.fold0[0]) {      // layer 0 in its folded form
            if (cond) return gated ? launch16<false, true, true, true, false, true>(lp, grid, s) : launch16<false, true, false, true, false, true>(lp, grid, s);
            return gated ? launch16<false, false, true, true, false, true>(lp, grid, s) : launch16<false, false, false, true, false, true>(lp, grid, s);
        }
        if (cond) return gated ? launch16<false, true, true, true>(lp, grid, s) : launch16<false, true, false, true>(lp, grid, s);
        return gated ? launch16<false, false, true, true>(lp, grid, s) : launch16<false, false, false, true>(lp, grid, s);
    }
    if (skip) {
        if (cond) return gated ? launch16<true, true, true>(lp, grid, s) : launch16<true, true, false>(lp, grid, s);
        return gated ? launch16<true, false, true>(lp, grid, s) : launch16<true, false, false>(lp, grid, s);
    }
    if (cond) return gated ? launch16<false, true, true>(lp, grid, s) : launch16<false, true, false>(lp, grid, s);
    return gated ? launch16<false, false, true>(lp, grid, s) : launch16<false, false, false>(lp, grid, s);
}

int launch_layer_f16x3_stream(const LayerParams& lp, const StreamParams& st, int per_net, hipStream_t s) {
    const dim3 grid(per_net * lp.G);
    if (lp.packed_head[0]) hipLaunchKernelGGL((layer_f16x3_stream_kernel<false, true>), grid, dim3(512), 0, s, lp, st);
    else if (lp.x_first) hipLaunchKernelGGL((layer_f16x3_stream_kernel<true, false>), grid, dim3(512), 0, s, lp, st);
    else hipLaunchKernelGGL((layer_f16x3_stream_kernel<false, false>), grid, dim3(512), 0, s, lp, st);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(PWV_EHIP, "f16x3 streaming layer kernel launch failed: %s", hipGetErrorString(e));
    return PWV_OK;
}

int launch_head_f16x3(const HeadParams& hp, bool from_gated, int grid, hipStream_t s) {
    if (from_gated)
        hipLaunchKernelGGL((head_f16x3_kernel<true>), dim3(grid), dim3(512), 0, s, hp);
    else
        hipLaunchKernelGGL((head_f16x3_kernel<false>), dim3(grid), dim3(512), 0, s, hp);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(PWV_EHIP, "f16x3 head kernel launch failed: %s", hipGetErrorString(e));
    return PWV_OK;
}

int launch_pack_layer_f16x3(const float* filter, const float* gate, const float* dense, const float* dense_bias,
                            const float* skip, const float* skip_bias, const float* gc_filter, const float* gc_gate,
                            int with_skip, int cond_c, float* out, hipStream_t s) {
    const int units = layer_floats(with_skip != 0, cond_c > 0) / 4;
    hipLaunchKernelGGL(pack_layer_f16_kernel, dim3((units + 255) / 256), dim3(256), 0, s, filter, gate, dense,
                       dense_bias, skip, skip_bias, gc_filter, gc_gate, with_skip, cond_c, out, units);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(PWV_EHIP, "f16x3 pack launch failed: %s", hipGetErrorString(e));
    return PWV_OK;
}

int launch_pack_first_fold_f16x3(const float* cf, const float* filter, const float* gate, float* out, hipStream_t s) {
    hipLaunchKernelGGL(pack_first_fold_f16_kernel, dim3(2), dim3(256), 0, s, cf, filter, gate, reinterpret_cast<f16x8*>(out));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(PWV_EHIP, "first-fold pack launch failed: %s", hipGetErrorString(e));
    return PWV_OK;
}

int launch_pack_head_f16x3(const float* skip, const float* skip_bias, const float* post1, const float* post1_bias,
                           const float* post2, const float* post2_bias, int Q, float* out, hipStream_t s) {
    const int total = head_floats(Q);
    const int units = (total + 3) / 4;
    hipLaunchKernelGGL(pack_head_f16_kernel, dim3((units + 255) / 256), dim3(256), 0, s, skip, skip_bias, post1,
                       post1_bias, post2, post2_bias, Q, out, total);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(PWV_EHIP, "f16x3 pack launch failed: %s", hipGetErrorString(e));
    return PWV_OK;
}

}  // namespace pwv
