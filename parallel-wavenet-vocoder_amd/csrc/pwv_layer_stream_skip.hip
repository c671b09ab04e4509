// Streaming layer kernels with SKIP ACCUMULATION (include/pwv_hip_stream_skip.h; DESIGN.md section 9, "Streaming the skip-connection
// architecture"): the streaming forms of pwv_layer.hip / pwv_layer_f16.hip for models with model.use_skip_connection (the reference's
// modules.py:142-147, :243-250), whose head reads the sum over all layers of o_j @ skip_j + skip_bias_j instead of the last layer's o.
//
// The skip sum of a row is a function of that row's gated outputs alone, so it needs no history: these are the one-shot SKIP kernels
// (layer_*_kernel<true, false, GATED>) with the look-back of the streaming ones -- the same body text (pwv_layer_f32_body.inc,
// pwv_layer_f16x3_body.inc) instantiated with STREAM = SKIP = true.  Every row goes through the one-shot kernels' instructions in
// their order, the accumulator of a chunk is read and written in layer order exactly as the one-shot's (no atomics), so the chunks of a
// stream concatenate to the one-shot forward bit for bit.
//
// Two forms per arithmetic: a residual layer, and the LAST layer with gated output (which the skip architecture never reads: the
// one-shot stack runs it as out_mode PWV_OUT_GATED too, and so its skip contribution has the same bits).  Layer 0 is a residual layer
// like any other: the one-shot forward of a skip model never rebuilds the causal layer inside layer 0 (neither unfolded nor folded),
// it reads the rows pwv_iaf_front_f32 wrote -- and so does the stream, from stream_front_kernel below, which is that front with
// x[-1] taken from the session's scalar history instead of zero.  Layer 0's look-back is then a row history of h like every other
// layer's.  The head is the ordinary launch (pwv_wavenet_head_f32, PWV_HEAD_IN_SKIPSUM) on the chunk's accumulator: row-local.
#include "pwv_f16x3.h"
#include "pwv_layer_f32_tile.h"
#include "pwv_hip_stream_skip.h"

namespace pwv {

template <bool LAST>
__global__ __launch_bounds__(512) void layer_f32_stream_skip_kernel(const LayerParams p, const StreamParams st) {
    constexpr bool STREAM = true, SKIP = true, COND = false, GATED = LAST, HEAD = false, FIRST = false, FOLD = false;
#include "pwv_layer_f32_body.inc"
}

template <bool LAST>
__global__ __launch_bounds__(512) void layer_f16x3_stream_skip_kernel(const LayerParams p, const StreamParams st) {
    constexpr bool STREAM = true, SKIP = true, COND = false, GATED = LAST, HEAD = false, FIRST = false, FOLD = false;
#include "pwv_layer_f16x3_body.inc"
}

// pwv_iaf_front_stream_f32: iaf_front_kernel (pwv_misc.hip) at W = 2, R = 64 on a chunk -- one thread per row (blockIdx.y = net),
// h[t] = fma(x[t], w1, fma(x[t-1], w0, 0)), the front's own operations in its order -- with x[-1] of a session read from its scalar
// history (one float at scalar_off; zero for a fresh session: the one-shot left edge) and the chunk's last sample stored as the next.
struct StreamFrontParams {
    const float* x;
    const float* filt[PWV_MAX_NETS];
    float* h[PWV_MAX_NETS];
    int N, T;
};

__global__ __launch_bounds__(256) void stream_front_kernel(const StreamFrontParams p, const StreamParams st) {
    __shared__ __attribute__((aligned(16))) float fl[128];
    const int g = blockIdx.y;
    if (threadIdx.x < 128) fl[threadIdx.x] = p.filt[g][threadIdx.x];
    __syncthreads();
    const unsigned rows = (unsigned)p.N * (unsigned)p.T;
    const unsigned row = blockIdx.x * 256u + threadIdx.x;
    if (row >= rows) return;
    const unsigned n = row / (unsigned)p.T, t = row - n * (unsigned)p.T;
    const int2 blk = reinterpret_cast<const int2*>(st.slot_tab)[n];
    const float xcur = p.x[row];
    const float xprev = t ? p.x[row - 1] : st.hist_rd[(long long)blk.x * st.block_stride + st.scalar_off];
    if (g == 0 && t + 1 == (unsigned)p.T) st.hist_wr[(long long)blk.y * st.block_stride + st.scalar_off] = xcur;
    float* out = p.h[g] + (size_t)(row >> 5) * (32u * 64u) + (row & 31u) * 4u;
    for (int q = 0; q < 16; ++q) {
        const f32x4 w0 = *reinterpret_cast<const f32x4*>(&fl[4 * q]);
        const f32x4 w1 = *reinterpret_cast<const f32x4*>(&fl[64 + 4 * q]);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = fmaf(xprev, w0[e], acc[e]);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = fmaf(xcur, w1[e], acc[e]);
        *reinterpret_cast<f32x4*>(out + q * 128) = acc;
    }
}

// (layer_call of pwv_layer.hip has built `lp` and the grid; pwv_wavenet_layer_stream_skip_f32 has checked the form)
int launch_layer_stream_skip(const LayerParams& lp, const StreamParams& st, bool f16x3, bool gated, int per_net, hipStream_t s) {
    const dim3 grid(per_net * lp.G), block(512);
    if (f16x3) {
        if (gated) hipLaunchKernelGGL((layer_f16x3_stream_skip_kernel<true>), grid, block, 0, s, lp, st);
        else hipLaunchKernelGGL((layer_f16x3_stream_skip_kernel<false>), grid, block, 0, s, lp, st);
    } else {
        if (gated) hipLaunchKernelGGL((layer_f32_stream_skip_kernel<true>), grid, block, 0, s, lp, st);
        else hipLaunchKernelGGL((layer_f32_stream_skip_kernel<false>), grid, block, 0, s, lp, st);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(PWV_EHIP, "streaming skip layer kernel launch failed: %s", hipGetErrorString(e));
    return PWV_OK;
}

}  // namespace pwv

using namespace pwv;

extern "C" int pwv_wavenet_layer_stream_skip_f32(const pwv_layer_args* a, const pwv_stream_args* sa, pwv_stream_t stream) {
    static const char* const me = "pwv_wavenet_layer_stream_skip_f32";
    PWV_CHECK_ARG(a, "%s: args is NULL", me);
    pwv_stream_args v;
    StreamParams st{};
    const char* why = stream_args_view(sa, v, st);      // struct_size, NULL history / slot table, block_stride
    PWV_CHECK_ARG(!why, "%s: %s", me, why);
    PWV_CHECK_ARG(!v.cu_rows, "%s: hist->cu_rows is set: the per-layer kernels have no packed form", me);
    PWV_CHECK_ARG(a->precision == PWV_PREC_F32 || a->precision == PWV_PREC_F16X3,
                  "%s: PWV_PREC_F32 / PWV_PREC_F16X3 only (the fp16 storage mode has no streaming form and no skip accumulation)", me);
    PWV_CHECK_ARG(a->G >= 1 && a->G <= PWV_MAX_NETS && a->dilation >= 1 && a->T >= 1 && a->N >= 1, "%s: bad G / dilation / N / T", me);
    PWV_CHECK_ARG(!a->cond && a->cond_channels == 0, "%s: a per-sample condition (cond / cond_channels) together with skip accumulation has no streaming form", me);
    PWV_CHECK_ARG(!a->x_first, "%s: x_first is set: layer 0 of a skip stream is a plain layer on the rows of pwv_iaf_front_stream_f32 "
                  "(the one-shot skip forward never rebuilds the causal layer inside layer 0)", me);
    const long long hist_rows = ((long long)a->dilation + 31) / 32 * 32;
    for (int g = 0; g < a->G; ++g) {
        PWV_CHECK_ARG(a->skip[g], "%s: skip[%d] is NULL: this entry streams with skip accumulation (pwv_wavenet_layer_stream_f32 streams without)", me, g);
        PWV_CHECK_ARG(!a->head_packed[g], "%s: no fused head with skip accumulation (head_packed): the head reads the finished skip sum, "
                      "pwv_wavenet_head_f32 with PWV_HEAD_IN_SKIPSUM", me);
        PWV_CHECK_ARG(!a->first_fold[g], "%s: first_fold is set: layer 0 has no folded form here (it would not round as the one-shot skip forward does)", me);
        PWV_CHECK_ARG(v.row_off[g] % 4 == 0 && v.row_off[g] + (size_t)hist_rows * 64 <= v.block_stride,
                      "%s: row_off[%d] + round32(dilation) rows leave the history block", me, g);
        for (int o = 0; o < g; ++o)
            PWV_CHECK_ARG(v.row_off[o] + (size_t)hist_rows * 64 <= v.row_off[g] || v.row_off[g] + (size_t)hist_rows * 64 <= v.row_off[o],
                          "%s: the nets' row histories overlap", me);
    }
    PWV_CHECK_ARG(a->out_mode == PWV_OUT_RESIDUAL || a->out_mode == PWV_OUT_GATED, "%s: bad out_mode", me);
    return layer_call_stream(a, st, stream);
}

extern "C" int pwv_iaf_front_stream_f32(const float* x, int G, const float* const* filt, float* const* h, int N, int T,
                                        const pwv_stream_args* sa, pwv_stream_t stream) {
    static const char* const me = "pwv_iaf_front_stream_f32";
    PWV_CHECK_ARG(x && filt && h, "%s: NULL pointer", me);
    pwv_stream_args v;
    StreamParams st{};
    const char* why = stream_args_view(sa, v, st);
    PWV_CHECK_ARG(!why, "%s: %s", me, why);
    PWV_CHECK_ARG(!v.cu_rows, "%s: hist->cu_rows is set: no packed form", me);
    PWV_CHECK_ARG(G >= 1 && G <= PWV_MAX_NETS && N >= 1 && T >= 1, "%s: bad G / N / T", me);
    PWV_CHECK_ARG((long long)N * T < (1ll << 31) - 256, "%s: N*T too large", me);
    PWV_CHECK_ARG(v.scalar_off + 1 <= v.block_stride, "%s: scalar_off + 1 scalar leaves the history block", me);
    StreamFrontParams p{};
    p.x = x;
    p.N = N;
    p.T = T;
    for (int g = 0; g < G; ++g) {
        PWV_CHECK_ARG(filt[g] && h[g], "%s: NULL filter / output for net %d", me, g);
        p.filt[g] = filt[g];
        p.h[g] = h[g];
    }
    hipLaunchKernelGGL(stream_front_kernel, dim3((unsigned)(((long long)N * T + 255) / 256), G), dim3(256), 0, (hipStream_t)stream, p, st);
    PWV_CHECK_HIP(hipGetLastError());
    return PWV_OK;
}
