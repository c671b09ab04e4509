// Streaming layer kernels with a PER-SAMPLE condition (include/pwv_hip_stream_cond.h; DESIGN.md section 9, "Streaming transposed-conv
// conditioning"): the streaming forms of pwv_layer.hip / pwv_layer_f16.hip for models whose condition is upsampled by transposed
// convolutions (the reference's models.py:109-124) and enters every layer as a 1x1 product c[t] [gc_filter | gc_gate].
//
// The condition of a row needs no history -- row t of a chunk reads row t of the chunk's condition -- so these are the one-shot COND
// kernels (layer_*_kernel<false, true, ...>) with the look-back of the streaming ones: the same body text (pwv_layer_f32_body.inc,
// pwv_layer_f16x3_body.inc) instantiated with STREAM = COND = true.  Every row goes through the one-shot kernels' instructions in
// their order, so the chunks of a stream concatenate to the one-shot forward bit for bit.
//
// Three forms per arithmetic: layer 0 folded onto its scalar input (FIRST), a plain residual layer, and the LAST layer with gated
// output (LAST).  The fused head has no room for the condition weights -- filter|gate + skip + postprocess1 fill the 160 KB of LDS, and
// gc_filter|gc_gate are 40 KB more -- so the head runs as the ordinary launch behind the last layer (pwv_wavenet_head_f32,
// PWV_HEAD_IN_GATED): it is row-local and needs no streaming form.
#include "pwv_f16x3.h"
#include "pwv_layer_f32_tile.h"
#include "pwv_hip_stream_cond.h"

namespace pwv {

template <bool FIRST, bool LAST>
__global__ __launch_bounds__(512) void layer_f32_stream_cond_kernel(const LayerParams p, const StreamParams st) {
    constexpr bool STREAM = true, SKIP = false, COND = true, GATED = LAST, HEAD = false, FOLD = FIRST;
#include "pwv_layer_f32_body.inc"
}

template <bool FIRST, bool LAST>
__global__ __launch_bounds__(512) void layer_f16x3_stream_cond_kernel(const LayerParams p, const StreamParams st) {
    constexpr bool STREAM = true, SKIP = false, COND = true, GATED = LAST, HEAD = false, FOLD = FIRST;
#include "pwv_layer_f16x3_body.inc"
}

// (layer_call of pwv_layer.hip has built `lp` and the grid; pwv_wavenet_layer_stream_cond_f32 has checked the form)
int launch_layer_stream_cond(const LayerParams& lp, const StreamParams& st, bool f16x3, bool gated, int per_net, hipStream_t s) {
    const dim3 grid(per_net * lp.G), block(512);
    if (f16x3) {
        if (lp.x_first) hipLaunchKernelGGL((layer_f16x3_stream_cond_kernel<true, false>), grid, block, 0, s, lp, st);
        else if (gated) hipLaunchKernelGGL((layer_f16x3_stream_cond_kernel<false, true>), grid, block, 0, s, lp, st);
        else hipLaunchKernelGGL((layer_f16x3_stream_cond_kernel<false, false>), grid, block, 0, s, lp, st);
    } else {
        if (lp.x_first) hipLaunchKernelGGL((layer_f32_stream_cond_kernel<true, false>), grid, block, 0, s, lp, st);
        else if (gated) hipLaunchKernelGGL((layer_f32_stream_cond_kernel<false, true>), grid, block, 0, s, lp, st);
        else hipLaunchKernelGGL((layer_f32_stream_cond_kernel<false, false>), grid, block, 0, s, lp, st);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(PWV_EHIP, "streaming per-sample layer kernel launch failed: %s", hipGetErrorString(e));
    return PWV_OK;
}

}  // namespace pwv

using namespace pwv;

extern "C" int pwv_wavenet_layer_stream_cond_f32(const pwv_layer_args* a, const pwv_stream_args* sa, pwv_stream_t stream) {
    static const char* const me = "pwv_wavenet_layer_stream_cond_f32";
    PWV_CHECK_ARG(a, "%s: args is NULL", me);
    pwv_stream_args v;
    StreamParams st{};
    const char* why = stream_args_view(sa, v, st);      // struct_size, NULL history / slot table, block_stride
    PWV_CHECK_ARG(!why, "%s: %s", me, why);
    PWV_CHECK_ARG(!v.cu_rows, "%s: hist->cu_rows is set: the per-layer kernels have no packed form", me);
    PWV_CHECK_ARG(a->precision == PWV_PREC_F32 || a->precision == PWV_PREC_F16X3,
                  "%s: PWV_PREC_F32 / PWV_PREC_F16X3 only (the fp16 storage mode has no streaming form)", me);
    PWV_CHECK_ARG(a->G >= 1 && a->G <= PWV_MAX_NETS && a->dilation >= 1 && a->T >= 1 && a->N >= 1, "%s: bad G / dilation / N / T", me);
    PWV_CHECK_ARG(a->cond, "%s: cond is NULL: this entry streams a per-sample condition (pwv_wavenet_layer_stream_f32 streams without one)", me);
    PWV_CHECK_ARG(a->cond_channels == kCondC, "%s: per-sample conditioning supports %d channels, got %d", me, kCondC, a->cond_channels);
    const long long hist_rows = ((long long)a->dilation + 31) / 32 * 32;
    for (int g = 0; g < a->G; ++g) {
        PWV_CHECK_ARG(!a->skip[g], "%s: skip accumulation has no streaming form", me);
        PWV_CHECK_ARG(!a->head_packed[g], "%s: no fused head with a per-sample condition (its weights leave no LDS for gc_filter|gc_gate): "
                      "out_mode PWV_OUT_GATED, then pwv_wavenet_head_f32", me);
        PWV_CHECK_ARG(!a->x_first || a->first_fold[g], "%s: layer 0 streams in its folded form only (first_fold)", me);
        PWV_CHECK_ARG(a->x_first || (v.row_off[g] % 4 == 0 && v.row_off[g] + (size_t)hist_rows * 64 <= v.block_stride),
                      "%s: row_off[%d] + round32(dilation) rows leave the history block", me, g);
        for (int o = 0; o < g && !a->x_first; ++o)
            PWV_CHECK_ARG(v.row_off[o] + (size_t)hist_rows * 64 <= v.row_off[g] || v.row_off[g] + (size_t)hist_rows * 64 <= v.row_off[o],
                          "%s: the nets' row histories overlap", me);
    }
    PWV_CHECK_ARG(!a->x_first || v.scalar_off + (size_t)a->dilation + 1 <= v.block_stride,
                  "%s: scalar_off + dilation + 1 scalars leave the history block", me);
    PWV_CHECK_ARG(a->out_mode == PWV_OUT_RESIDUAL || (a->out_mode == PWV_OUT_GATED && !a->x_first),
                  "%s: out_mode is PWV_OUT_RESIDUAL, or PWV_OUT_GATED for a last layer that is not layer 0", me);
    return layer_call_stream(a, st, stream);
}
