// Training on packed batches (include/pwv_hip_train_varlen.h; DESIGN.md section 9, "Packed training"): the unit bodies of
// pwv_train_units.h instantiated with the packed geometry policy -- utterance i owns rows cu_rows[i] .. cu_rows[i + 1] - 1, the tables
// are read on the device, and 33 threads locate the rows of a 32-row unit once per unit, into LDS.  The head, the reduction of the
// weight-gradient partials and the workspace are those of csrc/pwv_train.hip.  The packed loss head of the same header is in
// csrc/pwv_train_loss.hip, beside the uniform one.
#include "pwv_common.h"
#include "pwv_hip_train_varlen.h"
#include "pwv_train_units.h"

namespace pwv {

__global__ __launch_bounds__(kTrThreads) void train_front_fwd_varlen_kernel(FrontFwdParams p) { front_fwd_body<PackedGeo>(p); }

__global__ __launch_bounds__(kTrThreads) void train_layer_fwd_varlen_kernel(LayerFwdParams p) { layer_fwd_body<PackedGeo, ProjCond>(p, {}); }

template <bool LAST>
__global__ __launch_bounds__(kTrThreads) void train_layer_bwd_varlen_kernel(LayerBwdParams p) {
    layer_bwd_body<PackedGeo, ProjCond, LAST>(p, {});
}

__global__ __launch_bounds__(kTrThreads) void train_front_bwd_varlen_kernel(FrontBwdParams p) { front_bwd_body<PackedGeo>(p); }

// ------------------------------------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------------------------------------
static int varlen_check(const pwv_train_varlen_args* a, const char* who, Geom& g, PackedTables& tab, bool layer) {
    PWV_CHECK_ARG(a, "%s: args is NULL", who);
    PWV_CHECK_ARG(a->struct_size == sizeof(pwv_train_varlen_args), "%s: struct_size %zu is not sizeof(pwv_train_varlen_args) = %zu", who,
                  a->struct_size, sizeof(pwv_train_varlen_args));
    PWV_CHECK_ARG(a->cu_rows, "%s: cu_rows is a NULL pointer", who);
    PWV_CHECK_ARG(a->cu_frames, "%s: cu_frames is a NULL pointer", who);
    PWV_CHECK_ARG(a->n >= 1, "%s: n = %d must be >= 1", who, a->n);
    PWV_CHECK_ARG(a->rows >= a->n, "%s: rows = %d is below n = %d", who, a->rows, a->n);
    PWV_CHECK_ARG((long long)a->rows < (1ll << 31) - 64, "%s: rows = %d is beyond int32 (2^31 - 64)", who, a->rows);
    PWV_CHECK_ARG(a->proj_rows >= a->n, "%s: proj_rows = %d is below n = %d", who, a->proj_rows, a->n);
    PWV_CHECK_ARG(a->max_workgroups >= 0, "%s: max_workgroups %d is negative", who, a->max_workgroups);
    g.rows = a->rows;
    g.T = 0;
    g.d = a->dilation;
    g.dnext = a->next_dilation;
    g.hop = a->cond_hop;
    g.off = a->cond_offset;
    g.frames = 0;
    g.pstride = a->proj_row_stride;
    g.dpstride = a->d_proj_row_stride;
    g.kmax = (a->cond_hop + 30) / 32 + 1;
    tab.cu_rows = a->cu_rows;
    tab.cu_frames = a->cu_frames;
    tab.n = a->n;
    tab.prows = a->proj_rows;
    // (every entry point locates with the conditioning geometry: the front too, whose P rows nobody reads)
    PWV_CHECK_ARG(a->cond_hop >= 1 && a->cond_offset >= 0, "%s: cond_hop %d, cond_offset %d", who, a->cond_hop, a->cond_offset);
    PWV_CHECK_ARG((long long)a->rows + a->cond_offset < (1ll << 31), "%s: cond_offset %d is beyond int32 with rows = %d", who, a->cond_offset, a->rows);
    if (layer) {
        PWV_CHECK_ARG(a->dilation >= 1, "%s: dilation %d must be >= 1", who, a->dilation);
        PWV_CHECK_ARG(a->proj_row_stride >= 128, "%s: proj_row_stride %d is below 128", who, a->proj_row_stride);
    }
    return PWV_OK;
}

}  // namespace pwv

using namespace pwv;

extern "C" int pwv_train_varlen_front_fwd_f32(const pwv_train_varlen_args* a, pwv_stream_t stream) {
    const char* who = "pwv_train_varlen_front_fwd_f32";
    Geom g;
    PackedTables tab;
    if (int e = varlen_check(a, who, g, tab, false)) return e;
    return train_front_fwd(a, who, g, tab, [&](int grid, const FrontFwdParams& p) {
        hipLaunchKernelGGL(train_front_fwd_varlen_kernel, dim3(grid), dim3(kTrThreads), 0, (hipStream_t)stream, p);
    });
}

extern "C" int pwv_train_varlen_layer_fwd_f32(const pwv_train_varlen_args* a, pwv_stream_t stream) {
    const char* who = "pwv_train_varlen_layer_fwd_f32";
    Geom g;
    PackedTables tab;
    if (int e = varlen_check(a, who, g, tab, true)) return e;
    return train_layer_fwd<ProjCond>(a, who, g, tab, [&](int grid, const LayerFwdParams& p) {
        hipLaunchKernelGGL(train_layer_fwd_varlen_kernel, dim3(grid), dim3(kTrThreads), 0, (hipStream_t)stream, p);
    });
}

extern "C" int pwv_train_varlen_layer_bwd_f32(const pwv_train_varlen_args* a, pwv_stream_t stream) {
    const char* who = "pwv_train_varlen_layer_bwd_f32";
    Geom g;
    PackedTables tab;
    if (int e = varlen_check(a, who, g, tab, true)) return e;
    return train_layer_bwd<ProjCond>(a, who, g, tab, {}, nullptr, 0, (hipStream_t)stream, [&](bool last, int grid, const LayerBwdParams& p) {
        if (last) hipLaunchKernelGGL(train_layer_bwd_varlen_kernel<true>, dim3(grid), dim3(kTrThreads), 0, (hipStream_t)stream, p);
        else hipLaunchKernelGGL(train_layer_bwd_varlen_kernel<false>, dim3(grid), dim3(kTrThreads), 0, (hipStream_t)stream, p);
    });
}

extern "C" int pwv_train_varlen_front_bwd_f32(const pwv_train_varlen_args* a, pwv_stream_t stream) {
    const char* who = "pwv_train_varlen_front_bwd_f32";
    Geom g;
    PackedTables tab;
    if (int e = varlen_check(a, who, g, tab, false)) return e;
    return train_front_bwd(a, who, g, tab, (hipStream_t)stream, [&](int grid, const FrontBwdParams& p) {
        hipLaunchKernelGGL(train_front_bwd_varlen_kernel, dim3(grid), dim3(kTrThreads), 0, (hipStream_t)stream, p);
    });
}
