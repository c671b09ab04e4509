// Training the skip-connection architecture (include/pwv_hip_train_skip.h; DESIGN.md section 9, "Training the skip-connection
// architecture"): the head of a net reads S = sum_j (o_j skip_j + skip_bias_j) over ALL layers.  The layer kernels are the bodies of
// pwv_train_units.h instantiated with the skip policy SumSkip, over the uniform and the packed geometry: the forward adds the unit's
// o skip + skip_bias to S (tile32, 128 channels), the backward stages the unit's dS rows, adds dS skip^T to d o and accumulates
// d skip = o^T dS in registers.  The head kernels are the one-output instances of csrc/pwv_train_head.h over its input policy SumIn:
// they begin at S and end at dS and its column sums (every layer's d skip_bias).  The reduction of the partials is train_reduce_kernel's.
#include "pwv_common.h"
#include "pwv_hip_train_skip.h"
#include "pwv_train_head.h"

namespace pwv {

constexpr int kSkipLayerPart = kLayerPart + SumSkip::kPartFloats;             // dWfg | d dense | d dense_bias | d skip
constexpr int kSkipMaxPart = kSkipLayerPart > kMaxPart ? kSkipLayerPart : kMaxPart;

template <class Geo>
__global__ __launch_bounds__(kTrThreads) void train_skip_layer_fwd_kernel(LayerFwdParams p, SkipParams sp) {
    layer_fwd_body<Geo, ProjCond, SumSkip>(p, {}, sp);
}

// Seven accumulator tiles stay in registers over a workgroup's units (dWfg 4, d dense 1, d skip 2) and the unit's arrays take
// 66304 bytes of LDS (the dS tile stays resident beside the layer's own): two workgroups share a compute unit, as the default grid
// assumes, and the second launch bound holds the kernel to the 256 registers per lane that takes
template <class Geo, bool LAST>
__global__ __launch_bounds__(kTrThreads, 2) void train_skip_layer_bwd_kernel(LayerBwdParams p, SkipParams sp) {
    layer_bwd_body<Geo, ProjCond, LAST, SumSkip>(p, {}, sp);
}

__global__ __launch_bounds__(kTrThreads) void train_skip_head_fwd_kernel(HeadParams p) { head_fwd_body<SumIn, 1>(p); }

__global__ __launch_bounds__(kTrThreads) void train_skip_head_bwd_kernel(HeadParams p) { head_bwd_body<SumIn, 1>(p); }

// ------------------------------------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------------------------------------
// what every entry point checks first: the struct and the batch, uniform or packed; `layer`: the conditioning geometry too
static int skip_check(const pwv_train_skip_args* s, const char* who, bool layer, Geom& g, PackedTables& tab) {
    PWV_CHECK_ARG(s, "%s: args is NULL", who);
    const pwv_train_args* a = &s->train;
    g = Geom{};
    tab = PackedTables{};
    if (s->cu_rows) {
        PWV_CHECK_ARG(a->struct_size == sizeof(pwv_train_skip_args), "%s: train.struct_size %zu is not sizeof(pwv_train_skip_args) = %zu", who,
                      a->struct_size, sizeof(pwv_train_skip_args));
        PWV_CHECK_ARG(s->n >= 1, "%s: n = %d must be >= 1", who, s->n);
        PWV_CHECK_ARG(s->rows >= s->n, "%s: rows = %d is below n = %d", who, s->rows, s->n);
        PWV_CHECK_ARG((long long)s->rows < (1ll << 31) - 64, "%s: rows = %d is beyond int32 (2^31 - 64)", who, s->rows);
        PWV_CHECK_ARG(a->max_workgroups >= 0, "%s: max_workgroups %d is negative", who, a->max_workgroups);
        g.rows = s->rows;
        if (layer) {
            PWV_CHECK_ARG(s->cu_frames, "%s: cu_frames is a NULL pointer", who);
            PWV_CHECK_ARG(s->proj_rows >= s->n, "%s: proj_rows = %d is below n = %d", who, s->proj_rows, s->n);
            PWV_CHECK_ARG(a->cond_hop >= 1 && a->cond_offset >= 0, "%s: cond_hop %d, cond_offset %d", who, a->cond_hop, a->cond_offset);
            PWV_CHECK_ARG((long long)s->rows + a->cond_offset < (1ll << 31), "%s: cond_offset %d is beyond int32 with rows = %d", who,
                          a->cond_offset, s->rows);
            tab.cu_rows = s->cu_rows;
            tab.cu_frames = s->cu_frames;
            tab.n = s->n;
            tab.prows = s->proj_rows;
        }
    } else {
        if (int e = train_check_batch(a, who, "train.struct_size", sizeof(pwv_train_skip_args), "pwv_train_skip_args")) return e;
        g.rows = a->N * a->T;
        g.T = a->T;
        g.frames = a->cond_frames;
        if (layer) {
            PWV_CHECK_ARG(a->cond_hop >= 1 && a->cond_offset >= 0 && a->cond_frames >= 1, "%s: cond_hop %d, cond_offset %d, cond_frames %d", who,
                          a->cond_hop, a->cond_offset, a->cond_frames);
            PWV_CHECK_ARG((a->T - 1 + a->cond_offset) / a->cond_hop < a->cond_frames, "%s: cond_frames %d is short of the frames T = %d needs", who,
                          a->cond_frames, a->T);
        }
    }
    if (layer) {
        PWV_CHECK_ARG(a->dilation >= 1, "%s: dilation %d must be >= 1", who, a->dilation);
        PWV_CHECK_ARG(a->proj_row_stride >= 128, "%s: proj_row_stride %d is below 128", who, a->proj_row_stride);
        g.d = a->dilation;
        g.dnext = a->next_dilation;
        g.hop = a->cond_hop;
        g.off = a->cond_offset;
        g.pstride = a->proj_row_stride;
        g.dpstride = a->d_proj_row_stride;
        g.kmax = (a->cond_hop + 30) / 32 + 1;
    }
    return PWV_OK;
}

static int skip_check_ws(const pwv_train_args* a, const char* who, int grid) {
    PWV_CHECK_ARG(a->workspace, "%s: workspace is a NULL pointer", who);
    PWV_CHECK_ARG(a->workspace_bytes >= (size_t)grid * kSkipMaxPart * sizeof(float),
                  "%s: workspace_bytes %zu is short of the %zu pwv_train_skip_workspace_bytes gives", who, a->workspace_bytes,
                  (size_t)grid * kSkipMaxPart * sizeof(float));
    return PWV_OK;
}

static int skip_head_check(const pwv_train_skip_args* s, const char* who, Geom& g) {
    PackedTables tab;
    if (int e = skip_check(s, who, false, g, tab)) return e;
    PWV_CHECK_ARG(s->skip_sum, "%s: skip_sum is a NULL pointer", who);
    PWV_CHECK_ARG(s->train.post1 && s->train.post2, "%s: post1 or post2 is a NULL pointer", who);
    return PWV_OK;
}

}  // namespace pwv

using namespace pwv;

extern "C" size_t pwv_train_skip_workspace_bytes(const pwv_train_skip_args* s) {
    Geom g;
    PackedTables tab;
    if (skip_check(s, "pwv_train_skip_workspace_bytes", false, g, tab) != PWV_OK) return 0;
    return (size_t)train_grid_size(s->train.max_workgroups, (g.rows + 31) / 32) * kSkipMaxPart * sizeof(float);
}

extern "C" int pwv_train_skip_layer_fwd_f32(const pwv_train_skip_args* s, pwv_stream_t stream) {
    const char* who = "pwv_train_skip_layer_fwd_f32";
    Geom g;
    PackedTables tab;
    if (int e = skip_check(s, who, true, g, tab)) return e;
    const pwv_train_args* a = &s->train;
    PWV_CHECK_ARG(a->form == PWV_TRAIN_RESIDUAL || a->form == PWV_TRAIN_LAST, "%s: form %d", who, a->form);
    const bool last = a->form == PWV_TRAIN_LAST;
    PWV_CHECK_ARG(a->x && a->filter && a->gate && a->proj, "%s: x, filter, gate or proj is a NULL pointer", who);
    PWV_CHECK_ARG(a->skip, "%s: train.skip is a NULL pointer", who);
    PWV_CHECK_ARG(s->skip_sum, "%s: skip_sum is a NULL pointer", who);
    PWV_CHECK_ARG(last || (a->dense && a->x_out), "%s: dense or x_out is a NULL pointer", who);
    LayerFwdParams p{};
    p.x = a->x; p.proj = a->proj; p.filter = a->filter; p.gate = a->gate; p.dense = a->dense; p.dense_bias = a->dense_bias;
    p.x_out = a->x_out;
    p.g = g;
    p.last = last;
    p.tab = tab;
    const SkipParams sp{a->skip, a->skip_bias, s->skip_sum, nullptr, s->skip_accumulate != 0};
    const dim3 grid(train_grid_size(a->max_workgroups, (g.rows + 31) / 32));
    if (s->cu_rows) hipLaunchKernelGGL(train_skip_layer_fwd_kernel<PackedGeo>, grid, dim3(kTrThreads), 0, (hipStream_t)stream, p, sp);
    else hipLaunchKernelGGL(train_skip_layer_fwd_kernel<UniformGeo>, grid, dim3(kTrThreads), 0, (hipStream_t)stream, p, sp);
    PWV_CHECK_HIP(hipGetLastError());
    return PWV_OK;
}

extern "C" int pwv_train_skip_head_fwd_f32(const pwv_train_skip_args* s, pwv_stream_t stream) {
    const char* who = "pwv_train_skip_head_fwd_f32";
    Geom g;
    if (int e = skip_head_check(s, who, g)) return e;
    PWV_CHECK_ARG(s->train.y, "%s: y is a NULL pointer", who);
    const int grid = train_grid_size(s->train.max_workgroups, (g.rows + 31) / 32);
    return head_fwd_launch(train_skip_head_fwd_kernel, head_params(&s->train, g.rows, s->skip_sum), grid, (hipStream_t)stream);
}

extern "C" int pwv_train_skip_head_bwd_f32(const pwv_train_skip_args* s, pwv_stream_t stream) {
    const char* who = "pwv_train_skip_head_bwd_f32";
    Geom g;
    if (int e = skip_head_check(s, who, g)) return e;
    const pwv_train_args* a = &s->train;
    PWV_CHECK_ARG(a->d_out, "%s: d_out is a NULL pointer", who);
    PWV_CHECK_ARG(s->d_skip_sum_out, "%s: d_skip_sum_out is a NULL pointer", who);
    const int grid = train_grid_size(a->max_workgroups, (g.rows + 31) / 32);
    if (int e = skip_check_ws(a, who, grid)) return e;
    const HeadParams p = head_params(a, g.rows, s->skip_sum, s->d_skip_sum_out);
    return head_bwd_launch_and_reduce<SumIn, 1>(train_skip_head_bwd_kernel, p, grid, a, s->d_skip_bias, (hipStream_t)stream);
}

extern "C" int pwv_train_skip_layer_bwd_f32(const pwv_train_skip_args* s, pwv_stream_t stream) {
    const char* who = "pwv_train_skip_layer_bwd_f32";
    Geom g;
    PackedTables tab;
    if (int e = skip_check(s, who, true, g, tab)) return e;
    const pwv_train_args* a = &s->train;
    PWV_CHECK_ARG(a->form == PWV_TRAIN_RESIDUAL || a->form == PWV_TRAIN_LAST, "%s: form %d", who, a->form);
    const bool last = a->form == PWV_TRAIN_LAST;
    PWV_CHECK_ARG(a->x && a->filter && a->gate, "%s: x, filter or gate is a NULL pointer", who);
    PWV_CHECK_ARG(a->u && a->v && a->d_filter && a->d_gate, "%s: u, v, d_filter or d_gate is a NULL pointer", who);
    PWV_CHECK_ARG(a->proj && a->d_proj, "%s: proj or d_proj is a NULL pointer", who);
    PWV_CHECK_ARG(a->d_proj_row_stride >= 128, "%s: d_proj_row_stride %d is below 128", who, a->d_proj_row_stride);
    PWV_CHECK_ARG(a->skip, "%s: train.skip is a NULL pointer", who);
    PWV_CHECK_ARG(s->d_skip_sum, "%s: d_skip_sum is a NULL pointer", who);
    PWV_CHECK_ARG(s->d_skip, "%s: d_skip is a NULL pointer", who);
    if (!last) {
        PWV_CHECK_ARG(a->dense && a->u_next && a->v_next && a->d_dense, "%s: dense, u_next, v_next or d_dense is a NULL pointer", who);
        PWV_CHECK_ARG(a->next_dilation >= 1, "%s: next_dilation %d must be >= 1", who, a->next_dilation);
        PWV_CHECK_ARG(a->u != a->u_next && a->v != a->v_next && a->u != a->v_next && a->v != a->u_next, "%s: u / v alias u_next / v_next", who);
    }
    const int grid = train_grid_size(a->max_workgroups, (g.rows + 31) / 32);
    if (int e = skip_check_ws(a, who, grid)) return e;
    LayerBwdParams p{};
    p.x = a->x; p.proj = a->proj; p.filter = a->filter; p.gate = a->gate; p.dense = a->dense;
    p.u_next = a->u_next; p.v_next = a->v_next;
    p.u = a->u; p.v = a->v; p.d_proj = a->d_proj; p.part = (float*)a->workspace;
    p.g = g;
    p.tab = tab;
    const SkipParams sp{a->skip, a->skip_bias, nullptr, s->d_skip_sum, 0};
    const dim3 grd(grid), blk(kTrThreads);
    const hipStream_t st = (hipStream_t)stream;
    if (s->cu_rows) {
        if (last) hipLaunchKernelGGL((train_skip_layer_bwd_kernel<PackedGeo, true>), grd, blk, 0, st, p, sp);
        else hipLaunchKernelGGL((train_skip_layer_bwd_kernel<PackedGeo, false>), grd, blk, 0, st, p, sp);
    } else {
        if (last) hipLaunchKernelGGL((train_skip_layer_bwd_kernel<UniformGeo, true>), grd, blk, 0, st, p, sp);
        else hipLaunchKernelGGL((train_skip_layer_bwd_kernel<UniformGeo, false>), grd, blk, 0, st, p, sp);
    }
    PWV_CHECK_HIP(hipGetLastError());
    // stage two: dWfg | d dense | d dense_bias | d skip; a PWV_TRAIN_LAST layer has no dense
    ReduceParams rp;
    rp.part = p.part; rp.n_part = grid; rp.stride = kSkipLayerPart; rp.total = kSkipLayerPart; rp.n_seg = 4;
    rp.seg[0] = ReduceSeg{0, 128 * 128, a->d_filter, a->d_gate};
    rp.seg[1] = ReduceSeg{128 * 128, 128 * 128 + 64 * 64, last ? nullptr : a->d_dense, nullptr};
    rp.seg[2] = ReduceSeg{128 * 128 + 64 * 64, kLayerPart, last ? nullptr : a->d_dense_bias, nullptr};
    rp.seg[3] = ReduceSeg{kLayerPart, kSkipLayerPart, s->d_skip, nullptr};
    return train_reduce(rp, st);
}
