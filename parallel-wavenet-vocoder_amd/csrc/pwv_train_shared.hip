// Training the shared-net architecture (include/pwv_hip_train_shared.h; DESIGN.md section 9, "Training the shared-net architecture"):
// one net per flow with two output channels, y_0 the scale and y_1 the shift.  Only the head knows the output width, so this file is
// the Q = 2 instances of the head of csrc/pwv_train_head.h, over both input policies (GatedIn: from the last layer's o; SumIn: from
// the skip sum S), and the entry points that check pwv_train_shared_args and choose between the two.
#include "pwv_common.h"
#include "pwv_hip_train_shared.h"
#include "pwv_train_head.h"

namespace pwv {

constexpr int kSharedMaxPart = head_part<GatedIn, 2>() > kMaxPart ? head_part<GatedIn, 2>() : kMaxPart;

template <class In>
__global__ __launch_bounds__(kTrThreads) void train_shared_head_fwd_kernel(HeadParams p) {
    head_fwd_body<In, 2>(p);
}

template <class In>
__global__ __launch_bounds__(kTrThreads) void train_shared_head_bwd_kernel(HeadParams p) {
    head_bwd_body<In, 2>(p);
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

static int shared_head_check(const pwv_train_shared_args* s, const char* who) {
    if (int e = shared_check(s, who)) return e;
    const pwv_train_args* a = &s->train;
    if (s->head_in == PWV_TRAIN_HEAD_IN_GATED) {
        PWV_CHECK_ARG(a->x, "%s: train.x is a NULL pointer (head_in GATED reads the last layer's o)", who);
        PWV_CHECK_ARG(a->skip, "%s: train.skip is a NULL pointer (head_in GATED)", who);
    } else {
        PWV_CHECK_ARG(s->skip_sum, "%s: skip_sum is a NULL pointer (head_in SKIPSUM)", who);
    }
    PWV_CHECK_ARG(a->post1 && a->post2, "%s: post1 or post2 is a NULL pointer", who);
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
    if (int e = shared_head_check(s, who)) return e;
    const pwv_train_args* a = &s->train;
    PWV_CHECK_ARG(a->y, "%s: train.y is a NULL pointer", who);
    PWV_CHECK_ARG(s->y_shift, "%s: y_shift is a NULL pointer", who);
    const HeadParams p = head_params(a, a->N * a->T, s->skip_sum, s->d_skip_sum_out, s->y_shift);
    const bool gated = s->head_in == PWV_TRAIN_HEAD_IN_GATED;
    return head_fwd_launch(gated ? train_shared_head_fwd_kernel<GatedIn> : train_shared_head_fwd_kernel<SumIn>, p,
                           train_grid_size(a->max_workgroups, (p.rows + 31) / 32), (hipStream_t)stream);
}

extern "C" int pwv_train_shared_head_bwd_f32(const pwv_train_shared_args* s, pwv_stream_t stream) {
    const char* who = "pwv_train_shared_head_bwd_f32";
    if (int e = shared_head_check(s, who)) return e;
    const pwv_train_args* a = &s->train;
    const bool gated = s->head_in == PWV_TRAIN_HEAD_IN_GATED;
    PWV_CHECK_ARG(a->d_out, "%s: train.d_out is a NULL pointer", who);
    if (gated) PWV_CHECK_ARG(a->d_o_out, "%s: train.d_o_out is a NULL pointer (head_in GATED)", who);
    else PWV_CHECK_ARG(s->d_skip_sum_out, "%s: d_skip_sum_out is a NULL pointer (head_in SKIPSUM)", who);
    const HeadParams p = head_params(a, a->N * a->T, s->skip_sum, s->d_skip_sum_out, s->y_shift);
    const int grid = train_grid_size(a->max_workgroups, (p.rows + 31) / 32);
    PWV_CHECK_ARG(a->workspace, "%s: workspace is a NULL pointer", who);
    PWV_CHECK_ARG(a->workspace_bytes >= (size_t)grid * kSharedMaxPart * sizeof(float),
                  "%s: workspace_bytes %zu is short of the %zu pwv_train_shared_workspace_bytes gives", who, a->workspace_bytes,
                  (size_t)grid * kSharedMaxPart * sizeof(float));
    const hipStream_t st = (hipStream_t)stream;
    if (gated) return head_bwd_launch_and_reduce<GatedIn, 2>(train_shared_head_bwd_kernel<GatedIn>, p, grid, a, a->d_skip_bias, st);
    return head_bwd_launch_and_reduce<SumIn, 2>(train_shared_head_bwd_kernel<SumIn>, p, grid, a, a->d_skip_bias, st);
}
