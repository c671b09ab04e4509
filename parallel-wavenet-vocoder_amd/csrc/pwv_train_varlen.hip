// Training on packed batches (include/pwv_hip_train_varlen.h; DESIGN.md section 9, "Packed training"): the unit bodies of
// pwv_train_units.h instantiated with the packed geometry policy -- utterance i owns rows cu_rows[i] .. cu_rows[i + 1] - 1, the tables
// are read on the device, and 33 threads locate the rows of a 32-row unit once per unit, into LDS.  The head, the reduction of the
// weight-gradient partials and the workspace are those of csrc/pwv_train.hip.  Behind them the packed loss head.
#include <cfloat>

#include "pwv_common.h"
#include "pwv_hip_train_varlen.h"
#include "pwv_train_loss_frame.h"
#include "pwv_train_units.h"

namespace pwv {

struct FrontFwdParams {
    const float *in, *cf;
    float* x0;
    Geom g;
    PackedTables tab;
};

// x_0[t] = in[t - 1] cf[0] + in[t] cf[1], in[-1] = 0 at every utterance's first sample; one unit per workgroup
__global__ __launch_bounds__(kTrThreads) void train_front_fwd_varlen_kernel(FrontFwdParams p) {
    __shared__ PackedGeo::Loc loc;
    const int u = blockIdx.x;
    PackedGeo::locate(loc, u, p.g, p.tab);
    for (int idx = threadIdx.x; idx < 512; idx += kTrThreads) {
        const int q = idx >> 5, r = idx & 31, row = 32 * u + r;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (row < p.g.rows) {
            const float cur = p.in[row], prev = loc.t[r] > 0 ? p.in[row - 1] : 0.f;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = prev * p.cf[4 * q + e] + cur * p.cf[64 + 4 * q + e];
        }
        *reinterpret_cast<f32x4*>(p.x0 + (size_t)u * 2048 + q * 128 + r * 4) = v;
    }
}

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

// ------------------------------------------------------------------------------------------------------------------------------
// the packed loss head: the frame body of csrc/pwv_train_loss.hip (pwv_train_loss_frame.h); the lengths are read on the device, the
// grids are sized from the capacities n and rows, every workgroup finds its utterance by bisection and leaves if its slot is not in
// use (the scheme of csrc/pwv_score.hip)
// ------------------------------------------------------------------------------------------------------------------------------
struct LossVarlenParams {
    const float* out;
    const float* y;
    const int* cu;
    float* d_out;
    double* result;
    double* part;                       // [frame_slots] power partials, then [tile_slots] L1 partials
    double* grad;                       // [frame_slots][win]: the frames' gradients, unscaled
    double scale_l1, power4;            // weight_l1 / rows;  weight_power 4 (the kernel divides by B sum_i F_i)
    long long rows, frame_slots, tile_slots;
    int n, win, hop, nfft;              // win = 0: the L1 alone
};

// bound i of the batch (0 .. n), inside 0 .. rows whatever the table holds
__device__ __forceinline__ long long lossv_bound(const LossVarlenParams& p, int i) {
    const long long v = p.cu[i];
    return v < 0 ? 0 : (v > p.rows ? p.rows : v);
}

// utterance i = samples [s, e)
__device__ __forceinline__ void lossv_span(const LossVarlenParams& p, int i, long long& s, long long& e) {
    s = lossv_bound(p, i);
    e = lossv_bound(p, i + 1);
    if (e < s) e = s;
}

__device__ __forceinline__ long long lossv_frames(const LossVarlenParams& p, long long L) {
    return p.win < 1 || L < p.win ? 0 : 1 + (L - p.win) / p.hop;
}

// The utterance that owns `slot` where utterance i's slots begin at bound(i) / unit + i (strictly increasing in i), and the slot's index
// within it (negative: before the first utterance's).  Every thread of the workgroup gets the same answer.
__device__ __forceinline__ int lossv_owner(const LossVarlenParams& p, long long slot, int unit, long long& idx) {
    int lo = 0, hi = p.n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (lossv_bound(p, mid) / unit + mid <= slot) lo = mid; else hi = mid - 1;
    }
    idx = slot - (lossv_bound(p, lo) / unit + lo);
    return lo;
}

// blockIdx.x < frame_slots: a frame slot; else a tile slot
__global__ __launch_bounds__(256) void loss_frames_varlen_kernel(LossVarlenParams p) {
    extern __shared__ __attribute__((aligned(16))) double loss_sm[];
    double* red = loss_sm;
    const int tid = threadIdx.x;
    long long slot = blockIdx.x, idx, s, e;
    if (slot < p.frame_slots) {
        const int i = lossv_owner(p, slot, p.hop, idx);
        lossv_span(p, i, s, e);
        if (idx < 0 || idx >= lossv_frames(p, e - s)) return;             // (uniform over the workgroup: before any barrier)
        const long long at = s + idx * p.hop;                             // the frame ends at s + idx hop + win - 1 <= e - 1 < rows
        loss_frame(p.out + at, p.y + at, p.win, p.nfft, red, p.part + slot, p.grad + (size_t)slot * p.win);
        return;
    }
    slot -= p.frame_slots;
    const int i = lossv_owner(p, slot, kLossTile, idx);
    lossv_span(p, i, s, e);
    const long long L = e - s, first = idx * kLossTile;
    if (idx < 0 || first >= L) return;
    double acc = 0.0;
    for (long long t = first + tid; t < first + kLossTile && t < L; t += kLossThreads) acc += fabs((double)p.out[s + t] - (double)p.y[s + t]);
    acc = loss_block_sum(acc, red);
    if (tid == 0) p.part[p.frame_slots + slot] = acc;
}

// blockIdx.x < tile_slots: d_out of a tile of samples; else the table row of utterance blockIdx.x - tile_slots
__global__ __launch_bounds__(256) void loss_gather_varlen_kernel(LossVarlenParams p) {
    __shared__ double red[kLossThreads];
    const int tid = threadIdx.x;
    const long long slot = blockIdx.x;
    long long idx, s, e;
    if (slot < p.tile_slots) {
        const int i = lossv_owner(p, slot, kLossTile, idx);
        lossv_span(p, i, s, e);
        const long long L = e - s, first = idx * kLossTile, F = lossv_frames(p, L);
        if (idx < 0 || first >= L) return;                                // (uniform over the workgroup: before any barrier)
        double scale_power = 0.0;
        if (p.win > 0) {                                                  // the batch's frames: integers, exact in any order
            double tot = 0.0;
            for (int k = tid; k < p.n; k += kLossThreads) {
                long long ks, ke;
                lossv_span(p, k, ks, ke);
                tot += (double)lossv_frames(p, ke - ks);
            }
            tot = loss_block_sum(tot, red);
            if (tot > 0.0) scale_power = p.power4 / (tot * (p.nfft / 2 + 1));
        }
        const double* g = p.grad + (size_t)(s / p.hop + i) * p.win;
        for (long long t = first + tid; t < first + kLossTile && t < L; t += kLossThreads) {
            const double diff = (double)p.out[s + t] - (double)p.y[s + t];
            double v = p.scale_l1 * (diff > 0.0 ? 1.0 : (diff < 0.0 ? -1.0 : 0.0));
            if (F > 0) {
                // the frames f with 0 <= t - f hop < win, in ascending order; none behind the last frame or in a gap (hop > win)
                const long long lo = t >= p.win ? (t - p.win) / p.hop + 1 : 0;
                const long long hi = t / p.hop < F - 1 ? t / p.hop : F - 1;
                double sum = 0.0;
                for (long long f = lo; f <= hi; ++f) sum += g[(size_t)f * p.win + (t - f * p.hop)];
                v = fma(scale_power, sum, v);
            }
            p.d_out[s + t] = (float)v;
        }
        return;
    }
    // thread t adds the partials t, t + 256, ... of the utterance in that order, the 256 sums go through the tree
    const int i = (int)(slot - p.tile_slots);
    lossv_span(p, i, s, e);
    const long long L = e - s, frames = lossv_frames(p, L), tiles = (L + kLossTile - 1) / kLossTile;
    double pw = 0.0, l1 = 0.0;
    if (frames > 0) {
        const double* part = p.part + (s / p.hop + i);
        for (long long f = tid; f < frames; f += kLossThreads) pw += part[f];
    }
    const double* part = p.part + p.frame_slots + (s / kLossTile + i);
    for (long long t = tid; t < tiles; t += kLossThreads) l1 += part[t];
    pw = loss_block_sum(pw, red);
    l1 = loss_block_sum(l1, red);
    if (tid == 0) {
        double* r = p.result + 4 * (size_t)i;
        r[0] = l1;
        r[1] = (double)L;
        r[2] = pw;
        r[3] = (double)frames * (double)(frames > 0 ? p.nfft / 2 + 1 : 0);
    }
}

static size_t lossv_workspace_doubles(const LossVarlenParams& p) {
    return (size_t)p.frame_slots + (size_t)p.tile_slots + (size_t)p.frame_slots * p.win;
}

static int lossv_params(const pwv_train_loss_varlen_args* a, const char* who, LossVarlenParams* p, bool need_buffers) {
    PWV_CHECK_ARG(a, "%s: args is NULL", who);
    PWV_CHECK_ARG(a->struct_size == sizeof(pwv_train_loss_varlen_args), "%s: struct_size %zu is not sizeof(pwv_train_loss_varlen_args) = %zu", who,
                  a->struct_size, sizeof(pwv_train_loss_varlen_args));
    PWV_CHECK_ARG(a->n >= 1, "%s: n %d must be >= 1", who, a->n);
    PWV_CHECK_ARG(a->rows >= a->n, "%s: rows %d is below n %d", who, a->rows, a->n);
    PWV_CHECK_ARG((long long)a->rows < (1ll << 31) - 64, "%s: rows %d is beyond int32 (2^31 - 64)", who, a->rows);
    PWV_CHECK_ARG(a->hop_length >= 1, "%s: hop_length %d must be >= 1", who, a->hop_length);
    PWV_CHECK_ARG(a->win_length >= 0 && a->win_length <= PWV_SCORE_MAX_WIN, "%s: win_length %d must be 0 (L1 only) .. %d", who, a->win_length,
                  PWV_SCORE_MAX_WIN);
    PWV_CHECK_ARG(a->weight_l1 >= 0.0 && a->weight_l1 <= DBL_MAX, "%s: weight_l1 %g must be finite and >= 0", who, a->weight_l1);
    PWV_CHECK_ARG(a->weight_power >= 0.0 && a->weight_power <= DBL_MAX, "%s: weight_power %g must be finite and >= 0", who, a->weight_power);
    const bool power = a->weight_power > 0.0 && a->win_length > 0;
    int nfft = 0;
    if (power)
        for (nfft = 1; nfft < a->win_length; nfft <<= 1) {}
    *p = LossVarlenParams{a->out, a->y, a->cu_rows, a->d_out, a->result, (double*)a->workspace, nullptr,
                          a->weight_l1 / (double)a->rows, power ? a->weight_power * 4.0 : 0.0,
                          a->rows, power ? (long long)a->rows / a->hop_length + a->n : 0, (long long)a->rows / kLossTile + a->n,
                          a->n, power ? a->win_length : 0, a->hop_length, nfft};
    PWV_CHECK_ARG(p->frame_slots + p->tile_slots + a->n <= 0x7fffffffll, "%s: rows %d / hop_length %d with n %d: more workgroups than a grid holds",
                  who, a->rows, a->hop_length, a->n);
    if (!need_buffers) return PWV_OK;
    PWV_CHECK_ARG(a->out, "%s: out is a NULL pointer", who);
    PWV_CHECK_ARG(a->y, "%s: y is a NULL pointer", who);
    PWV_CHECK_ARG(a->cu_rows, "%s: cu_rows is a NULL pointer", who);
    PWV_CHECK_ARG(a->d_out, "%s: d_out is a NULL pointer", who);
    PWV_CHECK_ARG(a->result, "%s: result is a NULL pointer", who);
    PWV_CHECK_ARG(a->workspace, "%s: workspace is a NULL pointer", who);
    const size_t need = lossv_workspace_doubles(*p) * sizeof(double);
    PWV_CHECK_ARG(a->workspace_bytes >= need, "%s: workspace_bytes %zu is too small (pwv_train_loss_varlen_workspace_bytes: %zu)", who,
                  a->workspace_bytes, need);
    p->grad = p->part + p->frame_slots + p->tile_slots;
    return PWV_OK;
}

}  // namespace pwv

using namespace pwv;

extern "C" int pwv_train_varlen_front_fwd_f32(const pwv_train_varlen_args* a, pwv_stream_t stream) {
    const char* who = "pwv_train_varlen_front_fwd_f32";
    FrontFwdParams p{};
    if (int e = varlen_check(a, who, p.g, p.tab, false)) return e;
    PWV_CHECK_ARG(a->in && a->causal_filter && a->x_out, "%s: in, causal_filter or x_out is a NULL pointer", who);
    p.in = a->in; p.cf = a->causal_filter; p.x0 = a->x_out;
    hipLaunchKernelGGL(train_front_fwd_varlen_kernel, dim3((p.g.rows + 31) / 32), dim3(kTrThreads), 0, (hipStream_t)stream, p);
    PWV_CHECK_HIP(hipGetLastError());
    return PWV_OK;
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

extern "C" size_t pwv_train_loss_varlen_workspace_bytes(const pwv_train_loss_varlen_args* a) {
    LossVarlenParams p{};
    if (lossv_params(a, "pwv_train_loss_varlen_workspace_bytes", &p, false) != PWV_OK) return 0;
    return lossv_workspace_doubles(p) * sizeof(double);
}

extern "C" int pwv_train_loss_varlen_f32(const pwv_train_loss_varlen_args* a, pwv_stream_t stream) {
    LossVarlenParams p{};
    const int rc = lossv_params(a, "pwv_train_loss_varlen_f32", &p, true);
    if (rc != PWV_OK) return rc;
    const size_t smem = (size_t)(kLossThreads + 2 * p.nfft + 2 * (p.nfft / 2 + 1) + 2 * p.win) * sizeof(double);
    hipLaunchKernelGGL(loss_frames_varlen_kernel, dim3((unsigned)(p.frame_slots + p.tile_slots)), dim3(kLossThreads), smem, (hipStream_t)stream, p);
    PWV_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(loss_gather_varlen_kernel, dim3((unsigned)(p.tile_slots + p.n)), dim3(kLossThreads), 0, (hipStream_t)stream, p);
    PWV_CHECK_HIP(hipGetLastError());
    return PWV_OK;
}
