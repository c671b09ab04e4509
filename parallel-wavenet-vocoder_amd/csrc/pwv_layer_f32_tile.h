// The register tile of one 32-row unit of the exact-fp32 layer kernels and its loads: shared by pwv_layer.hip and the streaming forms with a
// per-sample condition (pwv_layer_stream_cond.hip) or with skip accumulation (pwv_layer_stream_skip.hip), which include the same body text
// (pwv_layer_f32_body.inc).
#pragma once

#include "pwv_layer_common.h"

namespace pwv {

template <bool SKIP, bool COND>
struct TileRegs {
    float xb[32];                 // x[t-d], this lane's 32 channels
    float xc[32];                 // x[t]
    float pj[64];                 // P[frame(t)] : accumulator init for the 4 F/G row tiles
    float cd[COND ? 40 : 4];      // cond[t], this lane's 40 channels
    float sk[SKIP ? 64 : 4];      // running skip sum (D layout)
    int row;                      // flattened row n*T + t of this lane
    int t;                        // position inside the utterance
    bool valid;
};

// the skip-sum row [128] of a unit: chunk for (it, q) = channel quad 8*it + 2*q + h
template <bool SKIP, bool COND>
__device__ __forceinline__ void load_skip_row(const LayerParams& p, int net, int lane, TileRegs<SKIP, COND>& r, bool skip_load) {
    if constexpr (SKIP) {
        const int h = lane >> 5;
        const int rows = p.N * p.T;
        const int rc = r.valid ? r.row : rows - 1;
        if (skip_load) {
            const float* srow = p.skip[net] + tile_off(rc, h, 128);
#pragma unroll
            for (int it = 0; it < 4; ++it)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(srow + (8 * it + 2 * q) * 128);
#pragma unroll
                    for (int e = 0; e < 4; ++e) r.sk[it * 16 + q * 4 + e] = v[e];
                }
        } else {
#pragma unroll
            for (int i = 0; i < 64; ++i) r.sk[i] = 0.f;
        }
    }
}

// The skip-sum row is NOT loaded with the tile (the kernel requests it in front of GEMM2 / the gating instead: its 64 registers
// next to x[t-d], x[t], P and the per-sample condition at the top of the unit were the 27-35 spilled VGPRs of the SKIP + COND
// variants)
// STREAM (layer_f32_stream_kernel): rows left of the chunk come from the session's history block instead of zeros (StreamParams,
// pwv_layer_common.h; every address a valid one, selected rather than predicated); `wr` = the block the lane's utterance writes.
template <bool SKIP, bool COND, bool FIRST, bool STREAM>
__device__ __forceinline__ void load_tile(const LayerParams& p, const StreamParams& st, int net, int unit, int lane, TileRegs<SKIP, COND>& r, int& wr) {
    const int h = lane >> 5;
    const int rows = p.N * p.T;
    const int row = unit * 32 + (lane & 31);
    r.row = row;
    r.valid = row < rows;

    const int rc = r.valid ? row : rows - 1;          // clamped: loads never leave the tensor
    const int n = rc / p.T;
    const int t = rc - n * p.T;
    const bool has_prev = t >= p.dilation;            // x[t-d] = 0 left of the utterance start
    r.t = t;
    if constexpr (STREAM) {
        const int2 blk = reinterpret_cast<const int2*>(st.slot_tab)[n];
        wr = blk.y;
        const float* hist = st.hist_rd + (long long)blk.x * st.block_stride;
        if constexpr (FIRST) {
            const float* x1 = p.x_first + rc;
            const float* hx = hist + st.scalar_off;      // x[-(d + 1)] .. x[-1]: time r < 0 is hx[d + 1 + r]
            const int d = p.dilation;
            r.xc[0] = *x1;
            r.xc[1] = *(t >= 1 ? x1 - 1 : hx + d);
            r.xb[0] = *(has_prev ? x1 - d : hx + t + 1);
            r.xb[1] = *(t >= d + 1 ? x1 - d - 1 : hx + t);
        } else {
            load_tiled<8, 64>(p.x_in[net], rc, h, true, r.xc);
            load_tiled<8, 64>(has_prev ? p.x_in[net] : hist + st.row_off[net], has_prev ? rc - p.dilation : t, h, true, r.xb);
        }
    } else if constexpr (FIRST) {
        // the four scalars the two rows are functions of: x[t], x[t-1], x[t-d], x[t-d-1] (zero left of the start);
        // rebuild_first() turns them into the rows
        const float* x1 = p.x_first;
        const int d = p.dilation;
        r.xc[0] = x1[rc];
        r.xc[1] = t >= 1 ? x1[rc - (t >= 1 ? 1 : 0)] : 0.f;
        r.xb[0] = has_prev ? x1[rc - (has_prev ? d : 0)] : 0.f;
        r.xb[1] = t >= d + 1 ? x1[rc - (t >= d + 1 ? d + 1 : 0)] : 0.f;
    } else {
        load_tiled<8, 64>(p.x_in[net], rc, h, true, r.xc);
        load_tiled<8, 64>(p.x_in[net], has_prev ? rc - p.dilation : rc, h, has_prev, r.xb);
    }
    int prow = 0;
    if (p.cond_hop > 0) prow = n * p.cond_frames + fast_div(t + p.cond_offset, p.hop_magic, p.hop_shift);
    load_contig<16>(p.proj[net] + (size_t)prow * p.proj_row_stride + h * 64, r.pj);
    if constexpr (COND) load_tiled<10, kCondC>(p.cond, rc, h, true, r.cd);
}

}  // namespace pwv
