// The host side of a persistent launch (pwv_stack_persist.hip) that needs no device: how the units are dealt to workgroups (PersistPlan)
// and where the polled words lie in the workspace (PersistLayout).  Plain C++, no HIP include: tests/test_persist_plan_host.py builds it
// into a stand-alone program.  A refusal goes through PWV_CHECK_ARG(cond, printf-style message); a program that has not defined it
// gets the bare return code.
#pragma once

#include <cstddef>

#include "pwv_hip.h"

#ifndef PWV_CHECK_ARG
#define PWV_CHECK_ARG(cond, ...)          \
    do {                                  \
        if (!(cond)) return PWV_EINVAL;   \
    } while (0)
#endif

namespace pwv {

constexpr int kLeftN = 32;                 // unit mode (short inputs): "layers completed" bytes of the 32 units LEFT of the range, as last seen
// unit mode up to this many units per workgroup and layer (wave 7 is the loader.  Against the general kernel: 4 units per workgroup -17 %,
// 5: -8 %, 6: -11.5 %, 7: -11 %; profiles/r06_ab_experiments.md, r06_z2)
constexpr int kUnitModeMaxPerWg = 7;
constexpr int kUnitStride = 32;            // ints between two units' words (own 128-byte lines: a poll asks for exactly the unit it waits for)
constexpr int kMaxPLayers = 32;
constexpr int kProgStride = 32;            // ints between two workgroups' progress words (own 128-byte lines)
constexpr int kMaxReachWgs = 60;           // neighbours polled by one wave instruction
constexpr int kMaxUnitsWg = 832;           // units per workgroup: the per-unit bytes behind the kernel's LDS layout (checked against it there)
constexpr int kPlanMaxQ = 4;               // head outputs of the tail (kMaxQ, pwv_layer_common.h; checked there)

struct PersistPlan { int units, nwg, per_wg, last_wg, reach_wgs, xcd_map, tail_reach_wgs, unit_mode; };

inline int persist_plan(int G, long long rows, int n_layers, const int* dil, int cus, int max_wgs, int min_units, int tail_q, int tail_dil, PersistPlan& pl) {
    PWV_CHECK_ARG(G >= 1 && G <= PWV_MAX_NETS, "persistent stack: G=%d out of range", G);
    PWV_CHECK_ARG(n_layers >= 2 && n_layers <= kMaxPLayers && dil, "persistent stack: 2..%d layers per launch, got %d", kMaxPLayers, n_layers);
    PWV_CHECK_ARG(rows >= 1 && rows < (1ll << 31) - 256, "persistent stack: bad N*T");
    PWV_CHECK_ARG(cus >= G, "persistent stack: %d CUs for %d nets", cus, G);
    int dmax = 1;
    for (int j = 0; j < n_layers; ++j) {
        PWV_CHECK_ARG(dil[j] >= 1, "persistent stack: bad dilation");
        dmax = dil[j] > dmax ? dil[j] : dmax;
    }
    pl.units = (int)((rows + 31) / 32);
    PWV_CHECK_ARG((long long)pl.units * 8192 < (1ll << 32), "persistent stack: buffers beyond the 4 GB reach of a buffer descriptor");
    int wgs = cus / G;                                  // every workgroup must be resident: one per CU (its LDS is the whole CU's)
    if (max_wgs > 0 && max_wgs / G < wgs) wgs = max_wgs / G;
    PWV_CHECK_ARG(wgs >= 1, "persistent stack: no workgroups");
    // short inputs: at least `min_units` units per workgroup and layer: fewer workgroups instead of ranges of one or two units
    // (default 4 = one per SIMD; measured at 16000 rows x 2 nets: 0.64 ms per forward with 4, 0.76 ms with 8)
    if (min_units <= 0) min_units = 4;
    int want = (pl.units + min_units - 1) / min_units;
    if (want < 1) want = 1;
    pl.nwg = wgs < want ? wgs : want;
    pl.per_wg = (pl.units + pl.nwg - 1) / pl.nwg;
    PWV_CHECK_ARG(pl.per_wg <= kMaxUnitsWg, "persistent stack: %d units per workgroup (max %d)", pl.per_wg, kMaxUnitsWg);
    pl.last_wg = (pl.units - 1) / pl.per_wg;
    const int reach = (dmax + 31) / 32;      // units a task looks back (RAW) / is looked back at from (WAR)
    pl.reach_wgs = (reach + pl.per_wg - 1) / pl.per_wg;
    PWV_CHECK_ARG(pl.reach_wgs <= kMaxReachWgs, "persistent stack: dilation %d reaches over %d workgroups (max %d)", dmax, pl.reach_wgs, kMaxReachWgs);
    const int grid = G * pl.nwg;
    pl.xcd_map = (pl.nwg % 8 == 0 && grid % 8 == 0) ? 1 : 0;
    // Short inputs (a handful of units per workgroup and layer: every layer is ONE unit's latency per SIMD): progress per UNIT instead of per
    // workgroup.  A range's bottom unit waits for the left neighbour's TOP units, which that workgroup computes FIRST; its workgroup word
    // appears only when its slowest unit -- its own bottom one, which waited for ITS left neighbour -- is through: with workgroup words every
    // layer of the chain costs a cross-workgroup hop (profiles/r06_short_timeline.md).
    pl.unit_mode = 0;      // 2: the short-input instantiation (the launcher: and a folded layer 0, if the run starts there)
    if (reach <= kLeftN && pl.nwg > 1 && pl.per_wg <= kUnitModeMaxPerWg) {
        pl.unit_mode = 2;
        PWV_CHECK_ARG(pl.reach_wgs <= 32, "persistent stack: unit mode polls at most 32 right neighbours (reach %d workgroups)", pl.reach_wgs);
    }
    // the tail's layer looks back too (a stack whose LAST dilation is its largest passed the probe and failed at the launch)
    pl.tail_reach_wgs = 0;
    if (tail_q > 0) {
        PWV_CHECK_ARG(tail_q <= kPlanMaxQ && tail_dil >= 1, "persistent stack: tail_q 1..%d, tail_dilation >= 1", kPlanMaxQ);
        PWV_CHECK_ARG(rows * tail_q * 4 < (1ll << 32), "persistent stack: tail_out beyond the 4 GB reach of a buffer descriptor");
        pl.tail_reach_wgs = ((tail_dil + 31) / 32 + pl.per_wg - 1) / pl.per_wg;
        PWV_CHECK_ARG(pl.tail_reach_wgs <= kMaxReachWgs, "persistent stack: tail dilation %d reaches over %d workgroups (max %d)", tail_dil, pl.tail_reach_wgs, kMaxReachWgs);
    }
    return PWV_OK;
}

// The workspace, in bytes from its start: [G][nwg] progress words, kProgStride ints apart, with the abort word and the exit counter behind
// them (prog_bytes .. prog_bytes + 8; one 256-byte line); at pair_off one arrival counter per range (the tail's affine); at uprog_off, in
// unit mode, one word per unit and net, kUnitStride ints apart.  Every part 256-byte aligned; `total` is what the launch needs and zeroes.
struct PersistLayout { size_t prog_bytes, pair_off, uprog_off, total; };

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

inline PersistLayout persist_layout(int G, const PersistPlan& pl) {
    PersistLayout l;
    l.prog_bytes = (size_t)G * pl.nwg * kProgStride * 4;
    l.pair_off = align256(l.prog_bytes + 256);
    l.uprog_off = l.pair_off + align256((size_t)pl.nwg * 4);
    l.total = l.uprog_off + (pl.unit_mode ? align256((size_t)G * pl.units * kUnitStride * 4) : 0);
    return l;
}

}  // namespace pwv
