// Persistent kernel for a run of consecutive gated-residual layers (modules.py:185-259, the loop at modules.py:138-143)
// of one or two nets -- ONE launch instead of one launch per layer, split-fp16 or exact-fp32 arithmetic.
//
// Why: a per-layer launch of layer_f16x3_kernel pays, besides its steady state, a weight-staging prologue (1.7 us), the
// first rows' latency (1.3 us), the spread of its workgroups' end times (~8 %: every workgroup waits for the slowest at
// EVERY layer) and the gap to the dependent launch (1.5 us): ~20 % of a 46 us launch (HISTORY.md section 4, K1p).
//
// Round 3 design -- STATIC ownership (the round-2 kernel dealt (layer, unit) tasks out of per-XCD pools with global
// atomics, recomputed the x[t-d] halo per XCD and was 3 % slower than the launches it replaced):
//
//  * Workgroup w of a net owns the units [u_begin, u_end) -- the SAME contiguous rows in every layer, what the per-layer
//    kernel gives it per launch -- and walks layer after layer over them.  Nothing is recomputed.  Its 8 waves take
//    (layer, unit) tasks from ONE LDS counter, layer-major, units in DESCENDING order; a wave that finishes its last unit
//    of layer j takes a unit of layer j+1 at once: no barrier between layers, inside the workgroup or across the grid.
//  * Dependencies are tracked, not assumed.  RAW: task (j, u) reads layer j-1's units u, u - ceil(d/32), (32u+31-d)>>5.
//    WAR: it overwrites ring slot j % 3, last read by layer j-2's tasks of the units u, u + floor(d'/32), u + ceil(d'/32).
//    Inside the own range: one byte per unit in LDS ("layers completed").  Across workgroups: one progress word per
//    workgroup in global memory ("layers completed for ALL my units"), needed only by the bottom units (left neighbour's
//    top rows) and the top units (right neighbour's reads of the slot being overwritten).  With descending order and a
//    ring of THREE buffers both cross-workgroup dependencies are a whole layer old when they are needed: a workgroup is
//    coupled to its neighbours only loosely, so the per-layer end-time noise averages out instead of adding up.
//  * Visibility (MI355X_MICROARCH.md, inter-workgroup visibility; cdna_hip_programming.md Guideline 16 R1): every x load
//    is `sc1` (L2-served, never the CU's L1, which other CUs' stores do not refresh); units a neighbour reads are stored
//    write-through (`sc1`); every wave drains `vmcnt(0)` before it publishes; the progress word is an agent-scope store
//    by the LAST wave to leave the layer (each wave counts itself out only after its drain).
//  * Weights: LDS holds layers j and j+1 (2 x 79 KB + 2 x 256 B of dense bias); the last wave to leave layer j refills
//    that slot with layer j+2 by LDS-DMA and announces it at its next drain.  The 2 KB that buys the control state come
//    from the LAST 1 KB fragment of each layer's dense matrix, which every unit reads from global memory (one 16-byte load
//    per lane, an L1 / L2 hit) instead.
//  * The launch leaves its workspace as it found it (zeros): the last workgroup to finish cleans up, so a caller that keeps the
//    workspace needs no zeroing kernel in front of the next launch (pwv_persist_args.workspace_clean).
//  * Every wait is bounded (20 ms, or until any wave of the launch has given up) and reports through a sticky status word in pinned host memory; the host then reruns on the
//    per-layer path.  All workgroups must be resident (grid <= CUs, one workgroup per CU by its LDS size).
// Results are bit-identical to the per-layer launches (same per-unit arithmetic): tests/test_gpu_persist.py.
//
// Files: this one holds the constants of the LDS layout, PersistParams, the kernel templates and the launcher.  The kernels' body is
// pwv_stack_persist_body.inc, which includes its parts in order -- pwv_persist_geometry.inc (row maps, descriptors, row loaders),
// _protocol (dependency bytes, progress words, waits, task claiming), _loader, _fold0, _tasks (the unit's arithmetic in
// pwv_persist_unit_f32.inc / pwv_persist_unit_f16x3.inc), _tail (the fused head: pwv_head_f32.inc / pwv_head_f16x3.inc / pwv_head_pp2.inc, the
// very text of the per-layer HEAD kernels) and _exit.  The plan and the workspace layout need no device: pwv_persist_plan.h.
#include "pwv_f16x3.h"
#include "pwv_persist_plan.h"

#include <cstddef>
#include <cstdlib>
#include <cstring>

namespace pwv {

constexpr int kStoreAuxLocal = 0;              // cache policy of the stores of units no other workgroup reads (plain: produced and consumed through one CU's L2)

constexpr int kSlotFull = kA1Size + kA2Size;   // floats of a layer's matrices: filter|gate (hi+lo) + dense (hi+lo) = 81,920 B
constexpr int kSlot = kSlotFull - 256;         // held in LDS: everything but the last 1 KB fragment of the dense matrix
constexpr int kBiasF = 2 * kSlot;              // [2 slots][64] dense bias
constexpr int kCtlF = kBiasF + 128;            // control ints: [0] task counter, [1] abort, [2..3] flag bytes, [8 + j] waves that left layer j
constexpr int kCtlInts = 40;
constexpr int kLdsFloats = 40960;              // all 160 KB of the CU
constexpr int kCfF = kCtlF + kCtlInts;       // causal filter [2][64] (a run that starts with the net's layer 0, see x_first)
constexpr int kLeftB = (kCfF + 128) * 4;                   // ... in front of the own units' bytes, so one linear address serves both
constexpr int kDoneB = kLeftB + kLeftN;                    // byte offset of the per-unit "layers completed" bytes
constexpr int kMaxUnitsWgLds = kLdsFloats * 4 - kDoneB;    // units per workgroup: one "layers completed" byte each
static_assert(kMaxUnitsWg == kMaxUnitsWgLds && kPlanMaxQ == kMaxQ, "pwv_persist_plan.h restates the kernel's limits");
static_assert(kUnitModeMaxPerWg <= 7, "the short-input instantiation keeps wave 7 as its loader");
// unit mode reads the left neighbours' unit words with lanes 1 / 2 and the right neighbours' workgroup words with lanes 32..63 of one
// instruction (poll_units): the look-back stays within 32 units, and persist_plan grants it only with at most 32 right neighbours
static_assert(kLeftN <= 32, "unit mode: the right neighbours are polled by lanes 32..63 alone");
constexpr int kFlagB = (kCtlF + 2) * 4;        // flag bytes: +0 seenL, +1 seenR, +2 / +3 newest layer in LDS slot 0 / 1, +4 always 255
constexpr int kSeenLB = kFlagB, kSeenRB = kFlagB + 1, kWreadyB = kFlagB + 2, kTrueB = kFlagB + 4;
constexpr long long kWaitTicks = 2000000;      // a wave gives up after 20 ms of the chip-wide 100 MHz clock (normal waits: microseconds)

struct PersistParams {
    float* ring[PWV_MAX_NETS];             // three full-size tile32 buffers, `ring_stride` floats apart; layer j reads buffer (j + 2 + rot) % 3, writes (j + rot) % 3
    long long ring_stride;
    const float* packed[PWV_MAX_NETS];     // packed layers of this launch, `packed_stride` floats apart
    const float* proj[PWV_MAX_NETS];       // P rows; this launch's first layer at column 0, layer j at 128 j
    int* prog;                             // [G][nwg] progress words, kProgStride ints apart, zeroed per launch
    int* uprog;                            // unit mode: [G][units] "layers completed" per UNIT (the left neighbours' top units are what a range's bottom units wait for)
    int unit_mode;
    int* abort;                            // one word behind them: != 0 once any wave of the launch has given up
    int* exited;                           // ... and one more: workgroups that have finished; the last one zeroes all of these words
    int active_wgs;                        // workgroups that own units (the others return at once)
    int* status;                           // pinned host word: != 0 after a give-up
    long long packed_stride;
    int proj_row_stride;
    int G, N, T, n_layers, units, per_wg, nwg, last_wg, reach_wgs, xcd_map, rot;
    int all_wt;                            // != 0: every ring store is write-through (a layer's rows exceed the L2s: see the launcher)
    int cond_hop, cond_offset, cond_frames;
    unsigned T_magic, T_shift, hop_magic, hop_shift;
    int dil[kMaxPLayers];
    const float* x_first;                  // != NULL: the run starts with the net's layer 0, which rebuilds the causal layer from the scalar input
    const float* cfilt[PWV_MAX_NETS];      // ... and each net's causal filter [2,1,64]
    const float* fold0[PWV_MAX_NETS];      // optional: layer 0's filter|gate GEMM folded onto the four scalars (pwv_pack_first_fold_f16x3 / _f32)
    float x_limit;                         // range guard of the split-fp16 arithmetic on x_first (include/pwv_hip.h)
    int* range_flag;
    long long* trace;                      // -DPWV_PTRACE builds: per-wave cycle accounting (tools/persist_trace.py)
    long long* trace_ev;                   // -DPWV_PTRACE builds: per-wave event timeline, [wave][64][4] = {s_memrealtime, code, layer, unit | bits << 32}
    // TAIL (tail_q > 0; both arithmetics since round 6): behind the run's layers every workgroup runs the net's LAST layer with the post-processing
    // head behind it on its own units (layer_f16x3_kernel's HEAD variant, the same operations) -- and, with `pair`, the IAF affine
    const float* tail_layer[PWV_MAX_NETS]; // the last layer's packed weights (its filter|gate fragments are used)
    const float* tail_head[PWV_MAX_NETS];  // the packed head
    float* tail_out[PWV_MAX_NETS];         // [rows, tail_q]
    int tail_q, tail_dil, tail_reach_wgs;
    const float* affine_x;                 // != NULL: out = fma(x, s, b) (modules.py:59) for the workgroup's rows, by whichever of the
    float* affine_out;                     // two nets' workgroups of a range finishes second (G = 2, Q = 1), or in place (G = 1, Q = 2)
    int* pair;                             // [nwg] arrival counters of the two nets' workgroups of a range (zero on entry and on exit)
    // VARLEN instantiations: a packed batch (N = 1, T = R rows here); [units][kVarlenRec] records of pwv_varlen_unit_map (pwv_layer_common.h)
    const int* unit_map;
    // STREAM instantiations (pwv_persist_args.hist): the launch continues N sessions.  Session n reads block slot_tab[2n] of hist_rd and writes
    // block slot_tab[2n+1] of hist_wr (StreamParams, pwv_layer_common.h); hist_off[net][j] = float offset of the row history of the launch's
    // layer j inside a block ([n_layers]: the tail's layer), hist_scalar_off = the scalar history of a run that starts at x_first
    const float* hist_rd;
    float* hist_wr;
    const int* slot_tab;
    long long hist_block_stride;
    long long hist_scalar_off;
    long long hist_off[PWV_MAX_NETS][kMaxPLayers + 1];
    // RAGGED instantiations (stack_persist_ragged_kernel: VARLEN and STREAM): device int32 [N + 1], session n's chunk is rows cu_rows[n] .. cu_rows[n+1]-1
    const int* cu_rows;
};

// -DPWV_PTRACE: every wave accumulates s_memtime cycles: [0] whole loop, [1] drain at the top, [2] RAW spins, [3] WAR spins,
// [4] settle (publish / leave / refill), [5] units, [6] tasks that were not prefetched, [7] first task at, [8] last task done at;
// round 5, phases of a unit of the general loop (PT_PHASE: the time since the previous stamp goes to slot k): [9] top of the unit up
// to the drain (P row requested, next task located, look-back row split), [10] GEMM1, [11] GEMM2, [12] stores + moving on;
// inside [11] (PT_LAP: the time since PT_BEGIN or the previous lap goes to slot k): [13] prefetch_next (the next unit's rows requested -- and whatever
// the wave waits for before it gets on), [14] GEMM2 proper;
// inside [9] (PT_LAP from the loop's header on; the trace record keeps them in its words 21 .. 23): [15] header -> the P row's loads issued (row maps, the P address),
// [16] -> the first split8 of the unit's own rows done (next task located, its dependency byte read, whatever the wave waits for in front of the rows), [17] -> the
// other three split8, up to settle_top's drain
#ifdef PWV_PTRACE
#define PT_DECL long long pt_acc[18] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; long long pt_t = 0, pt_p = 0; (void)pt_t; (void)pt_p;
#define PT_BEGIN() pt_t = __builtin_amdgcn_s_memtime()
#define PT_END(k) pt_acc[k] += __builtin_amdgcn_s_memtime() - pt_t
#define PT_ADD(k, v) pt_acc[k] += (v)
#define PT_LAP(k) do { __builtin_amdgcn_sched_barrier(0); const long long pt_n = __builtin_amdgcn_s_memtime(); pt_acc[k] += pt_n - pt_t; pt_t = pt_n; __builtin_amdgcn_sched_barrier(0); } while (0)
#define PT_MARK() do { __builtin_amdgcn_sched_barrier(0); pt_p = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0); } while (0)
#define PT_PHASE(k) do { __builtin_amdgcn_sched_barrier(0); const long long pt_n = __builtin_amdgcn_s_memtime(); pt_acc[k] += pt_n - pt_p; pt_p = pt_n; __builtin_amdgcn_sched_barrier(0); } while (0)
// event timeline (round 6, tools/persist_timeline.py): 1 unit computed, 2 stores issued, 3 own stores acknowledged (in front of a wait; 13 in front of a WAR wait), 4 dependencies
// satisfied (12: the WAR ones; bits << 32: what was missing at the first look), 5 rows arrived + look-back split, 6 top drained, 7 workgroup progress word published, 8 tail entered
#define PT_EV(code, jj, uu) do { if (p.trace_ev && pt_nev < 64) { if (lane == 0) { long long* e_ = p.trace_ev + (((size_t)blockIdx.x * 8 + wave) * 64 + pt_nev) * 4; \
    e_[0] = __builtin_amdgcn_s_memrealtime(); e_[1] = (code); e_[2] = (jj); e_[3] = (long long)(uu); } ++pt_nev; } } while (0)
#else
#define PT_DECL
#define PT_BEGIN() do {} while (0)
#define PT_END(k) do {} while (0)
#define PT_ADD(k, v) do {} while (0)
#define PT_LAP(k) do {} while (0)
#define PT_MARK() do {} while (0)
#define PT_PHASE(k) do {} while (0)
#define PT_EV(code, jj, uu) do {} while (0)
#endif

// dependency bits of a task: [0] own x[t] rows, [1] [2] x[t-d] rows, [3] this layer's weights resident (RAW side);
// [4] [5] readers of the ring slot it overwrites (WAR)
constexpr unsigned kRawMask = 0xFu, kWarMask = 0x30u;

// GEMM2 (dense, K = 64) with the fragment source as a functor: the persistent kernel takes the last fragment from a register
template <typename FR, typename BH, typename BL, typename EF>
__device__ __forceinline__ void gemm16_dense(FR&& fr, f32x16 (&acc)[2], f16x8 (&ah)[4], f16x8 (&al)[4], BH&& bh, BL&& bl, EF&& extra) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        f16x8 nh[2] = {ah[0], ah[1]};
        f16x8 nl[2] = {al[0], al[1]};
        if (s + 1 < 4) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                nh[i] = fr(0, i, s + 1);
                nl[i] = fr(1, i, s + 1);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        const f16x8 b_h = bh(s);
        const f16x8 b_l = bl(s);
#pragma unroll
        for (int i = 0; i < 2; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], b_h, acc[i], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 2; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], b_l, acc[i], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 2; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[i], b_h, acc[i], 0, 0, 0);
        extra(s);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            ah[i] = nh[i];
            al[i] = nl[i];
        }
    }
}

// the same for the exact-fp32 arithmetic: 8 groups of (2 row tiles x 4 k-steps)
template <typename FR, typename BF, typename EF>
__device__ __forceinline__ void gemm_groups_dense(FR&& fr, f32x16 (&acc)[2], f32x4 (&a)[4], BF&& bval, EF&& extra) {
#pragma unroll
    for (int g = 0; g < 8; ++g) {
        f32x4 n[2] = {a[0], a[1]};
        if (g + 1 < 8) {
#pragma unroll
            for (int i = 0; i < 2; ++i) n[i] = fr(i, g + 1);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float b = bval(g * 4 + e);
#pragma unroll
            for (int i = 0; i < 2; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][e], b, acc[i], 0, 0, 0);
        }
        extra(g);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < 2; ++i) a[i] = n[i];
    }
}

// SHORT (round 6): the instantiation for short inputs (at most kUnitModeMaxPerWg units per workgroup and layer: progress words per unit, stationary
// units, a loader wave) -- a template parameter, not a run-time mode: as run-time branches in the general task loop the additions cost the long-input
// launch 2.7 % of its step (SGPR spills reloaded per unit, profiles/r06_ab_experiments.md r06_r)
// VARLEN: a packed batch of utterances of different lengths (pwv_persist_args.cu_rows): a lane's (utterance, time) and P row come from
// its unit's record (unit_rows_varlen) instead of row / T.  Nothing else differs: the plan, ring, progress words and workspace are
// defined on rows and units.  The instantiations without it compile to the instruction stream they had before it existed.
// STREAM: the uniform [N, T] launch continues N sessions (pwv_persist_args.hist) -- the two changes layer_*_stream_kernel makes against
// layer_*_kernel.  A lane whose row has t < d takes its look-back x[t-d] from the session's history of that layer's input (row t of the
// layer's tile32 row history in the block the session reads; layer 0 folded: the scalar history) instead of zero, and the lanes with
// t >= T - d store their layer-input row -- in registers anyway -- to row t + d - T of the block the session writes.  All but
// ceil(d/32) + 1 units per session and layer have __all(t >= d) and none of the stored rows: they run the one-shot instruction
// sequence; the history addresses are made under wave-uniform branches for the boundary units only and not kept.  Plan, ring, progress
// words and waits are the one-shot kernel's (the waits are defined on units: merely conservative for lanes that read the history; a
// push reads one generation and writes the other, so the history adds no dependency inside a launch).  Plain stores: the next
// reader of hist_wr is a later launch.  The instantiations without it compile to the instruction stream they had before it existed.
template <bool F32, int MODE, bool VARLEN, bool STREAM = false>
__global__ __launch_bounds__(512) void stack_persist_kernel(const PersistParams p) {
    static_assert(!(VARLEN && STREAM), "streaming of packed batches is not built");
#include "pwv_stack_persist_body.inc"
}

// RAGGED: a packed launch that continues N sessions with chunks of DIFFERENT lengths (pwv_persist_args.hist with hist->cu_rows ==
// pwv_persist_args.cu_rows) -- VARLEN and STREAM both on, a kernel name of its own.  Rows map to (time, P row) through the unit
// records as in the packed instantiations; the history is indexed per lane by the session's INDEX (rec[0] + (rc >= rec[3])) and the rows
// that become the next history are the last d of the lane's OWN session (T_n = cu_rows[n+1] - cu_rows[n], not the launch's R): both made
// under the wave-uniform branches that fence the boundary units, from the unit's record and one scalar load of cu_rows.
template <bool F32, int MODE>
__global__ __launch_bounds__(512) void stack_persist_ragged_kernel(const PersistParams p) {
    constexpr bool VARLEN = true, STREAM = true;
#include "pwv_stack_persist_body.inc"
}

// pwv_stream_carry_f32 in its packed form (pwv_stream_args.cu_rows: sessions of different chunk lengths): stream_carry_kernel (pwv_layer.hip) with
// session n's own T_n = cu_rows[n+1] - cu_rows[n].  A kernel of its own: the uniform one keeps its instruction stream.
__global__ __launch_bounds__(256) void stream_carry_ragged_kernel(const StreamParams st, const int* __restrict__ tab, const int* __restrict__ cu_rows) {
    const int e = blockIdx.x, n = blockIdx.y;
    const int T = cu_rows[n + 1] - cu_rows[n];
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
    const int total = ((keep + 31) >> 5) * 512;
    for (int i = threadIdx.x; i < total; i += blockDim.x) {
        const int k = (i >> 9) * 32 + (i & 31), q = (i >> 5) & 15;
        if (k < keep) *reinterpret_cast<f32x4*>(dst + tile_off(k, q, 64)) = *reinterpret_cast<const f32x4*>(src + tile_off(k + T, q, 64));
    }
}

int launch_stream_carry_ragged(const StreamParams& st, const int* tab, int n_carry, const int* cu_rows, int N, hipStream_t s) {
    hipLaunchKernelGGL(stream_carry_ragged_kernel, dim3(n_carry, N), dim3(256), 0, s, st, tab, cu_rows);
    PWV_CHECK_HIP(hipGetLastError());
    return PWV_OK;
}

// every polled word starts at zero on EVERY call: either the caller says the workspace is clean (fresh zeros, or left by an
// earlier launch, which cleans up after itself) or this kernel runs first.  A kernel, not hipMemsetAsync: under stream capture the
// memset node of a torch-captured graph did not reset the words on replay (tests/test_gpu_persist.py::test_whole_model_persistent_eager_and_graph_replay)
__global__ void persist_zero_kernel(int4* p, size_t n16) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n16) p[i] = int4{0, 0, 0, 0};
}

// one thread per unit of a packed batch: the record unit_rows_varlen reads (pwv_layer_common.h)
__global__ void varlen_unit_map_kernel(const int* __restrict__ cu_rows, const int* __restrict__ cu_frames, int n_utt, int units, int* __restrict__ out) {
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= units) return;
    const int r = u * 32;
    int lo = 0, hi = n_utt - 1;          // the last utterance that starts at or before row r
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (cu_rows[mid] <= r) lo = mid;
        else hi = mid - 1;
    }
    int4* o = reinterpret_cast<int4*>(out + (size_t)u * kVarlenRec);
    o[0] = int4{lo, cu_rows[lo], cu_frames ? cu_frames[lo] : 0, cu_rows[lo + 1]};
    o[1] = int4{cu_frames ? cu_frames[lo + 1] : 0, 0, 0, 0};
}

}  // namespace pwv

using namespace pwv;

extern "C" {

int pwv_persist_status(int** status) {
    static int* g_status = nullptr;      // process lifetime; pinned + mapped: one pointer valid on host and device
    PWV_CHECK_ARG(status, "pwv_persist_status: NULL argument");
    if (!g_status) {
        PWV_CHECK_HIP(hipHostMalloc((void**)&g_status, sizeof(int), hipHostMallocMapped | hipHostMallocPortable));
        *g_status = 0;
    }
    *status = g_status;
    return PWV_OK;
}

// the exact-fp32 ragged instantiations: built only if they stay spill-free ("Ragged pushes")
#ifndef RAGGED_F32
#define RAGGED_F32 1
#endif

// the four kernel families, each [F32][MODE == 2]
typedef void (*persist_kernel_t)(const PersistParams);
#define PERSIST_FAMILY(K, ...) {{K<false, 0, ##__VA_ARGS__>, K<false, 2, ##__VA_ARGS__>}, {K<true, 0, ##__VA_ARGS__>, K<true, 2, ##__VA_ARGS__>}}
static const persist_kernel_t kUniform[2][2] = PERSIST_FAMILY(stack_persist_kernel, false), kPacked[2][2] = PERSIST_FAMILY(stack_persist_kernel, true),
                              kStreaming[2][2] = PERSIST_FAMILY(stack_persist_kernel, false, true);
#if RAGGED_F32
static const persist_kernel_t kRagged[2][2] = PERSIST_FAMILY(stack_persist_ragged_kernel);
#else
static const persist_kernel_t kRagged[2][2] = {{stack_persist_ragged_kernel<false, 0>, stack_persist_ragged_kernel<false, 2>}, {nullptr, nullptr}};
#endif

static bool is_varlen(const pwv_persist_args* a) { return a->cu_rows || a->cu_frames || a->unit_map || a->varlen_rows != 0; }
// the rows a launch covers: N*T, or R of a packed batch
static long long launch_rows(const pwv_persist_args* a) { return is_varlen(a) ? a->varlen_rows : (long long)a->N * a->T; }

// the packed-batch fields are all set or all NULL / 0 (include/pwv_hip.h); checked before the plan, which needs a device
static int varlen_check(const pwv_persist_args* a, const char* who) {
    if (!is_varlen(a)) return PWV_OK;
    PWV_CHECK_ARG(a->cu_rows && a->unit_map && a->varlen_rows > 0, "%s: a packed batch needs cu_rows, unit_map and varlen_rows (R) together", who);
    PWV_CHECK_ARG(a->cond_hop <= 0 || a->cu_frames, "%s: a packed batch with a frame-rate condition (cond_hop > 0) needs cu_frames", who);
    PWV_CHECK_ARG(a->N >= 1 && a->varlen_rows >= (long long)kVarlenMinRows * a->N,
                  "%s: packed batch of %d utterances in %lld rows: every utterance needs at least %d rows", who, a->N, a->varlen_rows, kVarlenMinRows);
    return PWV_OK;
}

// STREAMING (pwv_persist_args.hist): what can be refused without a device, each with the field's name; `sa` receives the caller's
// pwv_stream_args as far as its struct_size reaches
static int stream_check(const pwv_persist_args* a, pwv_stream_args& sa, const char* who) {
    if (!a->hist) return PWV_OK;
    // (read ahead of the full copy below: is this the RAGGED form, hist->cu_rows set?  Only a struct that reaches the field can say so)
    const int32_t* h_cu = a->hist->struct_size >= offsetof(pwv_stream_args, cu_rows) + sizeof(const int32_t*) && a->hist->struct_size <= 4096
                              ? a->hist->cu_rows : nullptr;
    PWV_CHECK_ARG(!is_varlen(a) || h_cu, "%s: hist together with cu_rows: a packed batch streams only as the ragged launch (set hist->cu_rows too)", who);
    PWV_CHECK_ARG(!h_cu || is_varlen(a), "%s: hist->cu_rows is set but the launch is not packed (pwv_persist_args.cu_rows, unit_map, varlen_rows)", who);
    PWV_CHECK_ARG(!h_cu || h_cu == a->cu_rows, "%s: hist->cu_rows differs from pwv_persist_args.cu_rows: one table describes the launch", who);
    PWV_CHECK_ARG(a->precision == PWV_PREC_F16X3 || a->precision == PWV_PREC_F32, "%s: hist needs precision PWV_PREC_F16X3 or PWV_PREC_F32", who);
    PWV_CHECK_ARG(a->G >= 1 && a->G <= PWV_MAX_NETS, "%s: G=%d out of range", who, a->G);
    for (int g = 0; g < a->G; ++g) {
        PWV_CHECK_ARG(!a->x_first || a->first_fold[g], "%s: hist with x_first needs first_fold: layer 0 streams in its folded form only", who);
        PWV_CHECK_ARG(a->hist_row_off[g], "%s: hist without hist_row_off[%d]", who, g);
    }
    PWV_CHECK_ARG(a->hist->struct_size != 0, "%s: hist->struct_size is 0 (set it to sizeof(pwv_stream_args))", who);
    PWV_CHECK_ARG(a->hist->struct_size >= offsetof(pwv_stream_args, carry_tab) && a->hist->struct_size <= 4096,
                  "%s: hist->struct_size does not cover the history fields", who);
    sa = pwv_stream_args{};
    memcpy(&sa, a->hist, a->hist->struct_size < sizeof(sa) ? a->hist->struct_size : sizeof(sa));
    PWV_CHECK_ARG(sa.slot_tab, "%s: hist->slot_tab is NULL", who);
    PWV_CHECK_ARG(sa.hist_rd && sa.hist_wr, "%s: hist->hist_rd / hist->hist_wr is NULL", who);
    PWV_CHECK_ARG(sa.block_stride > 0 && sa.block_stride % 4 == 0, "%s: hist->block_stride must be a positive multiple of 4 floats", who);
    return PWV_OK;
}

// the short-input instantiation: the plan's verdict (units per workgroup, look-back reach), and a folded layer 0 if the run starts with one (it has
// no unfolded form), and the P rows inside the 2 GB its buffer descriptor's 32-bit offsets reach.  (The workspace is sized by the plan alone.)
static int short_input_mode(const pwv_persist_args* a, const PersistPlan& pl) {
    if (pl.unit_mode != 2) return 0;
    if (a->x_first && !a->first_fold[0]) return 0;
    // (a packed batch: R / hop + N frames, the layout's t_mel_i = len_i / hop + 1)
    const long long p_rows = a->cond_hop > 0 ? (is_varlen(a) ? a->varlen_rows / a->cond_hop + a->N : (long long)a->N * a->cond_frames) : 1;
    if (p_rows * a->proj_row_stride * 4 >= (1ll << 31)) return 0;
    return 2;
}

// The caller's struct, as far as the caller knows it (struct_size), in front of zeros: a client compiled against an earlier minor version
// of the header passes a shorter struct, and what lies behind it in its memory is not ours to read (a garbage `status`
// pointer would be written through on a give-up, a garbage tail_q would switch the tail on)
static int persist_args_copy(const pwv_persist_args* a, pwv_persist_args& out, const char* who) {
    PWV_CHECK_ARG(a, "%s: NULL argument", who);
    const size_t need = offsetof(pwv_persist_args, min_units_per_workgroup) + sizeof(int);
    PWV_CHECK_ARG(a->struct_size >= need, "%s: pwv_persist_args.struct_size = %zu (set it to sizeof(pwv_persist_args); at least %zu)", who,
                  (size_t)a->struct_size, need);
    memset(&out, 0, sizeof(out));
    memcpy(&out, a, a->struct_size < sizeof(out) ? a->struct_size : sizeof(out));
    return PWV_OK;
}

// One resolution of the caller's arguments for the three entry points: the struct copy, what can be refused without a device, the plan
// and the workspace layout.  `launch`: the launcher's own refusals, in the places they have always had among the others.
struct Resolved {
    pwv_persist_args a;
    pwv_stream_args sa;
    PersistPlan pl;
    PersistLayout lay;
};

static int persist_resolve(const pwv_persist_args* args, const char* who, Resolved& r, bool launch = false) {
    if (int rc = persist_args_copy(args, r.a, who)) return rc;
    const pwv_persist_args* a = &r.a;
    if (launch) PWV_CHECK_ARG(a->workspace, "%s: NULL workspace", who);
    if (int rc = varlen_check(a, who)) return rc;
    r.sa = pwv_stream_args{};
    const int cus = device_cus();
    if (launch) {
        if (int rc = stream_check(a, r.sa, who)) return rc;
        PWV_CHECK_ARG(!(a->hist && is_varlen(a)) || a->precision == PWV_PREC_F16X3 || RAGGED_F32, "%s: the ragged launch (hist->cu_rows) is built for PWV_PREC_F16X3 only", who);
        if (cus <= 0) return set_error(PWV_EHIP, "no HIP device");
    }
    if (int rc = persist_plan(a->G, launch_rows(a), a->n_layers, a->dilations, cus, a->max_workgroups, a->min_units_per_workgroup, a->tail_q, a->tail_dilation, r.pl)) return rc;
    r.lay = persist_layout(a->G, r.pl);
    return PWV_OK;
}

size_t pwv_persist_workspace_bytes(const pwv_persist_args* args) {
    Resolved r;
    return persist_resolve(args, "pwv_persist_workspace_bytes", r) == PWV_OK ? r.lay.total : 0;
}

int pwv_persist_short_input(const pwv_persist_args* args) {
    Resolved r;
    if (persist_resolve(args, "pwv_persist_short_input", r) != PWV_OK) return -1;
    return short_input_mode(&r.a, r.pl) == 2 ? 1 : 0;
}

int pwv_wavenet_stack_persist_f32(const pwv_persist_args* args, pwv_stream_t stream) {
    Resolved r;
    if (int rc0 = persist_resolve(args, "pwv_wavenet_stack_persist_f32", r, true)) return rc0;
    const pwv_persist_args* a = &r.a;
    const pwv_stream_args& sa = r.sa;
    PersistPlan& pl = r.pl;
    const bool varlen = is_varlen(a);
    const bool streaming = a->hist != nullptr;
    const bool ragged = streaming && varlen;      // (stream_check: then hist->cu_rows == cu_rows)
    PersistParams p{};
    PWV_CHECK_ARG(a->N >= 1 && (varlen || a->T >= 1), "pwv_wavenet_stack_persist_f32: bad N/T");
    PWV_CHECK_ARG(a->precision == PWV_PREC_F16X3 || a->precision == PWV_PREC_F32, "pwv_wavenet_stack_persist_f32: precision must be PWV_PREC_F16X3 or PWV_PREC_F32");
    PWV_CHECK_ARG(a->proj_row_stride % 4 == 0 && a->cond_hop >= 0, "pwv_wavenet_stack_persist_f32: bad projection arguments");
    PWV_CHECK_ARG(a->workspace_bytes >= r.lay.total, "pwv_wavenet_stack_persist_f32: workspace too small");
    PWV_CHECK_ARG(((uintptr_t)a->workspace & 255) == 0, "pwv_wavenet_stack_persist_f32: workspace must be 256-byte aligned");
    p.prog = (int*)a->workspace;
    p.abort = (int*)((char*)a->workspace + r.lay.prog_bytes);
    p.exited = p.abort + 1;
    int* const pair_words = (int*)((char*)a->workspace + r.lay.pair_off);
    p.uprog = (int*)((char*)a->workspace + r.lay.uprog_off);
    pl.unit_mode = short_input_mode(a, pl);
    p.unit_mode = pl.unit_mode;
    p.active_wgs = a->G * (pl.last_wg + 1);
    for (int g = 0; g < a->G; ++g) {
        PWV_CHECK_ARG(a->x_ring[g] && a->packed_layers[g] && a->proj[g], "pwv_wavenet_stack_persist_f32: NULL buffer for net %d", g);
        p.ring[g] = a->x_ring[g];
        p.packed[g] = a->packed_layers[g];
        p.proj[g] = a->proj[g];
    }
    if (a->status) p.status = a->status;      // the caller's own sticky word (pwv_status_words_alloc): concurrent callers stay apart
    else PWV_CHECK_HIP(pwv_persist_status(&p.status) == PWV_OK ? hipSuccess : hipErrorUnknown);
    PWV_CHECK_ARG(a->ring_stride >= (size_t)pl.units * 2048 && a->ring_stride % 4 == 0,
                  "pwv_wavenet_stack_persist_f32: ring_stride smaller than one tile32 buffer (%lld floats)", (long long)pl.units * 2048);
    p.ring_stride = (long long)a->ring_stride;
    p.packed_stride = (long long)a->packed_layer_stride;
    p.proj_row_stride = a->proj_row_stride;
    p.G = a->G;
    p.N = varlen ? 1 : a->N;                   // (a packed batch is one run of R rows to everything but unit_rows_varlen)
    p.T = varlen ? (int)a->varlen_rows : a->T;
    p.unit_map = varlen ? a->unit_map : nullptr;
    p.cu_rows = ragged ? a->cu_rows : nullptr;
    p.n_layers = a->n_layers;
    p.units = pl.units;
    p.per_wg = pl.per_wg;
    p.nwg = pl.nwg;
    p.last_wg = pl.last_wg;
    p.reach_wgs = pl.reach_wgs;
    p.xcd_map = pl.xcd_map;
    // Ring stores that no other workgroup reads are plain (the line stays in the XCD's L2 for the next layer's loads) -- as long as a
    // layer's rows FIT the L2s (8 x 4 MB).  Beyond that the lines are evicted before they are re-read anyway, and what is still
    // dirty when the launch ends (dead data: the ring is scratch) is written back between this launch and the next one: all
    // write-through measures -0.8 % / -0.2 % on C3 on two boxes (82 MB per layer), -0.2 % on C4, but +5 % on C1 and level at 16000 rows
    // (4 - 8 MB per layer) (profiles/r05_ab_experiments.md, r05_h / r05_i).  Same bits either way.
    p.all_wt = launch_rows(a) * a->G * 256 > (32ll << 20) ? 1 : 0;
    PWV_CHECK_ARG(a->ring_rotation >= 0 && a->ring_rotation < 3, "pwv_wavenet_stack_persist_f32: ring_rotation must be 0, 1 or 2");
    p.rot = a->ring_rotation;
    p.cond_hop = a->cond_hop;
    p.cond_offset = a->cond_offset;
    p.cond_frames = a->cond_frames;
    make_magic((unsigned)p.T, p.T_magic, p.T_shift);
    make_magic((unsigned)(a->cond_hop > 0 ? a->cond_hop : 1), p.hop_magic, p.hop_shift);
    for (int j = 0; j < a->n_layers; ++j) p.dil[j] = a->dilations[j];
    p.x_first = a->x_first;
    if (a->x_first) {
        for (int g = 0; g < a->G; ++g) {
            PWV_CHECK_ARG(a->causal_filter[g], "pwv_wavenet_stack_persist_f32: x_first needs every net's causal filter");
            p.cfilt[g] = a->causal_filter[g];
        }
        p.x_limit = a->x_limit;
        p.range_flag = a->range_flag;
        for (int g = 0; g < a->G; ++g) p.fold0[g] = a->first_fold[g];
        for (int g = 1; g < a->G; ++g)
            PWV_CHECK_ARG((p.fold0[g] == nullptr) == (p.fold0[0] == nullptr), "pwv_wavenet_stack_persist_f32: first_fold must be set for all nets or for none");
    }
    // the tail: last layer + head (+ affine) behind the run's layers
    p.tail_q = 0;
    if (a->tail_q > 0) {
        for (int g = 0; g < a->G; ++g) {
            PWV_CHECK_ARG(a->tail_layer[g] && a->tail_head[g] && a->tail_out[g], "pwv_wavenet_stack_persist_f32: NULL tail buffer for net %d", g);
            p.tail_layer[g] = a->tail_layer[g];
            p.tail_head[g] = a->tail_head[g];
            p.tail_out[g] = a->tail_out[g];
        }
        p.tail_q = a->tail_q;
        p.tail_dil = a->tail_dilation;
        p.tail_reach_wgs = pl.tail_reach_wgs;
        if (a->affine_x) {
            PWV_CHECK_ARG(a->affine_out && ((a->G == 2 && a->tail_q == 1) || (a->G == 1 && a->tail_q == 2)),
                          "pwv_wavenet_stack_persist_f32: the fused affine needs affine_out and (G = 2, tail_q = 1) or (G = 1, tail_q = 2)");
            p.affine_x = a->affine_x;
            p.affine_out = a->affine_out;
            p.pair = pair_words;
        }
    } else {
        PWV_CHECK_ARG(!a->affine_x, "pwv_wavenet_stack_persist_f32: affine_x without a tail");
    }
    (void)pair_words;
    // the sessions' histories: every history of the launch inside a block (the layers' dilations are the plan's, checked above)
    if (streaming) {
        p.hist_rd = sa.hist_rd;
        p.hist_wr = sa.hist_wr;
        p.slot_tab = sa.slot_tab;
        p.hist_block_stride = (long long)sa.block_stride;
        p.hist_scalar_off = (long long)sa.scalar_off;
        PWV_CHECK_ARG(!a->x_first || sa.scalar_off + (size_t)a->dilations[0] + 1 <= sa.block_stride,
                      "pwv_wavenet_stack_persist_f32: hist->scalar_off + dilation + 1 scalars leave the history block");
        const int n_hist = a->n_layers + (a->tail_q > 0 ? 1 : 0);
        for (int g = 0; g < a->G; ++g)
            for (int j = a->x_first ? 1 : 0; j < n_hist; ++j) {
                const size_t off = a->hist_row_off[g][j];
                const size_t hist_rows = ((size_t)(j < a->n_layers ? a->dilations[j] : a->tail_dilation) + 31) / 32 * 32;
                PWV_CHECK_ARG(off % 4 == 0 && off + hist_rows * 64 <= sa.block_stride,
                              "pwv_wavenet_stack_persist_f32: hist_row_off[%d][%d] + round32(dilation) rows leave the history block", g, j);
                p.hist_off[g][j] = (long long)off;
            }
    }
    p.trace = nullptr;
#ifdef PWV_PTRACE
    { const char* e = getenv("PWV_PTRACE_PTR"); if (e) p.trace = (long long*)strtoull(e, nullptr, 0); }
    p.trace_ev = nullptr;
    { const char* e = getenv("PWV_PTRACE_EV_PTR"); if (e) p.trace_ev = (long long*)strtoull(e, nullptr, 0); }
#endif
    hipStream_t s = (hipStream_t)stream;
    const size_t n16 = r.lay.total / 16;      // (progress words, abort / exit line, pair counters)
    if (!a->workspace_clean)
        hipLaunchKernelGGL(persist_zero_kernel, dim3((unsigned)((n16 + 255) / 256)), dim3(256), 0, s, (int4*)a->workspace, n16);
    const dim3 grid(a->G * pl.nwg), block(512);
    const persist_kernel_t kernel = (ragged ? kRagged : streaming ? kStreaming : varlen ? kPacked : kUniform)[a->precision == PWV_PREC_F32][pl.unit_mode == 2];
    hipLaunchKernelGGL(kernel, grid, block, 0, s, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(PWV_EHIP, "persistent stack kernel launch failed: %s", hipGetErrorString(e));
    return PWV_OK;
}

int pwv_varlen_unit_map(const int* cu_rows, const int* cu_frames, int n_utt, int units, int* out, pwv_stream_t stream) {
    PWV_CHECK_ARG(cu_rows && out, "pwv_varlen_unit_map: NULL argument");
    PWV_CHECK_ARG(n_utt >= 1 && units >= 1, "pwv_varlen_unit_map: n_utt = %d, units = %d", n_utt, units);
    PWV_CHECK_ARG(((uintptr_t)out & 15) == 0, "pwv_varlen_unit_map: out must be 16-byte aligned");
    hipLaunchKernelGGL(varlen_unit_map_kernel, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, (hipStream_t)stream, cu_rows, cu_frames, n_utt, units, out);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(PWV_EHIP, "pwv_varlen_unit_map launch failed: %s", hipGetErrorString(e));
    return PWV_OK;
}

}  // extern "C"
