// Persistent kernel, part 1: geometry and memory.  The workgroup's (net, range), the row maps, the LDS control pointers, the first two
// layers' weights, the ring and P descriptors, the history look-back / store of the streaming forms and the row loaders.
// Expects: F32, MODE, VARLEN, STREAM, p.
// Defines: SHORT, RAGGED, stat, loader_mode, lds, tid, lane, wave, h, net, w, rows, u_begin, u_end, n, L, ctl, lb, prog_n, uprog_n, proj_n,
//          packed_n, ring_rs, proj_rs, proj_rs_at; rows_of, rows_of_top, top_rec, top_scalar, p_base, unit_rec, session_end, dil_of, dil_next,
//          fill_slot, in_soff, out_soff, toff, hist_lookback, hist_store, load_x, load_xc, load_xb.
    constexpr bool SHORT = MODE == 2;      // progress words per unit, stationary units, loader wave, ... (everything below that says SHORT)
    __shared__ __attribute__((aligned(16))) float lds[kLdsFloats];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = lane >> 5;

    // block -> (net, range).  Observed, for speed only: block b runs on XCD b % 8 -- consecutive ranges of a net go to
    // blocks of one XCD, so most neighbour traffic stays inside one L2.  Nothing depends on it.
    int net, w;
    if (p.xcd_map) {
        const int x = blockIdx.x & 7, s = blockIdx.x >> 3;
        net = s % p.G;
        w = x * (p.nwg >> 3) + s / p.G;
    } else {
        net = blockIdx.x % p.G;
        w = blockIdx.x / p.G;
    }
    const int rows = p.N * p.T;
    // (row, utterance, time) of this lane's row of `unit` -- with VARLEN `nn` is the first condition frame of the lane's utterance, so
    // that p_base(nn) is the first P row of the utterance either way
    auto rows_of = [&](int unit, int& row, bool& valid, int& rc, int& nn, int& t) {
        if constexpr (VARLEN) unit_rows_varlen(p.unit_map, unit, lane, rows, row, valid, rc, nn, t);
        else unit_rows(unit, lane, rows, p.N, p.T, p.T_magic, p.T_shift, row, valid, rc, nn, t);
    };
    // the per-layer dilations live in one VGPR (lane j holds entry j), read with v_readlane: a dynamically indexed kernel
    // argument is a scalar LOAD plus a wait each time.  The general loop keeps the scalars of the P row's address in the lanes behind
    // them: left as kernel arguments they are loop-invariant values the register allocator has no SGPR for, and it rematerialises them
    // as scalar loads, each with its own wait, in front of the P loads of EVERY unit (tests/test_persist_top_isa.py)
    constexpr int kLaneStride = kMaxPLayers, kLaneHopMagic = kMaxPLayers + 1, kLaneHopShift = kMaxPLayers + 2, kLaneCondOffset = kMaxPLayers + 3,
                  kLaneCondFrames = kMaxPLayers + 4;
    static_assert(kMaxPLayers + 5 <= 64, "the dilations and the P row's scalars share one VGPR");
    int v_dil = p.dil[lane & (kMaxPLayers - 1)];
    if constexpr (!SHORT) {
        const int k = lane - kMaxPLayers;
        const int c = k == 0 ? p.proj_row_stride : (k == 1 ? (int)p.hop_magic : (k == 2 ? (int)p.hop_shift : (k == 3 ? p.cond_offset : p.cond_frames)));
        v_dil = k >= 0 ? c : v_dil;
    }
    auto dil_of = [&](int j) -> int { return __builtin_amdgcn_readlane(v_dil, j); };
    auto top_scalar = [&](int k) -> int { return __builtin_amdgcn_readlane(v_dil, k); };
    (void)top_scalar;
    auto p_base = [&](int nn) -> int {
        if constexpr (VARLEN) return nn;
        else if constexpr (SHORT) return nn * p.cond_frames;
        else return nn * top_scalar(kLaneCondFrames);
    };
    // RAGGED (VARLEN && STREAM: sessions of different chunk lengths in one packed launch).  The streaming code needs two things the packed
    // row mapping does not hand out: the lane's session INDEX (slot_tab is indexed by it; `nn` is a frame base here) and the END of the
    // lane's session, since "the chunk's last d rows" are the session's own: with k = t + d - T_n and t = rc - start, T_n = end - start,
    // k = rc + d - end.  Both come from the unit's record (scalar loads, the ones unit_rows_varlen makes): the first session of the unit
    // is rec[0] and ends at rec[3]; a lane at or behind that row is in session rec[0] + 1 (a session has >= 32 rows: a unit spans at most
    // two), whose end is cu_rows[rec[0] + 2] -- a scalar load too, made only where the unit does span two sessions.
    constexpr bool RAGGED = VARLEN && STREAM;
    auto unit_rec = [&](int unit, int& s0, int& r1) {
        typedef const __attribute__((address_space(4))) int* const_ints_t;
        const int last = (rows - 1) >> 5;
        const const_ints_t rec = (const_ints_t)(p.unit_map + (size_t)(unit < last ? unit : last) * kVarlenRec);
        s0 = rec[0];
        r1 = rec[3];
    };
    auto session_end = [&](int s0, int r1, bool second) -> int {
        return second ? p.cu_rows[s0 + 2] : r1;      // (per lane, under the caller's fence; the load's address is made there and not kept)
    };
    (void)unit_rec;
    (void)session_end;
    const int u_begin = w * p.per_wg;
    const int u_end = u_begin + p.per_wg < p.units ? u_begin + p.per_wg : p.units;
    const int n = u_end - u_begin;
    if (n <= 0) return;      // owns nothing; nobody waits for it (the neighbour sets stop at the last owning workgroup)
    const int L = p.n_layers;
    constexpr bool stat = SHORT;                        // stationary units (below, at the task loop): n <= kUnitModeMaxPerWg <= 8 units, one per wave
    constexpr bool loader_mode = SHORT;                 // ... leave wave 7 idle (n <= kUnitModeMaxPerWg = 7): it is the workgroup's loader
#ifdef PWV_PTRACE
    int pt_nev = 0;
#endif

    typedef __attribute__((address_space(3))) int* lds_ints_t;
    const lds_ints_t ctl = (lds_ints_t)(lds + kCtlF);
    // (an LDS-address-space pointer: through a generic one the byte accesses become flat_load / flat_store and count on vmcnt)
    typedef __attribute__((address_space(3))) volatile unsigned char* lds_bytes_t;
    const lds_bytes_t lb = (lds_bytes_t)lds;
    int* prog_n = p.prog + (size_t)net * p.nwg * kProgStride;
    int* uprog_n = p.uprog + (size_t)net * p.units * kUnitStride;
    const float* const proj_n = p.proj[net];
    const float* const packed_n = p.packed[net];
    // the layer that reads layer j's rows next: j + 1 of this launch, the tail's layer behind the last one, else (another launch
    // follows: anything) its own
    auto dil_next = [&](int j) -> int { return j + 1 < L ? dil_of(j + 1) : (p.tail_q > 0 ? p.tail_dil : dil_of(j)); };

    // ---- control state, then the weights of the first two layers (LDS-DMA, packed order == LDS order) -------------------
    for (int k = tid; k < (kLdsFloats - kCtlF); k += 512) ctl[k] = 0;
    __syncthreads();
    if (tid == 0) {
        lb[kSeenLB] = w > 0 ? 0 : 255;
        lb[kSeenRB] = w < p.last_wg ? 0 : 255;
        lb[kWreadyB] = 0;
        lb[kWreadyB + 1] = 1;
        lb[kTrueB] = 255;
    }
    auto fill_slot = [&](int slot, int layer, int first, int step) {
        const float* src = packed_n + (size_t)layer * p.packed_stride + lane * 4;
        float* dst = lds + slot * kSlot;
        if constexpr (!SHORT) {
            // (general loop: the refill as BUFFER loads to LDS.  A global_load ... lds is a FLAT-encoded instruction that touches LDS and memory, and while the
            //  compiler knows of one in flight it turns every vector-memory wait it places into vmcnt(0); it never learns that the refill has landed -- the
            //  drains of this loop are inline asm -- so with the global form no load of the task loop is ever left in flight across a compiler's wait:
            //  tests/test_persist_top_isa.py.  Same bytes to the same LDS addresses: lane l's 16 bytes go to the chunk's base + 16 l either way.)
            const __amdgpu_buffer_rsrc_t prs = __builtin_amdgcn_make_buffer_rsrc((void*)(packed_n + (size_t)layer * p.packed_stride), 0, (kSlotFull + 64) * 4, 0x00020000);
#pragma clang loop unroll(disable)
            for (int c = first; c < kSlot / 256; c += step)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(prs, (lptr_t)(dst + c * 256), 16, lane * 16, c * 1024, 0, 0);
            if (first == 0 && lane < 16) __builtin_amdgcn_raw_ptr_buffer_load_lds(prs, (lptr_t)(lds + kBiasF + slot * 64), 16, lane * 16, kSlotFull * 4, 0, 0);
            return;
        }
#pragma clang loop unroll(disable)
        for (int c = first; c < kSlot / 256; c += step)
            __builtin_amdgcn_global_load_lds((gptr_t)(src + c * 256), (lptr_t)(dst + c * 256), 16, 0, 0);
        if (first == 0 && lane < 16)      // dense bias [2 h][32]
            __builtin_amdgcn_global_load_lds((gptr_t)(src + kSlotFull), (lptr_t)(lds + kBiasF + slot * 64), 16, 0, 0);
    };
    if (p.x_first && tid < 128) lds[kCfF + tid] = p.cfilt[net][tid];
    fill_slot(0, 0, wave, 8);
    if (L > 1) fill_slot(1, 1, wave, 8);
    __syncthreads();
    if (wave >= 4) __builtin_amdgcn_s_setprio(1);

    // ONE buffer descriptor for the three ring buffers (they are one allocation); the buffer of a layer is selected by the
    // scalar offset operand of the load / store.  sc1 loads: L2-served, never the CU's L1.
    const __amdgpu_buffer_rsrc_t ring_rs = [&]() {
        const unsigned long long a = (unsigned long long)p.ring[net];
        const unsigned long long span = (unsigned long long)p.ring_stride * 8ull + (unsigned long long)p.units * 8192ull;
        const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a), hi2 = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
        return __builtin_amdgcn_make_buffer_rsrc((void*)(((unsigned long long)hi2 << 32) | lo), 0, __builtin_amdgcn_readfirstlane((unsigned)span), 0x00020000);
    }();
    const __amdgpu_buffer_rsrc_t proj_rs = [&]() {      // (SHORT: the P rows through a buffer descriptor)
        const unsigned long long a = (unsigned long long)proj_n;
        const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a), hi2 = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
        return __builtin_amdgcn_make_buffer_rsrc((void*)(((unsigned long long)hi2 << 32) | lo), 0, 0xFFFFFFFFu, 0x00020000);
    }();
    (void)proj_rs;
    // (the general loop: a descriptor that starts `floats` -- wave-uniform: the unit's FIRST P row -- behind proj_n.  Its 32-bit offsets then span the
    //  P rows of one unit and never the whole of P, which a long batch takes past the 4 GB a descriptor reaches)
    auto proj_rs_at = [&](long long floats) -> __amdgpu_buffer_rsrc_t {
        return __builtin_amdgcn_make_buffer_rsrc((void*)(proj_n + floats), 0, 0xFFFFFFFFu, 0x00020000);
    };
    (void)proj_rs_at;
    const int slot_bytes = (int)(p.ring_stride * 4);
    // (RAGGED: the rotation is pinned in a register of its own.  Left as a kernel argument it is merged into a 16-byte scalar load that the general
    //  instantiations' register allocation marks for a spill slot and then rematerialises: no spill code, but 20 bytes of scratch reserved per lane)
    int rot_pinned = 0;
    if constexpr (RAGGED) {
        rot_pinned = p.rot;
        asm volatile("" : "+s"(rot_pinned));
    }
    auto rot_of = [&]() -> int {
        if constexpr (RAGGED) return rot_pinned;
        else return p.rot;
    };
    auto in_soff = [&](int j) -> int { return ((j + 2 + rot_of()) % 3) * slot_bytes; };
    auto out_soff = [&](int j) -> int { return ((j + rot_of()) % 3) * slot_bytes; };
    auto toff = [&](int row) -> int { return ((row >> 5) * 2048 + h * 128 + (row & 31) * 4) * 4; };
    // STREAM, boundary units only (64-bit global addresses: the histories are another allocation, and slots x 2 blocks pass 4 GB)
    // look-back from the history: lanes with t < d overwrite xb with row t of layer `jh`'s row history in the block their session reads
    // (RAGGED: `unit` and `rc` give the lane's session index, made under the same branches)
    auto hist_lookback = [&](int jh, int d, int nn, int t, int unit, int rc, float (&xb)[32]) {
        if constexpr (STREAM) {
            if (!__all(t >= d)) {
                int sn = nn;
                if constexpr (RAGGED) {
                    int s0, r1, uu = unit;
                    asm volatile("" : "+s"(uu));      // (the record is read HERE, for the boundary units: not hoisted into the unit loop's live ranges)
                    unit_rec(uu, s0, r1);
                    sn = s0 + (rc >= r1 ? 1 : 0);
                }
                if (t < d) {
                    const float* hr = p.hist_rd + (long long)p.slot_tab[2 * sn] * p.hist_block_stride + p.hist_off[net][jh] + tile_off(t, h, 64);
#pragma unroll
                    for (int g = 0; g < 8; ++g) {
                        const f32x4 v = *reinterpret_cast<const f32x4*>(hr + g * 256);
#pragma unroll
                        for (int e = 0; e < 4; ++e) xb[4 * g + e] = v[e];
                    }
                }
            }
        }
    };
    // history store: lanes with t >= T - d store their row of layer `jh`'s input to row t + d - T of the block their session writes
    // (RAGGED: T is the lane's session's own T_n, k = rc + d - the session's end.  The fence needs no load beyond the unit's record: a lane of
    //  the unit's first session stores iff it lies within d rows of rec[3]; a unit with a lane of a second session is a boundary unit anyway)
    // (`r1_top` >= 0: the end of the unit's first session as the caller already holds it -- the general loop's top_rec -- instead of a read of the record)
    auto hist_store = [&](int jh, int d, int nn, int t, int unit, int rc, bool valid, const float (&xr)[32], int r1_top = -1) {
        if constexpr (RAGGED) {
            int s0 = 0, r1 = r1_top;
            if (r1_top < 0) unit_rec(unit, s0, r1);
            (void)s0;
            const bool second = rc >= r1;
            int k = rc + d - r1;                        // (a lane of the unit's first session)
            if (__any(valid && (second || k >= 0))) {
                // (per-lane loads from here on: the unit loop keeps no scalar of this branch)
                int lo = second ? 1 : 0;
                asm volatile("" : "+v"(lo));
                const int last = (rows - 1) >> 5;
                const int sn = p.unit_map[(size_t)(unit < last ? unit : last) * kVarlenRec] + lo;
                k = rc + d - p.cu_rows[sn + 1];
                if (valid && k >= 0) {
                    float* hw = p.hist_wr + (long long)p.slot_tab[2 * sn + 1] * p.hist_block_stride + p.hist_off[net][jh] + tile_off(k, h, 64);
#pragma unroll
                    for (int g = 0; g < 8; ++g) {
                        const f32x4 v = {xr[4 * g], xr[4 * g + 1], xr[4 * g + 2], xr[4 * g + 3]};
                        *reinterpret_cast<f32x4*>(hw + g * 256) = v;
                    }
                }
            }
        } else if constexpr (STREAM) {
            const int k = t + d - p.T;
            if (__any(valid && k >= 0)) {
                if (valid && k >= 0) {
                    float* hw = p.hist_wr + (long long)p.slot_tab[2 * nn + 1] * p.hist_block_stride + p.hist_off[net][jh] + tile_off(k, h, 64);
#pragma unroll
                    for (int g = 0; g < 8; ++g) {
                        const f32x4 v = {xr[4 * g], xr[4 * g + 1], xr[4 * g + 2], xr[4 * g + 3]};
                        *reinterpret_cast<f32x4*>(hw + g * 256) = v;
                    }
                }
            }
        }
    };

    // x[t-d] / x[t] rows of one unit -> registers
    // (packed batches, general loop: the record of the unit whose rows load_x requested last -- every unit of the task loop has its rows requested by
    //  load_x before its top runs, so the top maps its rows from these four scalars instead of reading the record a second time: a scalar load and
    //  its wait on the address path of the P row, in every unit)
    int top_rec[4] = {0, 0, 0, 0};
    auto rows_of_top = [&](int unit, int& row, bool& valid, int& rc, int& nn, int& t) {
        if constexpr (VARLEN && !SHORT) unit_rows_from_record(top_rec, unit, lane, rows, row, valid, rc, nn, t);
        else rows_of(unit, row, valid, rc, nn, t);
    };
    (void)rows_of_top;
    auto load_x = [&](int j, int unit, float (&xb)[32], float (&xc)[32]) {
        int row, rc, nn, t;
        bool valid;
        if constexpr (VARLEN && !SHORT) {
            unit_record_varlen(p.unit_map, unit, rows, top_rec);
            unit_rows_from_record(top_rec, unit, lane, rows, row, valid, rc, nn, t);
        } else {
            rows_of(unit, row, valid, rc, nn, t);
        }
        const int d = dil_of(j);
        const bool has_prev = t >= d;
        if (p.x_first && j == 0) {
            // layer 0 of the net: the four scalars its two rows are functions of (x[t], x[t-1], x[t-d], x[t-d-1]; zero left of
            // the utterance start); rebuilt into rows at the top of the unit (layer_f16x3_kernel's FIRST variant)
            const float* x1 = p.x_first;
            xc[0] = x1[rc];
            xc[1] = t >= 1 ? x1[rc - (t >= 1 ? 1 : 0)] : 0.f;
            xb[0] = has_prev ? x1[rc - (has_prev ? d : 0)] : 0.f;
            xb[1] = t >= d + 1 ? x1[rc - (t >= d + 1 ? d + 1 : 0)] : 0.f;
#pragma unroll
            for (int k = 2; k < 32; ++k) xb[k] = xc[k] = 0.f;      // (every element written on every path: the arrays stay in registers)
            return;
        }
        const int so = in_soff(j);
        const int oc = toff(rc), ob = toff(has_prev ? rc - d : rc);
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            const f32x4 v = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(ring_rs, oc + g * 1024, so, 16));
#pragma unroll
            for (int e = 0; e < 4; ++e) xc[4 * g + e] = v[e];
        }
        // ONE load sequence for the look-back row; units at an utterance start (rare) zero their lanes IN PLACE behind it, under a wave-uniform
        // branch.  (Two sequences -- a plain one for __all(has_prev), one with the select -- had the compiler share the first chunk's load between
        // them and join the two results in another register than the one it is loaded into: `s_waitcnt vmcnt(7)` + a v_mov_b32 on the FAST path, i.e.
        // every unit stalled in front of GEMM2 until its successor's own rows and that chunk had arrived; tests/test_persist_prefetch_isa.py.)
        // The fast path has no instruction behind the loads: they stay in flight.
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            const f32x4 v = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(ring_rs, ob + g * 1024, so, 16));
#pragma unroll
            for (int e = 0; e < 4; ++e) xb[4 * g + e] = v[e];
        }
        if (!__all(has_prev)) {
#pragma unroll
            for (int k = 0; k < 32; ++k) xb[k] = has_prev ? xb[k] : 0.f;
        }
        hist_lookback(j, d, nn, t, unit, rc, xb);
    };

    // the unit's own rows alone (stationary units: once, in front of the task loop)
    auto load_xc = [&](int j, int unit, float (&xc)[32]) {
        int row, rc, nn, t;
        bool valid;
        rows_of(unit, row, valid, rc, nn, t);
        const int so = in_soff(j);
        const int oc = toff(rc);
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            const f32x4 v = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(ring_rs, oc + g * 1024, so, 16));
#pragma unroll
            for (int e = 0; e < 4; ++e) xc[4 * g + e] = v[e];
        }
    };
    // the look-back row alone (stationary units, layers >= 1)
    auto load_xb = [&](int j, int unit, float (&xb)[32]) {
        int row, rc, nn, t;
        bool valid;
        rows_of(unit, row, valid, rc, nn, t);
        const int d = dil_of(j);
        const bool has_prev = t >= d;
        const int so = in_soff(j);
        const int ob = toff(has_prev ? rc - d : rc);
        // (no select here: rows left of the utterance start are zeroed where the row is USED -- a select, or two paths that the register
        //  allocator joins with copies, behind these loads is a wait for them right here)
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            const f32x4 v = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(ring_rs, ob + g * 1024, so, 16));
#pragma unroll
            for (int e = 0; e < 4; ++e) xb[4 * g + e] = v[e];
        }
        hist_lookback(j, d, nn, t, unit, rc, xb);      // (STREAM: rows left of the chunk are the history's -- and are not zeroed where the row is used)
    };
