// The body of the persistent flow kernels (pwv_stack_persist.hip): stack_persist_kernel<F32, MODE, VARLEN, STREAM> and
// stack_persist_ragged_kernel<F32, MODE> (VARLEN and STREAM both on) include it -- an include, not a shared __device__ function:
// a function moves the register allocation of the instantiations that exist, an include leaves their instruction streams alone
// (as pwv_layer_f16x3_body.inc between the one-shot and the streaming layer kernels).  Expects F32, MODE, VARLEN, STREAM and `p`.
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
    auto p_base = [&](int nn) -> int {
        if constexpr (VARLEN) return nn;
        else return nn * p.cond_frames;
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
    // the per-layer dilations live in one VGPR (lane j holds entry j), read with v_readlane: a dynamically indexed kernel
    // argument is a scalar LOAD plus a wait each time
    const int v_dil = p.dil[lane & (kMaxPLayers - 1)];
    auto dil_of = [&](int j) -> int { return __builtin_amdgcn_readlane(v_dil, j); };
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
    auto hist_store = [&](int jh, int d, int nn, int t, int unit, int rc, bool valid, const float (&xr)[32]) {
        if constexpr (RAGGED) {
            int s0, r1;
            unit_rec(unit, s0, r1);
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
    auto load_x = [&](int j, int unit, float (&xb)[32], float (&xc)[32]) {
        int row, rc, nn, t;
        bool valid;
        rows_of(unit, row, valid, rc, nn, t);
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

    // ---- dependencies: lane k < 6 of a wave looks at ONE byte of LDS ------------------------------------------------------
    //   k = 0: own x[t] rows, 1 / 2: the x[t-d] rows (units u - ceil(d/32), u - floor(d/32)), 3: this layer's weights resident,
    //   4 / 5: the readers of the ring slot the task overwrites (layer j-2's tasks of the units u + floor(d'/32), u + ceil(d'/32)).
    // Per layer: the unit offsets and the values the bytes must have reached (two VGPRs); per task: one address VGPR.
    int vpack = 0;                     // need << 16 | (unit offset & 0xffff)
    auto layer_vectors = [&](int j) {
        const int d = dil_of(j), d2 = dil_of(j >= 2 ? j - 2 : 0);
        const int off = lane == 1 ? -((d + 31) >> 5) : (lane == 2 ? -(d >> 5) : (lane == 4 ? (d2 >> 5) : (lane == 5 ? ((d2 + 31) >> 5) : 0)));
        const int raw = j >= 1 ? j : 0, wts = j >= 2 ? j : 0, war = j >= 2 ? j - 1 : 0;
        const int need = lane < 3 ? raw : (lane == 3 ? wts : (lane < 6 ? war : 0));
        vpack = (need << 16) | (off & 0xffff);
    };
    auto dep_addr = [&](int j, int u) -> int {
        const int v = u + (int)(short)vpack;
        int a = kDoneB - u_begin + v;
        a = (v < u_begin && !SHORT) ? kSeenLB : a;      // (unit mode: the byte of that very unit, kLeftN bytes in front of the own ones)
        a = v >= u_end ? kSeenRB : a;
        a = (v < 0 || v >= p.units) ? kTrueB : a;
        a = lane == 3 ? kWreadyB + (j & 1) : a;
        return lane >= 6 ? kTrueB : a;
    };
    // bit k set: dependency k is NOT yet satisfied
    auto eval = [&](int addr) -> unsigned { return (unsigned)__ballot((int)lb[addr] < (vpack >> 16)); };
    // neighbours' progress words -> the cached "seen" byte of that side (only ever raised to a value that was observed)
    auto wave_min = [&](int v) -> int {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) { const int t = __shfl_xor(v, o); v = t < v ? t : v; }
        return v;
    };
    // (round 6: the byte takes the value that was OBSERVED, not just `need` -- a neighbour is usually a layer further on than what is
    //  asked for, and a poll is a 1.5 us round trip to the fabric for a word another CU wrote through)
    auto poll_side = [&](int side, int need) {
        const int w0 = side ? w + 1 : (w - p.reach_wgs > 0 ? w - p.reach_wgs : 0);
        const int cnt = side ? (w + p.reach_wgs < p.last_wg ? p.reach_wgs : p.last_wg - w) : w - w0;
        int v = 255;
        int lo = lane;
        asm volatile("" : "+v"(lo));      // (address made here, not hoisted out of the task loop into a spilled register pair)
        if (lo < cnt) v = __hip_atomic_load(prog_n + (size_t)(w0 + lo) * kProgStride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if constexpr (SHORT) {
            const int m = wave_min(v);
            if (m >= need) lb[side ? kSeenRB : kSeenLB] = (unsigned char)m;
        } else {
            if (__ballot(v < need) == 0) lb[side ? kSeenRB : kSeenLB] = (unsigned char)need;
        }
    };
    // unit mode: lanes 1 / 2 ask for exactly the unit they wait for (own 128-byte line each), lanes 32.. for the right neighbours'
    // workgroup words in the same instruction (the WAR side's byte is refreshed on the way, so the top unit's stores rarely have to poll)
    auto poll_units = [&](int addr, int jw) {
        const int cnt_r = w + p.reach_wgs < p.last_wg ? p.reach_wgs : p.last_wg - w;
        int lo = lane;
        asm volatile("" : "+v"(lo));      // (the addresses are made HERE: hoisted out of the task loop as loop-invariant per-lane pointers they are spilled registers)
        const bool left = (lo == 1 || lo == 2) && addr >= kLeftB && addr < kDoneB;
        int v = 255;
        if (left) {
            v = __hip_atomic_load(uprog_n + (size_t)(u_begin - kLeftN + addr - kLeftB) * kUnitStride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else if (lo >= 32 && lo - 32 < cnt_r) {
            v = __hip_atomic_load(prog_n + (size_t)(w + 1 + lo - 32) * kProgStride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        v = v > 255 ? 255 : v;
        if (left) lb[addr] = (unsigned char)v;
        // (the right neighbours are normally at layer jw or one further: two ballots instead of a reduction)
        if (cnt_r > 0) {
            const bool r = lo >= 32;
            if (__ballot(r && v < jw + 1) == 0) lb[kSeenRB] = (unsigned char)(jw + 1);
            else if (__ballot(r && v < jw) == 0 && (int)lb[kSeenRB] < jw) lb[kSeenRB] = (unsigned char)jw;
        }
    };

    // what this wave owes the others: the unit it has just stored and a weight refill it has issued (true at a vmcnt(0))
    int prev_addr = -1, prev_j = 0;      // LDS byte of the unit stored last, its layer
    int dma_pending = -1;                // layer whose LDS-DMA this wave issued and has not yet announced
    int left_upto = 0;                   // layers [0, left_upto) this wave has counted itself out of
    bool dead = false;
    auto publish = [&]() {               // (all lanes store the same byte: no exec juggling)
        if (prev_addr >= 0) {
            lb[prev_addr] = (unsigned char)(prev_j + 1);
            if (SHORT && lane == 0) __hip_atomic_store(uprog_n + (size_t)(prev_addr - kDoneB + u_begin) * kUnitStride, prev_j + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            prev_addr = -1;
        }
        if (dma_pending >= 0) { lb[kWreadyB + (dma_pending & 1)] = (unsigned char)dma_pending; dma_pending = -1; }
    };
    auto flush_owed = [&]() {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        publish();
    };
    // leaving layer jj (after a drain: this wave's layer-jj stores are complete).  The LAST of the 8 waves publishes the
    // workgroup's progress and refills the LDS slot with layer jj + 2.
    auto leave_layers = [&](int upto) {
        for (; left_upto < upto; ++left_upto) {
            const int jj = left_upto;
            int old = 0;
            if (lane == 0) old = __hip_atomic_fetch_add(&ctl[8 + jj], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            old = __builtin_amdgcn_readfirstlane(old);
            if (old == 7 && !loader_mode) {
                if (lane == 0) __hip_atomic_store(prog_n + (size_t)w * kProgStride, jj + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                PT_EV(7, jj, -1);
                if (jj + 2 < L) {
                    if (dma_pending >= 0) flush_owed();       // (last twice in a row: announce the earlier refill first)
                    fill_slot(jj & 1, jj + 2, 0, 1);
                    dma_pending = jj + 2;
                }
            }
        }
    };
    // bounded wait for the dependencies `mask` of task (j, u) (rare: everything a task needs is normally a layer old);
    // `lv` = the layer vpack describes on entry and again on return
    auto wait_deps = [&](int j, int u, unsigned mask, int lv, int code) {
        // never spin while holding unpublished work -- and "work" includes leaving the layers this wave has moved past: with few
        // units per workgroup a wave's next task can be two layers on, and the weights it then waits for are refilled by the
        // LAST wave to leave the layer it has just finished
        if (!SHORT || prev_addr >= 0 || dma_pending >= 0) {
            flush_owed();
            PT_EV(mask == kWarMask ? 13 : 3, j, u);
        }
        leave_layers(j);
        if (dma_pending >= 0) flush_owed();
        if (lv != j) layer_vectors(j);
        const int addr = dep_addr(j, u);
        bool ok = false;
        const long long t0 = __builtin_amdgcn_s_memrealtime();
#ifdef PWV_PTRACE
        unsigned pt_bad0 = 0, pt_badl = 0;
        int pt_polls = 0;
#endif
        for (int k = 0; !ok; ++k) {
            const unsigned bad = eval(addr) & mask;
#ifdef PWV_PTRACE
            if (k == 0) pt_bad0 = bad;
            if (bad) pt_badl = bad;
            pt_polls = k;
#endif
            if (!bad) { ok = true; break; }
            // somebody has given up (this workgroup: LDS word; any workgroup of the launch: the word behind the progress words,
            // looked at every 64th poll), or this wait has lasted 20 ms: give up too.  (readfirstlane: the loop stays wave-uniform)
            if (__builtin_amdgcn_readfirstlane(*(__attribute__((address_space(3))) volatile int*)&ctl[1])) break;
            if ((k & 63) == 63 && (__builtin_amdgcn_readfirstlane(__hip_atomic_load(p.abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) ||
                                   __builtin_amdgcn_s_memrealtime() - t0 > kWaitTicks)) break;
            if constexpr (SHORT) {
                if ((bad & 0x6u) && __ballot((lane == 1 || lane == 2) && addr < kDoneB && addr >= kLeftB)) poll_units(addr, j);
            } else if ((bad & 0x6u) && __ballot(addr == kSeenLB && (lane == 1 || lane == 2))) poll_side(0, j);
            if ((bad & 0x30u) && __ballot(addr == kSeenRB && (lane == 4 || lane == 5))) poll_side(1, j - 1);
            __builtin_amdgcn_s_sleep(4);
        }
        if (lv != j) layer_vectors(lv);
        PT_EV(mask == kWarMask ? 12 : 4, j, (long long)u | ((long long)pt_bad0 << 32) | ((long long)pt_badl << 40) | ((long long)pt_polls << 48));
        if (ok) return;
        // (every lane stores the same words: a lane-0 branch here makes the compiler treat `dead`, and with it the whole
        // task loop, as divergent -- scalar bookkeeping in VGPRs, a waterfall loop around every buffer access)
        __hip_atomic_store(p.status, code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(p.abort, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *(__attribute__((address_space(3))) volatile int*)&ctl[1] = 1;
        dead = true;
    };

    // ---- tasks: index i = layer * n + k, unit = u_end - 1 - k; claimed from the LDS counter one iteration ahead ---------
    auto claim = [&]() -> int {
        int v = 0;
        if (lane == 0) v = __hip_atomic_fetch_add(&ctl[0], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        return v;          // lane 0's value; readfirstlane at the point of use
    };
    auto locate = [&](int i, int& j) -> int {      // j: a layer at or before the task's (tasks are claimed in increasing order)
#pragma clang loop unroll(disable) vectorize(disable)
        while (j < L && i >= (j + 1) * n) ++j;      // (normally zero or one step: keep it a three-instruction scalar loop)
        return j < L ? u_end - 1 - (i - j * n) : -1;
    };
    // STATIONARY units (round 6; unit mode with at most one unit per wave): wave k owns unit u_end - 1 - k in EVERY layer, the other waves
    // have no tasks.  The unit's own rows x[t] then never travel: they are the accumulators the wave has just stored, and what it has to
    // fetch between two layers is the look-back row alone -- half the bytes in the CU's memory queue at the one moment a short layer waits
    // for (a CU loads freshly written rows at ~ 30 GB/s, latency-bound: 2.2 us for its four units' 64 KB; profiles/r06_short_timeline.md).
    int j = 0;
    int u = stat ? (wave < n ? u_end - 1 - wave : -1) : locate(__builtin_amdgcn_readfirstlane(claim()), j);
    int claim_v = stat ? 0 : claim();      // the task after that
    auto next_task = [&](int jc, int uc, int& jn) -> int {
        if (stat) { jn = jc + 1; return jn < L ? uc : -1; }
        return locate(__builtin_amdgcn_readfirstlane(claim_v), jn);
    };
    float rxb[32], rxc[32];
    bool war_ok = true;                    // (of the task in hand; its RAW side is satisfied when it starts)
    PT_DECL
#ifdef PWV_PTRACE
    const long long pt_start = __builtin_amdgcn_s_memtime();
    const long long pt_start_rt = __builtin_amdgcn_s_memrealtime();
    pt_acc[7] = pt_start;
#endif
    // ---- the loader (stationary units with an idle wave): it waits for the n active waves to have left layer jj, publishes the workgroup's
    // progress word and refills the LDS slot with layer jj + 2.  Left to the last wave to leave, as in the general scheme, the 80 KB of LDS-DMA
    // sit in THAT wave's memory queue in front of its next look-back row: 3 us on the top unit of every layer (r06_m timeline).
    if (loader_mode && wave == 7) {
        __builtin_amdgcn_s_setprio(0);      // (it shares its SIMD with an active wave)
        bool gone = false;
        for (int jj = 0; jj < L && !gone; ++jj) {
            const long long t0 = __builtin_amdgcn_s_memrealtime();
            for (int k = 0;; ++k) {
                if (__builtin_amdgcn_readfirstlane(*(__attribute__((address_space(3))) volatile int*)&ctl[8 + jj]) >= n) break;
                if (__builtin_amdgcn_readfirstlane(*(__attribute__((address_space(3))) volatile int*)&ctl[1])) { gone = true; break; }
                if ((k & 63) == 63 && (__builtin_amdgcn_readfirstlane(__hip_atomic_load(p.abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) ||
                                       __builtin_amdgcn_s_memrealtime() - t0 > kWaitTicks)) {
                    __hip_atomic_store(p.status, 7, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    __hip_atomic_store(p.abort, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    *(__attribute__((address_space(3))) volatile int*)&ctl[1] = 1;
                    gone = true;
                    break;
                }
                __builtin_amdgcn_s_sleep(2);
            }
            if (gone) break;
            if (lane == 0) __hip_atomic_store(prog_n + (size_t)w * kProgStride, jj + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            PT_EV(7, jj, -1);
            if (jj + 2 < L) {
                fill_slot(jj & 1, jj + 2, 0, 1);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                lb[kWreadyB + (jj & 1)] = (unsigned char)(jj + 2);
            }
        }
    }
    // ---- layer 0 in its folded form (pwv_persist_args.first_fold), a loop of its own in front of the general one.
    // h[t] = x[t-1] w0 + x[t] w1 (modules.py:179-180) makes filter|gate(h[t-d], h[t]) a [4 -> 128] map of the scalars
    // x[t-d-1], x[t-d], x[t-1], x[t]: ONE split-fp16 MFMA k-step (4 of its 16 k values used) instead of eight -- two fp32
    // k-steps instead of 64 -- with no LDS fragment reads and no operand splits.  Layer 0 depends on nothing inside the launch
    // (its input was complete before it started and the ring slot it writes has no earlier reader), so this loop never waits;
    // tasks are layer-major, so it ends when the wave's next task is a layer-1 one, and the general loop's first-task code
    // takes over.  (As a branch INSIDE the general loop the two accumulator sets cost it 60-80 spilled registers.)
    if (p.x_first && p.fold0[net]) {
        const float* Af = lds;                                                    // layer 0's weights: slot 0
        const f16x8* A2 = reinterpret_cast<const f16x8*>(lds + kA1Size);
        (void)Af;
        (void)A2;
        const float* bias = lds + kBiasF + h * 32;
        const char* F0 = reinterpret_cast<const char*>(p.fold0[net]);
        const float* lastfrag = packed_n + kSlot + lane * 4;
        const int d = dil_of(0);
        const int dn = dil_next(0);
        typedef const __attribute__((address_space(3))) f32x4* lds_f4_t;
        const lds_f4_t cfb = (lds_f4_t)(lds + kCfF + 4 * h);
        // the folded fragments and the dense tail are the same for every unit: registers for the whole loop
        f16x8 fh[4], fl[4];      // split-fp16: [hi | lo][4 row tiles][64 lanes] f16x8
        f32x4 ff[4];             // fp32: [4 row tiles][64 lanes] {k = h, k = 2 + h, 0, 0}
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            if constexpr (F32) {
                ff[it] = *reinterpret_cast<const f32x4*>(F0 + it * 1024 + lane * 16);
            } else {
                fh[it] = *reinterpret_cast<const f16x8*>(F0 + it * 1024 + lane * 16);
                fl[it] = *reinterpret_cast<const f16x8*>(F0 + (4 + it) * 1024 + lane * 16);
            }
        }
        const f32x4 lf32 = *reinterpret_cast<const f32x4*>(lastfrag);      // (16 bytes either way)
        while (u >= 0 && j == 0) {
            int row, rc, nn, t;
            bool valid;
            rows_of(u, row, valid, rc, nn, t);
            // the four scalars (zero left of the utterance start) and the P row
            const float* x1 = p.x_first;
            const bool has_prev = t >= d;
            const float x0 = x1[rc];
            float x1v, xd0, xd1;
            if constexpr (STREAM) {
                // x[t-1], x[t-d], x[t-d-1] with a negative time come from the session's scalar history: time r < 0 is element d + 1 + r
                // (every address a valid one, selected: layer_*_stream_kernel's FIRST form); the chunk's last d + 1 scalars are the next history
                if constexpr (RAGGED) {
                    // (the lane's session index and its own T_n -- k = rc + d + 1 - the session's end -- from the unit's record)
                    int s0, r1;
                    unit_rec(u, s0, r1);
                    const bool second = rc >= r1;
                    const int sn = s0 + (second ? 1 : 0);
                    const float* hx = p.hist_rd + (long long)p.slot_tab[2 * sn] * p.hist_block_stride + p.hist_scalar_off;
                    x1v = *(t >= 1 ? x1 + rc - 1 : hx + d);
                    xd0 = *(has_prev ? x1 + rc - d : hx + t + 1);
                    xd1 = *(t >= d + 1 ? x1 + rc - d - 1 : hx + t);
                    const int k = rc + d + 1 - session_end(s0, r1, second);
                    if (valid && h == 0 && k >= 0) p.hist_wr[(long long)p.slot_tab[2 * sn + 1] * p.hist_block_stride + p.hist_scalar_off + k] = x0;
                } else {
                    const float* hx = p.hist_rd + (long long)p.slot_tab[2 * nn] * p.hist_block_stride + p.hist_scalar_off;
                    x1v = *(t >= 1 ? x1 + rc - 1 : hx + d);
                    xd0 = *(has_prev ? x1 + rc - d : hx + t + 1);
                    xd1 = *(t >= d + 1 ? x1 + rc - d - 1 : hx + t);
                    const int k = t + d + 1 - p.T;
                    if (valid && h == 0 && k >= 0) p.hist_wr[(long long)p.slot_tab[2 * nn + 1] * p.hist_block_stride + p.hist_scalar_off + k] = x0;
                }
            } else {
                x1v = t >= 1 ? x1[rc - (t >= 1 ? 1 : 0)] : 0.f;
                xd0 = has_prev ? x1[rc - (has_prev ? d : 0)] : 0.f;
                xd1 = t >= d + 1 ? x1[rc - (t >= d + 1 ? d + 1 : 0)] : 0.f;
            }
            f32x16 acc[4];
            {
                int prow = 0;
                if (p.cond_hop > 0) prow = p_base(nn) + fast_div(t + p.cond_offset, p.hop_magic, p.hop_shift);
                const float* pr = proj_n + (size_t)prow * p.proj_row_stride + h * 64;
#pragma unroll
                for (int it = 0; it < 4; ++it)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const f32x4 v = *reinterpret_cast<const f32x4*>(pr + it * 16 + q * 4);
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc[it][q * 4 + e] = v[e];
                    }
            }
            int j2 = 0;
            const int u2 = next_task(0, u, j2);
            // drain (the loads above, the previous unit's stores), publish that unit, claim the task after the next
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            publish();
            if (u2 >= 0 && !stat) claim_v = claim();
            if (p.range_flag && !(fabsf(x0) <= p.x_limit)) __hip_atomic_store(p.range_flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            if constexpr (F32) {
                const float b0 = h ? xd0 : xd1, b1 = h ? x0 : x1v;      // k = 0, 1 | k = 2, 3
#pragma unroll
                for (int it = 0; it < 4; ++it) acc[it] = __builtin_amdgcn_mfma_f32_32x32x2f32(ff[it][0], b0, acc[it], 0, 0, 0);
#pragma unroll
                for (int it = 0; it < 4; ++it) acc[it] = __builtin_amdgcn_mfma_f32_32x32x2f32(ff[it][1], b1, acc[it], 0, 0, 0);
            } else {
                f16x8 b_h = {0, 0, 0, 0, 0, 0, 0, 0}, b_l = {0, 0, 0, 0, 0, 0, 0, 0};      // k = 0..3: lanes of the lower half
                const float sc[4] = {xd1, xd0, x1v, x0};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float v = h == 0 ? sc[q] : 0.f;
                    const _Float16 vh = (_Float16)v;
                    b_h[q] = vh;
                    b_l[q] = (_Float16)(v - (float)vh);
                }
#pragma unroll
                for (int it = 0; it < 4; ++it) acc[it] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fh[it], b_h, acc[it], 0, 0, 0);
#pragma unroll
                for (int it = 0; it < 4; ++it) acc[it] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fh[it], b_l, acc[it], 0, 0, 0);
#pragma unroll
                for (int it = 0; it < 4; ++it) acc[it] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fl[it], b_h, acc[it], 0, 0, 0);
            }
            // GEMM2's accumulator starts at h[t] + dense_bias; h[t] with the operations of iaf_front_kernel (same bits as unfolded)
            f32x16 acc2[2];
#pragma unroll
            for (int it = 0; it < 2; ++it)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const f32x4 w0 = cfb[2 * (4 * it + q)];
                    const f32x4 w1 = cfb[16 + 2 * (4 * it + q)];
                    const f32x4 bd = *reinterpret_cast<const f32x4*>(bias + it * 16 + q * 4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc2[it][q * 4 + e] = fmaf(x0, w1[e], x1v * w0[e]) + bd[e];
                }
            float o[32];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                o[r] = gate_act(acc[0][r], acc[2][r]);
                o[16 + r] = gate_act(acc[1][r], acc[3][r]);
            }
            if constexpr (F32) {
                f32x4 a[4];
                a[0] = frag(Af, kA1Size, 0, 8, 0, lane);
                a[1] = frag(Af, kA1Size, 1, 8, 0, lane);
                gemm_groups_dense([&](int it, int g) -> f32x4 { return (it == 1 && g == 7) ? lf32 : frag(Af, kA1Size, it, 8, g, lane); },
                                  acc2, a, [&](int ks) -> float { return o[ks]; }, [](int) {});
            } else {
                const f16x8 lf = __builtin_bit_cast(f16x8, lf32);
                f16x8 ah[4], al[4];
                first_frags<4, 2, 0, 1, 2>(A2, lane, ah, al);
                f16x8 oh[4], ol[4];
                split8<0>(o, oh[0], ol[0]);
                split8<8>(o, oh[1], ol[1]);
                split8<16>(o, oh[2], ol[2]);
                split8<24>(o, oh[3], ol[3]);
                gemm16_dense(
                    [&](int comp, int it, int s) -> f16x8 { return (comp == 1 && it == 1 && s == 3) ? lf : frag16<4, 2>(A2, comp, it, s, lane); },
                    acc2, ah, al, [&](int s) -> f16x8 { return oh[s]; }, [&](int s) -> f16x8 { return ol[s]; }, [](int) {});
            }
            {
                const int so = out_soff(0);
                const int oo = toff(row);
                const bool shared = p.all_wt || u + ((dn + 31) >> 5) >= u_end;      // units the right neighbour reads in layer 1: write-through
                if (valid) {
                    if (shared) {
#pragma unroll
                        for (int g = 0; g < 8; ++g) {
                            const int it = g >> 2, q = g & 3;
                            const f32x4 v = {acc2[it][q * 4], acc2[it][q * 4 + 1], acc2[it][q * 4 + 2], acc2[it][q * 4 + 3]};
                            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), ring_rs, oo + g * 1024, so, kAuxWriteThrough);
                        }
                    } else {
#pragma unroll
                        for (int g = 0; g < 8; ++g) {
                            const int it = g >> 2, q = g & 3;
                            const f32x4 v = {acc2[it][q * 4], acc2[it][q * 4 + 1], acc2[it][q * 4 + 2], acc2[it][q * 4 + 3]};
                            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), ring_rs, oo + g * 1024, so, kStoreAuxLocal);
                        }
                    }
                }
            }
            PT_EV(2, 0, u);
            prev_addr = kDoneB + (u - u_begin);
            prev_j = 0;
            j = j2;
            u = u2;
        }
    }
    if (u >= 0) {
        // the first task of the general loop: nothing was prefetched (after the folded loop: drain and publish its last unit first)
        flush_owed();
        leave_layers(j);
        layer_vectors(j);
        if constexpr (SHORT) {
            // the unit's own rows: this wave's own layer-0 output (stationary units; complete: the drain above) or the run's input
            load_xc(j, u, rxc);
        } else {
            const unsigned bad = eval(dep_addr(j, u));
            if (bad & kRawMask) wait_deps(j, u, kRawMask, j, 4);
            war_ok = (bad & kWarMask) == 0;
            if (!dead) load_x(j, u, rxb, rxc);
        }
    }
    int lv_j = j;                          // layer voff / vneed currently describe

    // SHORT (stationary units): a unit is NOT software-pipelined over the previous one.  Its top: what the previous unit owes (drain, publish), then
    // its P row, then its dependencies, then its look-back row.  The loads are issued and consumed in ONE iteration: across the back-edge the
    // compiler's vmcnt bookkeeping is conservative, and a P row carried over as 64 accumulator registers costs GEMM1 fifty spilled ones.  (The packed
    // K order is x[t] first so that GEMM1 could start on the unit's own rows while the look-back row is in flight -- the "early half" -- which the
    // measurements of round 6 did not reward in any form the compiler or inline asm allows; see the comment at the dependency check below.)
    while (u >= 0 && !dead) {
        PT_MARK();
        // ---- TOP: P row requested; the rows of this unit were requested during the previous one ---------------------------
        int row, rc, nn, t;
        bool valid;
        rows_of(u, row, valid, rc, nn, t);
        if constexpr (SHORT) {
            flush_owed();
            PT_EV(3, j, u);
            leave_layers(j);
        }
        f32x16 acc[4];
        if constexpr (SHORT) {
            // (buffer loads, like the rows: the compiler's scoreboard takes "all but the last 8 loads have landed" for the P row only if both are the
            //  same kind of vector-memory instruction; the launcher keeps the P rows of a short launch inside a descriptor's 4 GB)
            int prow = 0;
            if (p.cond_hop > 0) prow = p_base(nn) + fast_div(t + p.cond_offset, p.hop_magic, p.hop_shift);
            const int po = (prow * p.proj_row_stride + j * 128 + h * 64) * 4;
#pragma unroll
            for (int it = 0; it < 4; ++it)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const f32x4 v = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(proj_rs, po + (it * 16 + q * 4) * 4, 0, 0));
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[it][q * 4 + e] = v[e];
                }
        } else {
            int prow = 0;
            if (p.cond_hop > 0) prow = p_base(nn) + fast_div(t + p.cond_offset, p.hop_magic, p.hop_shift);
            const float* pr = proj_n + (size_t)prow * p.proj_row_stride + j * 128 + h * 64;
#pragma unroll
            for (int it = 0; it < 4; ++it)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(pr + it * 16 + q * 4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[it][q * 4 + e] = v[e];
                }
        }
        if constexpr (SHORT) {
            // (An "early half" -- GEMM1's x[t] k-steps of pair 0 run while the look-back row is still in flight -- needs the compiler's scoreboard to know that
            //  the P row has landed when the look-back loads go out: a vmcnt(0) BUILTIN directly behind the P loads does that, inline asm or a wait further
            //  down does not, and then the first MFMA gets a vmcnt(0), look-back row included.  Priced, profiles/r06_ab_experiments.md r06_u ... r06_x: with
            //  that builtin the wait for the P row (0.7 us, this path's latency, not a miss: touching the rows from the loader wave two layers ahead changes
            //  nothing) stands in front of the dependency check and costs more than the 24 MFMAs it frees: 0.457 against 0.452 ms at 1 x 16000; the P row
            //  requested in FRONT of the drain delays the publication the neighbours wait for by 1 us: 0.462 ms.  So: P row and look-back row in one queue,
            //  one wait in front of the first MFMA.)
            PT_EV(15, j, u);
            if (lv_j != j) { layer_vectors(j); lv_j = j; }
            const unsigned bad = eval(dep_addr(j, u)) & ~1u;      // (its own rows are this wave's previous output: program order)
            war_ok = (bad & kWarMask) == 0;
            if (bad & kRawMask) {
                wait_deps(j, u, kRawMask & ~1u, j, 4);
                if (dead) break;
            }
            PT_EV(16, j, u);
            load_xb(j, u, rxb);
            PT_EV(18, j, u);
        }
        // the next task (claimed an iteration ago) and the bytes it depends on
        int j2 = j;
        const int u2 = next_task(j, u, j2);
        unsigned bad2 = 0;                     // its dependency bits (one LDS byte per lane, read here under the P loads)
        if (u2 >= 0) {
            if (j2 != lv_j) { layer_vectors(j2); lv_j = j2; }
            bad2 = eval(dep_addr(j2, u2));
            if (stat) bad2 &= ~1u;             // (its own rows are this very task's output: program order)
        }

        if (!SHORT && p.x_first && j == 0) {
            // rebuild this lane's 32 channels (8g + 4h + e) of h[t] and h[t-d] from the scalars; the operation order of
            // iaf_front_kernel / the FIRST variant of the per-layer kernel: round(x[t-1] w0), then fma(x[t], w1, .)
            const float x0 = rxc[0], x1v = rxc[1], xd0 = rxb[0], xd1 = rxb[1];
            const bool has_prev = t >= dil_of(0);
            if (p.range_flag && !(fabsf(x0) <= p.x_limit)) __hip_atomic_store(p.range_flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
#pragma unroll
            for (int g = 0; g < 8; ++g) {
                const f32x4 w0 = *reinterpret_cast<const f32x4*>(&lds[kCfF + 8 * g + 4 * h]);
                const f32x4 w1 = *reinterpret_cast<const f32x4*>(&lds[kCfF + 64 + 8 * g + 4 * h]);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    rxc[4 * g + e] = fmaf(x0, w1[e], x1v * w0[e]);
                    const float vb = fmaf(xd0, w1[e], xd1 * w0[e]);
                    rxb[4 * g + e] = has_prev ? vb : 0.f;
                }
            }
        }
        const float* bias = lds + kBiasF + (j & 1) * 64 + h * 32;
        float o[32];
        f32x16 acc2[2];
        // drain + publish + leave, behind the first operand work of the unit (the P row and the previous unit's stores land
        // meanwhile); then the verdict on the next task's dependencies
        auto settle_top = [&]() {
            PT_PHASE(9);
            if (!SHORT) PT_EV(5, j, u);
            PT_BEGIN();
            if (!SHORT) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // (SHORT: nothing is owed here -- the top of this unit has drained and published)
            PT_END(1);
            PT_EV(6, j, u);
            if constexpr (!SHORT) {      // (SHORT: the top of the unit has done all of it)
                publish();
                if (left_upto < j) leave_layers(j);
                if (u2 >= 0) claim_v = claim();
            }
            PT_ADD(5, 1);
            PT_MARK();
        };
        // the next task's rows: requested between GEMM1 and GEMM2, in flight under GEMM2 + gating + stores -- if their
        // producers are done (normally they are a layer-sweep old); otherwise behind this unit's stores, after a wait.
        // ("In flight" is a property of the COMPILED loop, not of this source: no s_waitcnt vmcnt may stand between the loads and GEMM2's
        //  first fragment reads on the wave-uniform path; see load_x and tests/test_persist_prefetch_isa.py.  -DPWV_PTRACE slot [13] times it.)
        // (stationary units) the word of a LEFT NEIGHBOUR's unit the next task waits for: asked for here, under GEMM2 -- a poll is a
        // 2 us round trip, and that unit, its workgroup's top one, is usually through by now; the answer goes into its byte before the wait
        int early_v = -1;
        auto prefetch_next = [&]() {
            PT_PHASE(10);
            PT_BEGIN();
            if (u2 >= 0 && !(bad2 & kRawMask) && !stat) {
                load_x(j2, u2, rxb, rxc);
            } else {      // (ends the old rows' live ranges: without it they would occupy 64 registers through both GEMMs)
#pragma unroll
                for (int k = 0; k < 32; ++k) rxb[k] = rxc[k] = 0.f;
            }
            if (stat && u2 >= 0 && (bad2 & 0x36u)) {
                // (lanes 1 / 2: the left neighbour's unit; lanes 32..: the RIGHT neighbours' workgroup words when the next task's stores will have
                //  to know that the readers of their ring slot are through -- the top unit's WAR side, a 2 - 3 us poll in front of its stores otherwise)
                const int a2 = dep_addr(j2, u2);
                const int cnt_r = w + p.reach_wgs < p.last_wg ? p.reach_wgs : p.last_wg - w;
                int lo = lane;
                asm volatile("" : "+v"(lo));
                if ((lo == 1 || lo == 2) && a2 >= kLeftB && a2 < kDoneB)
                    early_v = __hip_atomic_load(uprog_n + (size_t)(u_begin - kLeftN + a2 - kLeftB) * kUnitStride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                else if ((bad2 & 0x30u) && lo >= 32 && lo - 32 < cnt_r)
                    early_v = __hip_atomic_load(prog_n + (size_t)(w + 1 + lo - 32) * kProgStride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            __builtin_amdgcn_sched_barrier(0);
            PT_LAP(13);
        };
        // the last fragment of the dense matrix (not in LDS): global memory, 16 bytes per lane
        const float* lastfrag = packed_n + (size_t)j * p.packed_stride + kSlot + lane * 4;

        if constexpr (F32) {
            // ---- exact-fp32 arithmetic: v_mfma_f32_32x32x2_f32, the operands are the rows as loaded (pwv_layer.hip) ----
            float xc[32], xb[32];
#pragma unroll
            for (int k = 0; k < 32; ++k) { xc[k] = rxc[k]; xb[k] = rxb[k]; }
            if constexpr (SHORT && !STREAM) {      // (SHORT: the look-back row arrives unselected, see load_xb; rows left of the utterance start are zero, modules.py:24-28)
                if (!__all(t >= dil_of(j))) {
                    const bool hp = t >= dil_of(j);
#pragma unroll
                    for (int k = 0; k < 32; ++k) xb[k] = hp ? xb[k] : 0.f;
                }
            }
            settle_top();
            hist_store(j, dil_of(j), nn, t, u, rc, valid, xc);
            const float* Af = lds + (j & 1) * kSlot;                 // [kA1 | kA2 minus its last fragment]
            f32x4 a[4];
            f32x4 lf = {0.f, 0.f, 0.f, 0.f};
            auto bx = [&](int ks) -> float { return ks < 32 ? xb[ks] : xc[ks - 32]; };
            a[0] = frag(Af, 0, 0, 16, 0, lane);
            a[1] = frag(Af, 0, 2, 16, 0, lane);
            gemm_groups<16, 2, 0, 2>(Af, 0, lane, acc, a, bx, [](int) {}, [&](f32x4(&nf)[4]) {
                nf[0] = frag(Af, 0, 1, 16, 0, lane);
                nf[1] = frag(Af, 0, 3, 16, 0, lane);
            });
            gemm_groups<16, 2, 1, 2>(
                Af, 0, lane, acc, a, bx,
                [&](int g) {
                    o[g] = gate_act(acc[0][g], acc[2][g]);
                    asm volatile("" : "+v"(o[g]));   // keep the gating inside this MFMA group (no sinking)
                    if (g == 10) lf = *reinterpret_cast<const f32x4*>(lastfrag);
                },
                [&](f32x4(&nf)[4]) {
                    nf[0] = frag(Af, kA1Size, 0, 8, 0, lane);
                    nf[1] = frag(Af, kA1Size, 1, 8, 0, lane);
                });
#pragma unroll
            for (int it = 0; it < 2; ++it)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const f32x4 bd = *reinterpret_cast<const f32x4*>(bias + it * 16 + q * 4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc2[it][q * 4 + e] = xc[it * 16 + q * 4 + e] + bd[e];
                }
            asm volatile("" : "+v"(acc2[0]), "+v"(acc2[1]), "+v"(lf));
            prefetch_next();
            gemm_groups_dense(
                [&](int it, int g) -> f32x4 { return (it == 1 && g == 7) ? lf : frag(Af, kA1Size, it, 8, g, lane); }, acc2, a,
                [&](int ks) -> float { return o[ks]; },
                [&](int g) {
                    if (g < 4) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            o[16 + 4 * g + e] = gate_act(acc[1][4 * g + e], acc[3][4 * g + e]);
                            asm volatile("" : "+v"(o[16 + 4 * g + e]));
                        }
                    }
                });
            PT_LAP(14);
        } else {
            const f16x8* A1 = reinterpret_cast<const f16x8*>(lds + (j & 1) * kSlot);
            const f16x8* A2 = reinterpret_cast<const f16x8*>(lds + (j & 1) * kSlot + kA1Size);

            f16x8 bh[8], bl[8];      // B operands: bh[0..3] = x[t-d], bh[4..7] = x[t]; packed K order: x[t] first (pwv_layer_f16.hip)
            float xc[32];
#pragma unroll
            for (int k = 0; k < 32; ++k) xc[k] = rxc[k];
            split8<0>(xc, bh[4], bl[4]);
            split8<8>(xc, bh[5], bl[5]);
            split8<16>(xc, bh[6], bl[6]);
            split8<24>(xc, bh[7], bl[7]);
            settle_top();
            hist_store(j, dil_of(j), nn, t, u, rc, valid, xc);
            auto bxh = [&](int s) -> f16x8 { return bh[s ^ 4]; };
            auto bxl = [&](int s) -> f16x8 { return bl[s ^ 4]; };
            f16x8 oh[4], ol[4];
            f16x8 ah[4], al[4];
            f16x8 lf = {0, 0, 0, 0, 0, 0, 0, 0};

            {
            // ---- GEMM1, row-tile pair 0 = (F[0:32], G[0:32]); x[t-d] is split under its first four MFMA groups ----------
            first_frags<8, 2, 0, 2, 4>(A1, lane, ah, al);
            gemm16<8, 2, 0, 2, 4>(
                A1, lane, acc, ah, al, bxh, bxl,
                [&](int s) {
                    if constexpr (SHORT) {      // the look-back row (no select behind its loads, see load_xb) is zeroed left of the utterance start and split HERE, in one piece
                        if (s == 3) {
                            PT_EV(14, j, u);
                            if constexpr (!STREAM) {      // (STREAM: load_xb has put the history's rows there)
                                if (!__all(t >= dil_of(j))) {      // (rows left of the utterance start: zero, modules.py:24-28)
                                    const bool hp = t >= dil_of(j);
#pragma unroll
                                    for (int k = 0; k < 32; ++k) rxb[k] = hp ? rxb[k] : 0.f;
                                }
                            }
                            split8<0>(rxb, bh[0], bl[0]);
                            split8<8>(rxb, bh[1], bl[1]);
                            split8<16>(rxb, bh[2], bl[2]);
                            split8<24>(rxb, bh[3], bl[3]);
                            asm volatile("" : "+v"(bh[0]), "+v"(bl[0]), "+v"(bh[1]), "+v"(bl[1]), "+v"(bh[2]), "+v"(bl[2]), "+v"(bh[3]), "+v"(bl[3]));
                            PT_EV(5, j, u);
                        }
                    } else {
                        if (s == 0) { split8<0>(rxb, bh[0], bl[0]); asm volatile("" : "+v"(bh[0]), "+v"(bl[0])); }
                        if (s == 1) { split8<8>(rxb, bh[1], bl[1]); asm volatile("" : "+v"(bh[1]), "+v"(bl[1])); }
                        if (s == 2) { split8<16>(rxb, bh[2], bl[2]); asm volatile("" : "+v"(bh[2]), "+v"(bl[2])); }
                        if (s == 3) { split8<24>(rxb, bh[3], bl[3]); asm volatile("" : "+v"(bh[3]), "+v"(bl[3])); }
                    }
                },
                [&](f16x8(&nh)[4], f16x8(&nl)[4]) { first_frags<8, 2, 1, 2, 4>(A1, lane, nh, nl); });
            // ---- pair 1 = (F[32:64], G[32:64]); pair 0 is gated + split under these MFMAs -----------------------------------
            gemm16<8, 2, 1, 2, 4>(
                A1, lane, acc, ah, al, bxh, bxl,
                [&](int s) {
                    o[2 * s] = gate_act(acc[0][2 * s], acc[2][2 * s]);
                    o[2 * s + 1] = gate_act(acc[0][2 * s + 1], acc[2][2 * s + 1]);
                    asm volatile("" : "+v"(o[2 * s]), "+v"(o[2 * s + 1]));
                    if (s == 3) { split8<0>(o, oh[0], ol[0]); asm volatile("" : "+v"(oh[0]), "+v"(ol[0])); }
                    if (s == 7) { split8<8>(o, oh[1], ol[1]); asm volatile("" : "+v"(oh[1]), "+v"(ol[1])); }
                    if (s == 5) lf = *reinterpret_cast<const f16x8*>(lastfrag);      // lands under the last two k-steps
                },
                [&](f16x8(&nh)[4], f16x8(&nl)[4]) { first_frags<4, 2, 0, 1, 2>(A2, lane, nh, nl); });
            }

            // ---- GEMM2: dense 64 -> 64, accumulator starts at x[t] + dense_bias ---------------------------------------------
#pragma unroll
            for (int it = 0; it < 2; ++it)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const f32x4 bd = *reinterpret_cast<const f32x4*>(bias + it * 16 + q * 4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc2[it][q * 4 + e] = xc[it * 16 + q * 4 + e] + bd[e];
                }
            asm volatile("" : "+v"(acc2[0]), "+v"(acc2[1]), "+v"(lf));
            prefetch_next();      // (xc is dead from here on)
            gemm16_dense(
                [&](int comp, int it, int s) -> f16x8 { return (comp == 1 && it == 1 && s == 3) ? lf : frag16<4, 2>(A2, comp, it, s, lane); },
                acc2, ah, al, [&](int s) -> f16x8 { return oh[s]; }, [&](int s) -> f16x8 { return ol[s]; },
                [&](int s) {
                    if (s < 2) {   // k-steps 0,1 use o tile 0; gate + split tile 1 under them
#pragma unroll
                        for (int e = 0; e < 8; ++e) o[16 + 8 * s + e] = gate_act(acc[1][8 * s + e], acc[3][8 * s + e]);
                        if (s == 0) split8<16>(o, oh[2], ol[2]);
                        else split8<24>(o, oh[3], ol[3]);
                        asm volatile("" : "+v"(oh[2 + (s & 1)]), "+v"(ol[2 + (s & 1)]));
                    }
                });
            PT_LAP(14);
        }
        if (dead) break;
        PT_PHASE(11);
        PT_EV(1, j, u);
        // ---- stores (after the readers of the ring slot they overwrite are known to be done) -------------------------------
        if (!war_ok) {
            // (that verdict is a task old: look again before the machinery of a wait -- drain, leave, poll -- is set in motion; 1 us per unit on
            //  short inputs, where every unit's verdict is stale, profiles/r06_short_timeline.md)
            unsigned badw = kWarMask;
            if constexpr (SHORT) {
                if (lv_j != j) layer_vectors(j);
                badw = eval(dep_addr(j, u)) & kWarMask;
                if (lv_j != j) layer_vectors(lv_j);
            }
            if (badw) {
                PT_BEGIN();
                wait_deps(j, u, kWarMask, lv_j, 5);
                PT_END(3);
                if (dead) break;
            }
        }
        {
            const int so = out_soff(j);
            const int oo = toff(row);
            // units the right neighbour reads as x[t-d] in the next layer are stored write-through
            const int dn = dil_next(j);
            const bool shared = p.all_wt || u + ((dn + 31) >> 5) >= u_end;
            if (valid) {
                if (shared) {
#pragma unroll
                    for (int g = 0; g < 8; ++g) {
                        const int it = g >> 2, q = g & 3;
                        const f32x4 v = {acc2[it][q * 4], acc2[it][q * 4 + 1], acc2[it][q * 4 + 2], acc2[it][q * 4 + 3]};
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), ring_rs, oo + g * 1024, so, kAuxWriteThrough);
                    }
                } else {
#pragma unroll
                    for (int g = 0; g < 8; ++g) {
                        const int it = g >> 2, q = g & 3;
                        const f32x4 v = {acc2[it][q * 4], acc2[it][q * 4 + 1], acc2[it][q * 4 + 2], acc2[it][q * 4 + 3]};
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), ring_rs, oo + g * 1024, so, kStoreAuxLocal);
                    }
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        PT_EV(2, j, u);

        // ---- move on ------------------------------------------------------------------------------------------------------
        prev_addr = kDoneB + (u - u_begin);
        prev_j = j;
        if (stat && u2 >= 0 && (bad2 & 0x36u)) {      // the early poll's answer (lv_j == j2 here)
            const int a2 = dep_addr(j2, u2);
            if (early_v >= 0 && lane < 32) lb[a2] = (unsigned char)(early_v > 255 ? 255 : early_v);
            if ((bad2 & 0x30u) && w < p.last_wg && __ballot(lane >= 32 && early_v >= 0 && early_v < j2 - 1) == 0 && (int)lb[kSeenRB] < j2 - 1)
                lb[kSeenRB] = (unsigned char)(j2 - 1);
        }
        if constexpr (SHORT) {
            // (the next unit's top drains, publishes, waits and loads; its own rows are these accumulators)
#pragma unroll
            for (int k = 0; k < 32; ++k) rxc[k] = acc2[k >> 4][k & 15];
        } else if (u2 >= 0 && (bad2 & kRawMask)) {
            // the next task's producers were still at work when this unit looked: publish what this wave owes (a wave never
            // spins while holding unpublished work), wait, then load with the latency exposed
            PT_BEGIN();
            PT_ADD(6, 1);
            wait_deps(j2, u2, kRawMask, lv_j, 4);
            PT_END(2);
            if (dead) break;
            load_x(j2, u2, rxb, rxc);
        }
        j = j2;
        u = u2;
        if constexpr (!SHORT) war_ok = (bad2 & kWarMask) == 0;
        PT_PHASE(12);
    }
    // the last unit's stores, a refill this wave still owes, and the layers it has not yet counted itself out of
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (!dead && !(loader_mode && wave >= n)) {      // (with a loader the idle waves are not counted: it waits for the n active ones)
        publish();
        leave_layers(L);
        if (dma_pending >= 0) flush_owed();
    }
    // ---- TAIL: the net's LAST layer with the head behind it (modules.py:145-165), then the IAF affine (modules.py:59) -------------
    // What used to be two more launches per flow (layer_f16x3_kernel<..., HEAD> and the affine) runs here on the workgroup's own
    // units as soon as ITS eight waves have left the run's last layer -- no grid-wide drain, no launch ramp.  The operations are
    // those of the HEAD variant in the same order (bit-identical, tests/test_gpu_persist.py).  The head's three matrices take
    // the whole LDS (filter|gate 64 KB + skip 32 KB + postprocess1 64 KB), so the control state above is gone from here on:
    // units are handed out statically, the left neighbours' progress words are polled directly, and the exit accounting at
    // the bottom is done by one thread behind a barrier.
    bool tail_done = false;
    {
        if (p.tail_q > 0) {
            tail_done = true;
            PT_EV(8, L, -1);
            __syncthreads();                       // every wave of the workgroup is out of the task loop (its stores drained, its layers left)
            const int wg_dead = __builtin_amdgcn_readfirstlane(*(__attribute__((address_space(3))) volatile int*)&ctl[1]);
            __syncthreads();                       // ... and has read that word before the weights overwrite it
            bool tail_ok = !wg_dead;
            if (tail_ok) {
                constexpr int kHS = kA1Size, kH1 = kA1Size + kASSize;
                fill_lds_dma<kA1Size / 4, 8>(lds, p.tail_layer[net] + kA1, wave, lane);
                fill_lds_dma<kASSize / 4, 8>(lds + kHS, p.tail_head[net] + kHAS, wave, lane);
                fill_lds_dma<kHA1Size / 4, 8>(lds + kH1, p.tail_head[net] + kHA1, wave, lane);
                // the look-back of this wave's first unit (u_begin + wave) reaches into the left neighbours iff wave < reach: they must
                // have completed the run's last layer ("layers completed for all my units" == L), bounded like every other wait
                const int td = p.tail_dil;
                if (w > 0 && wave < ((td + 31) >> 5)) {
                    const int w0 = w - p.tail_reach_wgs > 0 ? w - p.tail_reach_wgs : 0;
                    const int cnt = w - w0;
                    const long long t0 = __builtin_amdgcn_s_memrealtime();
                    for (int k = 0;; ++k) {
                        int v = 1 << 20;
                        if (lane < cnt) v = __hip_atomic_load(prog_n + (size_t)(w0 + lane) * kProgStride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if (__ballot(v < L) == 0) break;
                        if ((k & 63) == 63 && (__builtin_amdgcn_readfirstlane(__hip_atomic_load(p.abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) ||
                                               __builtin_amdgcn_s_memrealtime() - t0 > kWaitTicks)) {
                            __hip_atomic_store(p.status, 6, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                            __hip_atomic_store(p.abort, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            tail_ok = false;
                            break;
                        }
                        __builtin_amdgcn_s_sleep(4);
                    }
                }
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();                   // the head's weights are resident
                PT_EV(9, L, -1);
                const f16x8* A1 = reinterpret_cast<const f16x8*>(lds);
                const f16x8* HS = reinterpret_cast<const f16x8*>(lds + kHS);
                const f16x8* H1 = reinterpret_cast<const f16x8*>(lds + kH1);
                (void)A1; (void)HS; (void)H1;
                const float* hb = p.tail_head[net];
                const int Q = p.tail_q;
                const int so = in_soff(L);         // the run's last layer wrote buffer (L - 1 + rot) % 3
                const __amdgpu_buffer_rsrc_t out_rs = [&]() {
                    const unsigned long long a = (unsigned long long)p.tail_out[net];
                    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a), hi2 = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
                    return __builtin_amdgcn_make_buffer_rsrc((void*)(((unsigned long long)hi2 << 32) | lo), 0,
                                                             __builtin_amdgcn_readfirstlane((unsigned)rows * (unsigned)Q * 4u), 0x00020000);
                }();
                auto load_tail = [&](int unit, float (&xb)[32], float (&xc)[32]) {
                    int row, rc, nn, t;
                    bool valid;
                    rows_of(unit, row, valid, rc, nn, t);
                    const bool has_prev = t >= td;
                    const int oc = toff(rc), ob = toff(has_prev ? rc - td : rc);
#pragma unroll
                    for (int g = 0; g < 8; ++g) {
                        const f32x4 v = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(ring_rs, oc + g * 1024, so, 16));
#pragma unroll
                        for (int e = 0; e < 4; ++e) xc[4 * g + e] = v[e];
                    }
#pragma unroll
                    for (int g = 0; g < 8; ++g) {
                        const f32x4 v = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(ring_rs, ob + g * 1024, so, 16));
#pragma unroll
                        for (int e = 0; e < 4; ++e) xb[4 * g + e] = has_prev ? v[e] : 0.f;
                    }
                    hist_lookback(L, td, nn, t, unit, rc, xb);
                };
                auto no_extra = [](int) {};
                int unit = u_begin + wave;
                float txb[32], txc[32];
                load_tail(unit, txb, txc);      // (unconditional, like every load of rows here: clamped addresses, and registers that are
                                                // written on every path do not stay live across the GEMMs)
                while (tail_ok && unit < u_end) {
                    // (compiler barrier: the head's small vectors -- skip / postprocess1 biases, postprocess2 -- are read from global
                    // memory per unit like P; hoisted out of the loop they are 192 loop-invariant registers, i.e. spills)
                    asm volatile("" ::: "memory");
                    const int next = unit + 8;
                    int row, rc, nn, t;
                    bool valid;
                    rows_of(unit, row, valid, rc, nn, t);
                    hist_store(L, td, nn, t, unit, rc, valid, txc);
                    f32x16 acc[4];
                    {
                        int prow = 0;
                        if (p.cond_hop > 0) prow = p_base(nn) + fast_div(t + p.cond_offset, p.hop_magic, p.hop_shift);
                        const float* pr = proj_n + (size_t)prow * p.proj_row_stride + L * 128 + h * 64;
#pragma unroll
                        for (int it = 0; it < 4; ++it)
#pragma unroll
                            for (int q = 0; q < 4; ++q) {
                                const f32x4 v = *reinterpret_cast<const f32x4*>(pr + it * 16 + q * 4);
#pragma unroll
                                for (int e = 0; e < 4; ++e) acc[it][q * 4 + e] = v[e];
                            }
                    }
                    f32x16 acc1[4];      // postprocess1's accumulators: what both arithmetics hand to the postprocess2 dot below
                    if constexpr (F32) {
                        // ---- exact fp32 (round 6): the operations of layer_f32_kernel<..., GATED, HEAD> in the same order ----------
                        auto bx = [&](int ks) -> float { return ks < 32 ? txb[ks] : txc[ks - 32]; };
                        float o[32];
                        f32x4 a[4];
                        a[0] = frag(lds, 0, 0, 16, 0, lane);
                        a[1] = frag(lds, 0, 2, 16, 0, lane);
                        gemm_groups<16, 2, 0, 2>(lds, 0, lane, acc, a, bx, no_extra, [&](f32x4(&nf)[4]) {
                            nf[0] = frag(lds, 0, 1, 16, 0, lane);
                            nf[1] = frag(lds, 0, 3, 16, 0, lane);
                        });
                        gemm_groups<16, 2, 1, 2>(
                            lds, 0, lane, acc, a, bx,
                            [&](int g) {
                                o[g] = gate_act(acc[0][g], acc[2][g]);
                                asm volatile("" : "+v"(o[g]));
                            },
                            [&](f32x4(&nf)[4]) {
#pragma unroll
                                for (int i = 0; i < 4; ++i) nf[i] = frag(lds, kHS, i, 8, 0, lane);
                            });
                        asm volatile("" ::: "memory");      // (the bias loads below stay behind GEMM1: hoisted to the top of the unit they are 64 + 64 registers too many)
                        f32x16 accs[4];
#pragma unroll
                        for (int it = 0; it < 4; ++it)
#pragma unroll
                            for (int q = 0; q < 4; ++q) {
                                const f32x4 v = *reinterpret_cast<const f32x4*>(hb + kHBS + h * 64 + it * 16 + q * 4);
#pragma unroll
                                for (int e = 0; e < 4; ++e) accs[it][q * 4 + e] = v[e];
                            }
#pragma unroll
                        for (int r = 0; r < 16; ++r) o[16 + r] = gate_act(acc[1][r], acc[3][r]);
                        gemm_groups<8, 4, 0, 1>(lds, kHS, lane, accs, a, [&](int ks) -> float { return o[ks]; }, no_extra, [&](f32x4(&nf)[4]) {
#pragma unroll
                            for (int i = 0; i < 4; ++i) nf[i] = frag(lds, kH1, i, 16, 0, lane);
                        });
                        asm volatile("" ::: "memory");
#pragma unroll
                        for (int it = 0; it < 4; ++it)
#pragma unroll
                            for (int q = 0; q < 4; ++q) {
                                const f32x4 v = *reinterpret_cast<const f32x4*>(hb + kHB1 + h * 64 + it * 16 + q * 4);
#pragma unroll
                                for (int e = 0; e < 4; ++e) acc1[it][q * 4 + e] = v[e];
                            }
                        gemm_groups<16, 4, 0, 1>(lds, kH1, lane, acc1, a, [&](int ks) -> float { return fmaxf(accs[ks >> 4][ks & 15], 0.f); }, no_extra,
                                                 [](f32x4(&)[4]) {});
                    } else {
                        f16x8 bh[8], bl[8];
                        float xc[32];
#pragma unroll
                        for (int i = 0; i < 32; ++i) xc[i] = txc[i];
                        split8<0>(xc, bh[4], bl[4]);
                        split8<8>(xc, bh[5], bl[5]);
                        split8<16>(xc, bh[6], bl[6]);
                        split8<24>(xc, bh[7], bl[7]);
                        auto bxh = [&](int s) -> f16x8 { return bh[s ^ 4]; };
                        auto bxl = [&](int s) -> f16x8 { return bl[s ^ 4]; };
                        float o[32];
                        f16x8 oh[4], ol[4];
                        f16x8 ah[4], al[4];
                        first_frags<8, 2, 0, 2, 4>(A1, lane, ah, al);
                        gemm16<8, 2, 0, 2, 4>(
                            A1, lane, acc, ah, al, bxh, bxl,
                            [&](int s) {
                                if (s == 0) { split8<0>(txb, bh[0], bl[0]); asm volatile("" : "+v"(bh[0]), "+v"(bl[0])); }
                                if (s == 1) { split8<8>(txb, bh[1], bl[1]); asm volatile("" : "+v"(bh[1]), "+v"(bl[1])); }
                                if (s == 2) { split8<16>(txb, bh[2], bl[2]); asm volatile("" : "+v"(bh[2]), "+v"(bl[2])); }
                                if (s == 3) { split8<24>(txb, bh[3], bl[3]); asm volatile("" : "+v"(bh[3]), "+v"(bl[3])); }
                            },
                            [&](f16x8(&nh)[4], f16x8(&nl)[4]) { first_frags<8, 2, 1, 2, 4>(A1, lane, nh, nl); });
                        gemm16<8, 2, 1, 2, 4>(
                            A1, lane, acc, ah, al, bxh, bxl,
                            [&](int s) {
                                o[2 * s] = gate_act(acc[0][2 * s], acc[2][2 * s]);
                                o[2 * s + 1] = gate_act(acc[0][2 * s + 1], acc[2][2 * s + 1]);
                                asm volatile("" : "+v"(o[2 * s]), "+v"(o[2 * s + 1]));
                                if (s == 3) { split8<0>(o, oh[0], ol[0]); asm volatile("" : "+v"(oh[0]), "+v"(ol[0])); }
                                if (s == 7) { split8<8>(o, oh[1], ol[1]); asm volatile("" : "+v"(oh[1]), "+v"(ol[1])); }
                            },
                            [](f16x8(&)[4], f16x8(&)[4]) {});
                        // ---- head: o (registers) -> skip -> relu -> postprocess1 -> relu -> postprocess2 ---------------------------
                        f32x16 accs[4];
#pragma unroll
                        for (int it = 0; it < 4; ++it)
#pragma unroll
                            for (int q = 0; q < 4; ++q) {
                                const f32x4 v = *reinterpret_cast<const f32x4*>(hb + kHBS + h * 64 + it * 16 + q * 4);
#pragma unroll
                                for (int e = 0; e < 4; ++e) accs[it][q * 4 + e] = v[e];
                            }
#pragma unroll
                        for (int r = 0; r < 16; ++r) o[16 + r] = gate_act(acc[1][r], acc[3][r]);
                        split8<16>(o, oh[2], ol[2]);
                        split8<24>(o, oh[3], ol[3]);
                        first_frags<4, 4, 0, 1, 4>(HS, lane, ah, al);
                        gemm16<4, 4, 0, 1, 4>(HS, lane, accs, ah, al, [&](int s) -> f16x8 { return oh[s]; }, [&](int s) -> f16x8 { return ol[s]; }, no_extra,
                                              [&](f16x8(&nh)[4], f16x8(&nl)[4]) { first_frags<8, 4, 0, 1, 4>(H1, lane, nh, nl); });
#pragma unroll
                        for (int it = 0; it < 4; ++it)
#pragma unroll
                            for (int q = 0; q < 4; ++q) {
                                const f32x4 v = *reinterpret_cast<const f32x4*>(hb + kHB1 + h * 64 + it * 16 + q * 4);
#pragma unroll
                                for (int e = 0; e < 4; ++e) acc1[it][q * 4 + e] = v[e];
                            }
                        f16x8 sh[8], sl[8];
                        {
                            float r[64];
#pragma unroll
                            for (int i = 0; i < 64; ++i) r[i] = fmaxf(accs[i >> 4][i & 15], 0.f);
                            split8<0>(r, sh[0], sl[0]);
                            split8<8>(r, sh[1], sl[1]);
                            split8<16>(r, sh[2], sl[2]);
                            split8<24>(r, sh[3], sl[3]);
                            split8<32>(r, sh[4], sl[4]);
                            split8<40>(r, sh[5], sl[5]);
                            split8<48>(r, sh[6], sl[6]);
                            split8<56>(r, sh[7], sl[7]);
                        }
                        gemm16<8, 4, 0, 1, 4>(H1, lane, acc1, ah, al, [&](int s) -> f16x8 { return sh[s]; }, [&](int s) -> f16x8 { return sl[s]; }, no_extra,
                                              [](f16x8(&)[4], f16x8(&)[4]) {});
                    }
                    load_tail(next, txb, txc);      // the next unit's rows: in flight under the postprocess2 dot
                    float outv[kMaxQ] = {0.f, 0.f, 0.f, 0.f};
                    // (the addresses of the postprocess2 dot are made here, behind the GEMMs, from opaque copies: hoisted out of the unit loop as
                    // loop-invariant per-lane pointers they are the registers the exact-fp32 instantiation has to spill)
                    int out_idx = row * Q, hq = h * Q;
                    asm volatile("" : "+v"(out_idx), "+v"(hq));
                    for (int q = 0; q < Q; ++q) {
                        float part = 0.f;
                        const float* w2 = hb + kHW2 + (hq + q) * 64;
#pragma unroll
                        for (int i4 = 0; i4 < 16; ++i4) {
                            const f32x4 wv = *reinterpret_cast<const f32x4*>(w2 + 4 * i4);
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                const int i = 4 * i4 + e;
                                part = fmaf(fmaxf(acc1[i >> 4][i & 15], 0.f), wv[e], part);
                            }
                        }
                        part += __shfl_xor(part, 32);
                        part += hb[kHW2 + 2 * Q * 64 + q];
                        if (q < kMaxQ) outv[q] = part;
                        // (write-through: with `pair` the other net's workgroup of this range may be the one that reads it)
                        if (valid && h == 0) __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, part), out_rs, (out_idx + q) * 4, 0, kAuxWriteThrough);
                    }
                    if (p.affine_x && p.G == 1 && Q == 2) {      // one net with two outputs (scale, shift): the affine right here
                        if (valid && h == 0) p.affine_out[row] = fmaf(p.affine_x[row], outv[0], outv[1]);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    PT_EV(10, L, unit);
                    unit = next;
                }
            }
            // ---- the IAF affine for this range, by whichever of the two nets' workgroups arrives second ---------------------------
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wave's outputs are written through
            __syncthreads();
            if (p.affine_x && p.pair && p.G == 2) {
                if (tid == 0) {
                    const int old = __hip_atomic_fetch_add(p.pair + w, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    *(__attribute__((address_space(3))) volatile int*)&ctl[0] = old;
                }
                __syncthreads();
                const int old = __builtin_amdgcn_readfirstlane(*(__attribute__((address_space(3))) volatile int*)&ctl[0]);
                if (old == 1) {
                    const int r_end = u_end * 32 < rows ? u_end * 32 : rows;
                    for (int row = u_begin * 32 + tid; row < r_end; row += 512) {
                        const float sv = __hip_atomic_load(p.tail_out[0] + row, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        const float bv = __hip_atomic_load(p.tail_out[1] + row, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        p.affine_out[row] = fmaf(p.affine_x[row], sv, bv);
                    }
                    if (tid == 0) __hip_atomic_store(p.pair + w, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
            // exit accounting (below) without the LDS counter: one thread, behind the barrier
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            PT_EV(11, L, -1);
            if (wave == 0) {
                int done = 0;
                if (lane == 0) done = __hip_atomic_fetch_add(p.exited, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (__builtin_amdgcn_readfirstlane(done) == p.active_wgs - 1) {
                    for (int k = lane; k < p.G * p.nwg; k += 64) __hip_atomic_store(p.prog + (size_t)k * kProgStride, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (SHORT) for (int k = lane; k < p.G * p.units; k += 64) __hip_atomic_store(p.uprog + (size_t)k * kUnitStride, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (lane == 0) {
                        __hip_atomic_store(p.abort, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        __hip_atomic_store(p.exited, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                }
            }
        }
    }
    // The launch cleans up after itself: the LAST workgroup to finish zeroes every word a later launch polls (progress, abort,
    // this counter), so a launch that is handed this workspace again needs no zeroing kernel in front of it.  A wave counts
    // itself out only when its own global stores are complete (vmcnt(0)): no progress word can land after the zeroing.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (!tail_done) {
        int old = 0;
        if (lane == 0) old = __hip_atomic_fetch_add(&ctl[4], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (__builtin_amdgcn_readfirstlane(old) == 7) {
            int done = 0;
            if (lane == 0) done = __hip_atomic_fetch_add(p.exited, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (__builtin_amdgcn_readfirstlane(done) == p.active_wgs - 1) {
                for (int k = lane; k < p.G * p.nwg; k += 64) __hip_atomic_store(p.prog + (size_t)k * kProgStride, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (SHORT) for (int k = lane; k < p.G * p.units; k += 64) __hip_atomic_store(p.uprog + (size_t)k * kUnitStride, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (lane == 0) {
                    __hip_atomic_store(p.abort, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(p.exited, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
    }
#ifdef PWV_PTRACE
    if (p.trace && lane == 0) {
        pt_acc[8] = __builtin_amdgcn_s_memtime();
        pt_acc[0] = pt_acc[8] - pt_start;
        long long* tr = p.trace + ((size_t)blockIdx.x * 8 + wave) * 24;
        for (int k = 0; k < 15; ++k) tr[k] = pt_acc[k];
        tr[16] = net; tr[17] = w; tr[18] = dead ? 1 : 0; tr[19] = __builtin_amdgcn_s_memrealtime(); tr[20] = pt_start_rt;
    }
#endif
