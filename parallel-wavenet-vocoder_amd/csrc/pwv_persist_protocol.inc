// Persistent kernel, part 2: the dependency protocol.  One LDS byte per dependency and lane (dep_addr / eval), the neighbours' progress
// words (poll_side, poll_units), what a wave owes the others (publish, flush_owed, leave_layers), the bounded wait (wait_deps), task
// claiming.
// Expects: part 1.
// Defines: vpack, layer_vectors, dep_addr, eval, poll_side, poll_units, prev_addr, prev_j, dma_pending, left_upto, dead, publish,
//          flush_owed, leave_layers, wait_deps, claim, locate, next_task, j, u, claim_v, rxb, rxc, war_ok, PT_DECL's state.

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
