// Persistent kernel, part 5: the task loop -- the first task, then per unit: top (P row, dependencies), the unit's arithmetic
// (pwv_persist_unit_f32.inc / pwv_persist_unit_f16x3.inc), the stores, moving on; behind the loop what the wave still owes.
// Expects: parts 1, 2 (and j / u where the folded loop left them).  Defines lv_j.
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
        PT_BEGIN();      // (slots [15] .. [17]: the three spans of the top, stack_persist.hip)
        // ---- TOP: P row requested; the rows of this unit were requested during the previous one ---------------------------
        int row, rc, nn, t;
        bool valid;
        rows_of_top(u, row, valid, rc, nn, t);
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
            // No scalar memory load here: the row stride and the hop constants come out of lanes of v_dil (pwv_persist_geometry.inc).  Buffer
            // loads, the kind the rows are loaded with: one kind of vector-memory instruction in the queue is what lets the compiler count "all
            // but the last 16 have landed" for the rows it splits below instead of draining the queue in front of them.  The descriptor starts at
            // the unit's first P row -- lane 0's: the rows of a unit ascend with the lane and so do their P rows, an utterance's frames lying
            // inside its own block of P -- and the lanes' offsets are relative to it.
            int prow = 0;
            if (p.cond_hop > 0) prow = p_base(nn) + fast_div(t + top_scalar(kLaneCondOffset), (unsigned)top_scalar(kLaneHopMagic), (unsigned)top_scalar(kLaneHopShift));
            const int stride = top_scalar(kLaneStride);
            const int prow0 = __builtin_amdgcn_readfirstlane(prow);
            const __amdgpu_buffer_rsrc_t prs = proj_rs_at((long long)prow0 * stride);
            const int po = ((prow - prow0) * stride + h * 64) * 4;
#pragma unroll
            for (int it = 0; it < 4; ++it)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const f32x4 v = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(prs, po + (it * 16 + q * 4) * 4, j * 512, 0));
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[it][q * 4 + e] = v[e];
                }
            PT_LAP(15);
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
            // (the four scalars are read by every fmaf above, so the rebuilt elements 0 and 1 are born in other registers than the ones the rows are loaded
            //  into.  The copy home is spelled out HERE, as an instruction of this arm: left to the register allocator, the rebuilt value keeps its register
            //  and the join stands on the OTHER arm -- a v_mov_b32 behind an `s_waitcnt vmcnt(0)` of the compiler's own, in front of the split of every unit
            //  of every other layer; tests/test_persist_top_isa.py)
            const float n0 = rxc[0], n1 = rxc[1], m0 = rxb[0], m1 = rxb[1];
            __builtin_amdgcn_sched_barrier(0);      // (behind the last reader of the scalars)
            asm volatile("v_mov_b32 %0, %4\n\tv_mov_b32 %1, %5\n\tv_mov_b32 %2, %6\n\tv_mov_b32 %3, %7"
                         : "=&v"(rxc[0]), "=&v"(rxc[1]), "=&v"(rxb[0]), "=&v"(rxb[1]) : "v"(n0), "v"(n1), "v"(m0), "v"(m1));
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
            // (... and once more as the builtin, which the compiler's own scoreboard understands: the asm orders memory, this tells it that the P row has
            //  landed.  Without it the compiler puts its own waits for the P row's registers into GEMM1 -- behind leave_layers' refill, so that the one wave
            //  that issues a refill would sit out the whole 79 KB in front of its second MFMA; simm16 = vmcnt 0, expcnt 7, lgkmcnt 15)
            if (!SHORT) __builtin_amdgcn_s_waitcnt(0x0F70);
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
#include "pwv_persist_unit_f32.inc"
        } else {
#include "pwv_persist_unit_f16x3.inc"
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
