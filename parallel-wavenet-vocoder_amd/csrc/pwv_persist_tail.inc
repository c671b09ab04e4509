// Persistent kernel, part 6: the tail -- the net's last layer with the fused head behind it (pwv_head_f32.inc / pwv_head_f16x3.inc, the texts
// the per-layer HEAD kernels are made of), then the IAF affine and, with a tail, the exit accounting.
// Expects: parts 1, 2; every wave out of the task loop.  Defines tail_done.
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
#define PWV_HEAD_FENCE() asm volatile("" ::: "memory")      // (the bias loads stay behind the GEMM in front of them: hoisted to the top of the unit they are 64 + 64 registers too many)
#include "pwv_head_f32.inc"
#undef PWV_HEAD_FENCE
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
#include "pwv_head_f16x3.inc"
                    }
                    load_tail(next, txb, txc);      // the next unit's rows: in flight under the postprocess2 dot
                    float outv[kMaxQ] = {0.f, 0.f, 0.f, 0.f};
                    // (the addresses of the postprocess2 dot are made here, behind the GEMMs, from opaque copies: hoisted out of the unit loop as
                    // loop-invariant per-lane pointers they are the registers the exact-fp32 instantiation has to spill)
                    int out_idx = row * Q, hq = h * Q;
                    asm volatile("" : "+v"(out_idx), "+v"(hq));
#define PWV_HEAD_STORE(q, part) do { if ((q) < kMaxQ) outv[q] = (part); \
        /* (write-through: with `pair` the other net's workgroup of this range may be the one that reads it) */ \
        if (valid && h == 0) __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, (part)), out_rs, (out_idx + (q)) * 4, 0, kAuxWriteThrough); } while (0)
#include "pwv_head_pp2.inc"
#undef PWV_HEAD_STORE
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
