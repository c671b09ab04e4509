// The body of layer_f32_kernel and of its streaming form layer_f32_stream_kernel (pwv_layer.hip), included into both: the kernel's parameter block
// `p`, `constexpr bool STREAM` and `const StreamParams st` are in scope.  Text, not a function: the non-streaming kernels keep the very
// instruction streams they had before the streaming form existed (tools/isa_compare.py).
// The fused head of the HEAD variants is text of its own, pwv_head_f32.inc and pwv_head_pp2.inc, which the persistent kernel's tail (pwv_persist_tail.inc)
// includes too: the two are bit-identical because they are one text.
    static_assert(!FOLD || FIRST, "FOLD: layer 0 of a scalar-input net only");
    static_assert(!STREAM || (SKIP ? !COND && !FIRST && !HEAD : FOLD == FIRST && (COND ? !HEAD && !(FIRST && GATED) : GATED == HEAD)),
                  "STREAM: folded layer 0, plain residual layer, last layer + head; COND: the last layer gated, its head a launch of its own; "
                  "SKIP: a residual or gated layer on row histories (layer 0 behind a streaming front), the head a launch of its own");
    static_assert(!HEAD || (GATED && !SKIP && !COND && !FIRST), "HEAD: plain last layer only");
    static_assert(!FIRST || !SKIP, "FIRST: no skip accumulation");
    constexpr int WAVES = 8;
    constexpr int kLds = HEAD ? kA1Size + kASSize + kHA1Size : layer_floats(SKIP, COND);
    constexpr int kCF = kLds + 4;           // FIRST: the causal filter [2][64] behind the unit counter
    constexpr int kHS = kA1Size;            // HEAD: skip weights, then postprocess1
    constexpr int kH1 = kA1Size + kASSize;
    __shared__ __attribute__((aligned(16))) float lds[kLds + (HEAD ? 0 : 4) + (FIRST ? 128 : 0)];   // +4: the unit counter

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = lane >> 5;
    const int net = blockIdx.x % p.G;
    const int wg = blockIdx.x / p.G;
    const int nwg = gridDim.x / p.G;
    int* unit_counter = reinterpret_cast<int*>(&lds[HEAD ? 0 : kLds]);      // unused with HEAD

    if constexpr (HEAD) {
        fill_lds_dma<kA1Size / 4, WAVES>(lds, p.packed[net] + kA1, wave, lane);
        fill_lds_dma<kASSize / 4, WAVES>(lds + kHS, p.packed_head[net] + kHAS, wave, lane);
        fill_lds_dma<kHA1Size / 4, WAVES>(lds + kH1, p.packed_head[net] + kHA1, wave, lane);
    } else {
        fill_lds_dma<kLds / 4, WAVES>(lds, p.packed[net], wave, lane);
        if (tid == 0) *unit_counter = 0;
        if constexpr (FIRST) {
            if (tid < 128) lds[kCF + tid] = p.cfilt[net][tid];
        }
    }
    __syncthreads();

    constexpr int kAS = kLayerBase;
    constexpr int kBS = kAS + kASSize;
    constexpr int kAC = kLayerBase + (SKIP ? kASSize + kBSSize : 0);
    constexpr int NC8 = kCondC / 8;

    const int rows = p.N * p.T;
    const int units = (rows + 31) / 32;
    const bool skip_load = SKIP && !p.skip_init;

    // this workgroup's contiguous share of the units
    const int per_wg = (units + nwg - 1) / nwg;
    const int u_begin = wg * per_wg;
    const int u_end = (u_begin + per_wg < units) ? u_begin + per_wg : units;

    auto grab = [&]() -> int {   // next unit for this wave
        int v = 0;
        if (lane == 0) v = __hip_atomic_fetch_add(unit_counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        return u_begin + __builtin_amdgcn_readfirstlane(v);
    };

    TileRegs<SKIP, COND> cur;
    if (wave >= WAVES / 2) __builtin_amdgcn_s_setprio(1);
    int unit = HEAD ? u_begin + wave : grab();

    auto no_extra = [](int) {};
    const __amdgpu_buffer_rsrc_t out_rs = units_rsrc(p.x_out[net], u_begin, u_end, 32 * 64 * 4);      // unused with HEAD

    while (unit < u_end) {
        int wr = 0;
        (void)wr;
        load_tile<SKIP, COND, FIRST, STREAM>(p, st, net, unit, lane, cur, wr);
        if constexpr (STREAM) {
            // what the next chunk looks back at: the last d + 1 scalars of layer 0's input / the last d rows of this layer's
            const int k = cur.t + p.dilation + (FIRST ? 1 : 0) - p.T;
            if (cur.valid && k >= 0) {
                float* hw = st.hist_wr + (long long)wr * st.block_stride;
                if constexpr (FIRST) {
                    if (h == 0) hw[st.scalar_off + k] = cur.xc[0];
                } else {
                    hw += st.row_off[net] + tile_off(k, h, 64);
#pragma unroll
                    for (int g = 0; g < 8; ++g) {
                        const f32x4 v = {cur.xc[4 * g], cur.xc[4 * g + 1], cur.xc[4 * g + 2], cur.xc[4 * g + 3]};
                        *reinterpret_cast<f32x4*>(hw + g * 256) = v;
                    }
                }
            }
        }
        float first_x0 = 0.f, first_x1 = 0.f;      // FIRST: x[t], x[t-1]
        float fold_b0 = 0.f, fold_b1 = 0.f;        // FOLD: the B values of the two k-steps
        (void)first_x0;
        (void)first_x1;
        (void)fold_b0;
        (void)fold_b1;
        if constexpr (FIRST) {
            // this lane's 32 channels (8g + 4h + e) of h[t] and h[t-d] from the scalars; same operation order as
            // iaf_front_kernel: round(x[t-1] w0), then fma(x[t], w1, .)
            const float x0 = cur.xc[0], x1v = cur.xc[1], xd0 = cur.xb[0], xd1 = cur.xb[1];
            first_x0 = x0;
            first_x1 = x1v;
            const bool has_prev = cur.t >= p.dilation;
            if constexpr (FOLD) {      // (x[t-d], x[t-d-1] are already zero left of the start)
                fold_b0 = h ? xd0 : xd1;      // k = 0, 1
                fold_b1 = h ? x0 : x1v;       // k = 2, 3
            }
#pragma unroll
            for (int g = 0; g < (FOLD ? 0 : 8); ++g) {
                const f32x4 w0 = *reinterpret_cast<const f32x4*>(&lds[kCF + 8 * g + 4 * h]);
                const f32x4 w1 = *reinterpret_cast<const f32x4*>(&lds[kCF + 64 + 8 * g + 4 * h]);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    cur.xc[4 * g + e] = fmaf(x0, w1[e], x1v * w0[e]);
                    const float vb = fmaf(xd0, w1[e], xd1 * w0[e]);
                    cur.xb[4 * g + e] = has_prev ? vb : 0.f;
                }
                __builtin_amdgcn_sched_barrier(0);      // one filter quad at a time: the scheduler otherwise front-loads all 16 reads
            }
        }
        // ---- GEMM1: [F;G][128 x 32t] = W1^T[128 x K] * [x[t-d]; x[t]; (cond[t])] -------------
        // accumulators start at P[frame(t)] (conditioning projection + filter/gate bias)
        f32x16 acc[4];
#pragma unroll
        for (int it = 0; it < 4; ++it)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[it][r] = cur.pj[it * 16 + r];
        float o[32];
        f32x4 a[4];
        auto bx = [&](int ks) -> float { return ks < 32 ? cur.xb[ks] : cur.xc[ks - 32]; };
        auto bc = [&](int ks) -> float { return cur.cd[COND ? ks : 0]; };
        // pair 0 = row tiles (0: F[0:32], 2: G[0:32]); pair 1 = (1: F[32:64], 3: G[32:64]).
        // pair 0 is gated on the VALU while pair 1's MFMAs run.
        if constexpr (FOLD) {
            // ---- layer 0, folded: the per-sample condition's GEMM (if any), then two k-steps on the scalars ------------------
            if constexpr (COND) {
                a[0] = frag(lds, kAC, 0, NC8, 0, lane);
                a[1] = frag(lds, kAC, 2, NC8, 0, lane);
                gemm_groups<NC8, 2, 0, 2>(lds, kAC, lane, acc, a, bc, no_extra, [&](f32x4(&n)[4]) {
                    n[0] = frag(lds, kAC, 1, NC8, 0, lane);
                    n[1] = frag(lds, kAC, 3, NC8, 0, lane);
                });
                gemm_groups<NC8, 2, 1, 2>(lds, kAC, lane, acc, a, bc, no_extra, [](f32x4(&)[4]) {});
            }
            const f32x4* F0 = reinterpret_cast<const f32x4*>(p.fold0[net]);
            f32x4 ff[4];
#pragma unroll
            for (int it = 0; it < 4; ++it) ff[it] = F0[it * 64 + lane];
#pragma unroll
            for (int it = 0; it < 4; ++it) acc[it] = __builtin_amdgcn_mfma_f32_32x32x2f32(ff[it][0], fold_b0, acc[it], 0, 0, 0);
#pragma unroll
            for (int it = 0; it < 4; ++it) acc[it] = __builtin_amdgcn_mfma_f32_32x32x2f32(ff[it][1], fold_b1, acc[it], 0, 0, 0);
            if constexpr (!GATED) {
                a[0] = frag(lds, kA2, 0, 8, 0, lane);
                a[1] = frag(lds, kA2, 1, 8, 0, lane);
            }
#pragma unroll
            for (int g = 0; g < 16; ++g) o[g] = gate_act(acc[0][g], acc[2][g]);
        } else {
        if constexpr (COND) {
            a[0] = frag(lds, kAC, 0, NC8, 0, lane);
            a[1] = frag(lds, kAC, 2, NC8, 0, lane);
            gemm_groups<NC8, 2, 0, 2>(lds, kAC, lane, acc, a, bc, no_extra, [&](f32x4(&n)[4]) {
                n[0] = frag(lds, kA1, 0, 16, 0, lane);
                n[1] = frag(lds, kA1, 2, 16, 0, lane);
            });
        } else {
            a[0] = frag(lds, kA1, 0, 16, 0, lane);
            a[1] = frag(lds, kA1, 2, 16, 0, lane);
        }
        gemm_groups<16, 2, 0, 2>(lds, kA1, lane, acc, a, bx, no_extra, [&](f32x4(&n)[4]) {
            if constexpr (COND) {
                n[0] = frag(lds, kAC, 1, NC8, 0, lane);
                n[1] = frag(lds, kAC, 3, NC8, 0, lane);
            } else {
                n[0] = frag(lds, kA1, 1, 16, 0, lane);
                n[1] = frag(lds, kA1, 3, 16, 0, lane);
            }
        });
        if constexpr (COND) {
            gemm_groups<NC8, 2, 1, 2>(lds, kAC, lane, acc, a, bc, no_extra, [&](f32x4(&n)[4]) {
                n[0] = frag(lds, kA1, 1, 16, 0, lane);
                n[1] = frag(lds, kA1, 3, 16, 0, lane);
            });
        }
        gemm_groups<16, 2, 1, 2>(
            lds, kA1, lane, acc, a, bx,
            [&](int g) {
                o[g] = gate_act(acc[0][g], acc[2][g]);
                asm volatile("" : "+v"(o[g]));   // keep the gating inside this MFMA group (no sinking)
            },
            [&](f32x4(&n)[4]) {
                if constexpr (!GATED) {
                    n[0] = frag(lds, kA2, 0, 8, 0, lane);
                    n[1] = frag(lds, kA2, 1, 8, 0, lane);
                } else if constexpr (SKIP) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) n[i] = frag(lds, kAS, i, 8, 0, lane);
                } else if constexpr (HEAD) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) n[i] = frag(lds, kHS, i, 8, 0, lane);
                }
            });
        }

        const int ooff = units_off(cur.row, h, 64, u_begin);      // (rows past the end are never stored: `valid`)
        if constexpr (GATED && HEAD) {
            // ---- fused head: o (registers) -> skip -> relu -> postprocess1 -> relu -> postprocess2, the operations
            //      (and bits) of head_f32_kernel<true> ------------------------------------------------------------
            const float* hb = p.packed_head[net];
            f32x16 acc1[4];
#define PWV_HEAD_FENCE() do {} while (0)
#include "pwv_head_f32.inc"
#undef PWV_HEAD_FENCE
            const int Q = p.head_q;
            const int hq = h * Q;
#define PWV_HEAD_STORE(q, part) if (cur.valid && h == 0) p.head_out[net][(size_t)cur.row * Q + (q)] = (part)
#include "pwv_head_pp2.inc"
#undef PWV_HEAD_STORE
        } else if constexpr (GATED) {
            if constexpr (SKIP) load_skip_row<SKIP, COND>(p, net, lane, cur, skip_load);      // in flight under the gating
#pragma unroll
            for (int r = 0; r < 16; ++r) o[16 + r] = gate_act(acc[1][r], acc[3][r]);
            if (cur.valid) {
#pragma unroll
                for (int g = 0; g < 8; ++g) {
                    f32x4 v = {o[4 * g], o[4 * g + 1], o[4 * g + 2], o[4 * g + 3]};
                    store_wt(out_rs, ooff + g * 1024, v);
                }
            }
        } else {
            // ---- GEMM2: dense 64 -> 64, accumulator starts at x[t] + dense_bias ---------------
            f32x16 acc2[2];
#pragma unroll
            for (int it = 0; it < 2; ++it) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const f32x4 bd = *reinterpret_cast<const f32x4*>(&lds[kBD + h * 32 + it * 16 + q * 4]);
                    if constexpr (FIRST) {
                        // x[t] row evaluated again from the two scalars (same operations, same bits) rather than kept live
                        const int g = it * 4 + q;
                        const f32x4 w0 = *reinterpret_cast<const f32x4*>(&lds[kCF + 8 * g + 4 * h]);
                        const f32x4 w1 = *reinterpret_cast<const f32x4*>(&lds[kCF + 64 + 8 * g + 4 * h]);
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc2[it][q * 4 + e] = fmaf(first_x0, w1[e], first_x1 * w0[e]) + bd[e];
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc2[it][q * 4 + e] = cur.xc[it * 16 + q * 4 + e] + bd[e];
                    }
                }
            }
            if constexpr (SKIP) load_skip_row<SKIP, COND>(p, net, lane, cur, skip_load);      // in flight under GEMM2
            // k-steps 0..15 use o tile 0 (ready); pair 1 is gated under those MFMAs
            gemm_groups<8, 2, 0, 1>(
                lds, kA2, lane, acc2, a, [&](int ks) -> float { return o[ks]; },
                [&](int g) {
                    if (g < 4) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            o[16 + 4 * g + e] = gate_act(acc[1][4 * g + e], acc[3][4 * g + e]);
                            asm volatile("" : "+v"(o[16 + 4 * g + e]));
                        }
                    }
                },
                [&](f32x4(&n)[4]) {
                    if constexpr (SKIP) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) n[i] = frag(lds, kAS, i, 8, 0, lane);
                    }
                });
            if (cur.valid) {
#pragma unroll
                for (int g = 0; g < 8; ++g) {
                    const int it = g >> 2, q = g & 3;
                    f32x4 v = {acc2[it][q * 4], acc2[it][q * 4 + 1], acc2[it][q * 4 + 2], acc2[it][q * 4 + 3]};
                    store_wt(out_rs, ooff + g * 1024, v);
                }
            }
        }

        if constexpr (SKIP) {
            // ---- skip 64 -> 128, accumulated across layers (modules.py:243-250, :147) ----------
            f32x16 accs[4];
#pragma unroll
            for (int it = 0; it < 4; ++it)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const f32x4 bs = *reinterpret_cast<const f32x4*>(&lds[kBS + h * 64 + it * 16 + q * 4]);
#pragma unroll
                    for (int e = 0; e < 4; ++e) accs[it][q * 4 + e] = cur.sk[it * 16 + q * 4 + e] + bs[e];
                }
            gemm_groups<8, 4, 0, 1>(lds, kAS, lane, accs, a, [&](int ks) -> float { return o[ks]; }, no_extra,
                                    [](f32x4(&)[4]) {});
            if (cur.valid) {
                const __amdgpu_buffer_rsrc_t skip_rs = units_rsrc(p.skip[net], u_begin, u_end, 32 * 128 * 4);
                const int soff = units_off(cur.row, h, 128, u_begin);
#pragma unroll
                for (int it = 0; it < 4; ++it)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        f32x4 v = {accs[it][q * 4], accs[it][q * 4 + 1], accs[it][q * 4 + 2], accs[it][q * 4 + 3]};
                        store_wt(skip_rs, soff + (8 * it + 2 * q) * 512, v);
                    }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        unit = HEAD ? unit + WAVES : grab();
    }
