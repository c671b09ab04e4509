// Persistent kernel, the unit in exact-fp32 arithmetic (v_mfma_f32_32x32x2_f32; the operands are the rows as loaded, pwv_layer.hip).
// Expects: the unit's top of pwv_persist_tasks.inc -- rxb / rxc, acc (the P row), bias, lastfrag, o, acc2, settle_top, prefetch_next, j, u,
//          nn, t, rc, valid.  Leaves acc2 = the unit's output rows.
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
            hist_store(j, dil_of(j), nn, t, u, rc, valid, xc, (RAGGED && !SHORT) ? top_rec[2] : -1);
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
