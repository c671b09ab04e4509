// Persistent kernel, the unit in split-fp16 arithmetic (three v_mfma_f32_32x32x16_f16 per k-step, pwv_layer_f16.hip).
// Expects: the unit's top of pwv_persist_tasks.inc -- rxb / rxc, acc (the P row), bias, lastfrag, o, acc2, settle_top, prefetch_next, j, u,
//          nn, t, rc, valid.  Leaves acc2 = the unit's output rows.
            const f16x8* A1 = reinterpret_cast<const f16x8*>(lds + (j & 1) * kSlot);
            const f16x8* A2 = reinterpret_cast<const f16x8*>(lds + (j & 1) * kSlot + kA1Size);

            f16x8 bh[8], bl[8];      // B operands: bh[0..3] = x[t-d], bh[4..7] = x[t]; packed K order: x[t] first (pwv_layer_f16.hip)
            float xc[32];
            // (general loop: the rows to split were requested a unit ago; the 16 P loads of this unit's top are all that was issued behind them.  `vmcnt(16)`
            //  says exactly that -- loads return in order -- and leaves the P row in flight under the split.  As the BUILTIN it also tells the compiler's own
            //  scoreboard, which for loads carried over the loop's back-edge otherwise puts `s_waitcnt vmcnt(0)` here: simm16 = vmcnt 16, expcnt 7, lgkmcnt 15)
            if constexpr (!SHORT) __builtin_amdgcn_s_waitcnt(0x4F70);
#pragma unroll
            for (int k = 0; k < 32; ++k) xc[k] = rxc[k];
            split8<0>(xc, bh[4], bl[4]);
            if constexpr (!SHORT) PT_LAP(16);
            split8<8>(xc, bh[5], bl[5]);
            split8<16>(xc, bh[6], bl[6]);
            split8<24>(xc, bh[7], bl[7]);
            // (the split is register arithmetic, which nothing orders against settle_top's drain: left to itself the compiler runs the drain FIRST, and the
            //  split then starts only when the P row and the previous unit's stores have landed instead of running under them.  The drain is a volatile asm;
            //  so is this, and it needs the split's results.)
            if constexpr (!SHORT)
                asm volatile("" : "+v"(bh[4]), "+v"(bl[4]), "+v"(bh[5]), "+v"(bl[5]), "+v"(bh[6]), "+v"(bl[6]), "+v"(bh[7]), "+v"(bl[7]));
            if constexpr (!SHORT) PT_LAP(17);
            settle_top();
            hist_store(j, dil_of(j), nn, t, u, rc, valid, xc, (RAGGED && !SHORT) ? top_rec[2] : -1);
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
