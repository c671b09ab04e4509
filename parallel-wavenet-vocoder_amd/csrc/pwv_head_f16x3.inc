// The fused head in split-fp16 arithmetic, from the skip-bias accumulators through the postprocess1 GEMM: the ONE text of what
// layer_f16x3_kernel<..., HEAD> (one-shot and streaming, pwv_layer_f16x3_body.inc) and the split-fp16 arm of the persistent kernel's tail
// (pwv_persist_tail.inc) run behind the gating of row-tile pair 0 -- the suite asserts that the two are bit-identical.
// Expects: hb (the packed head), HS / H1 (skip and postprocess1 fragments in LDS), lane, h, acc (GEMM1's accumulators), o (o[0..15] gated),
//          oh / ol (tiles 0, 1 split), ah / al, no_extra, and an f32x16 acc1[4] declared by the site.
// Leaves:  acc1 = postprocess1's accumulators (before its relu), for the postprocess2 dot (pwv_head_pp2.inc).
            f32x16 accs[4];      // starts at the skip bias (requested now, lands while pair 1 is gated)
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
            gemm16<4, 4, 0, 1, 4>(HS, lane, accs, ah, al, [&](int s) -> f16x8 { return oh[s]; },
                                  [&](int s) -> f16x8 { return ol[s]; }, no_extra,
                                  [&](f16x8(&nh)[4], f16x8(&nl)[4]) { first_frags<8, 4, 0, 1, 4>(H1, lane, nh, nl); });
            // acc1 starts at the postprocess1 bias
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
            gemm16<8, 4, 0, 1, 4>(H1, lane, acc1, ah, al, [&](int s) -> f16x8 { return sh[s]; },
                                  [&](int s) -> f16x8 { return sl[s]; }, no_extra, [](f16x8(&)[4], f16x8(&)[4]) {});
