// The fused head in exact-fp32 arithmetic, from the skip-bias accumulators through the postprocess1 GEMM: the ONE text of what
// layer_f32_kernel<..., HEAD> (one-shot and streaming, pwv_layer_f32_body.inc) and the fp32 arm of the persistent kernel's tail
// (pwv_persist_tail.inc) run behind the gating of row-tile pair 0.
// Expects: lds, kHS / kH1 (float offsets of the skip and postprocess1 matrices), hb (the packed head), lane, h, acc, o (o[0..15] gated),
//          a (the skip matrix's first fragments), no_extra, an f32x16 acc1[4] declared by the site, and the hook PWV_HEAD_FENCE() in front
//          of each of the two bias loads: empty in the layer kernel; a compiler fence in the tail, where the loads hoisted above the GEMM
//          before them cost the instantiation its last registers.  The site #undefs it.
// Leaves:  acc1 = postprocess1's accumulators (before its relu), for the postprocess2 dot (pwv_head_pp2.inc).
            PWV_HEAD_FENCE();
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
            gemm_groups<8, 4, 0, 1>(lds, kHS, lane, accs, a, [&](int ks) -> float { return o[ks]; }, no_extra,
                                    [&](f32x4(&n)[4]) {
#pragma unroll
                                        for (int i = 0; i < 4; ++i) n[i] = frag(lds, kH1, i, 16, 0, lane);
                                    });
            PWV_HEAD_FENCE();
#pragma unroll
            for (int it = 0; it < 4; ++it)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(hb + kHB1 + h * 64 + it * 16 + q * 4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc1[it][q * 4 + e] = v[e];
                }
            gemm_groups<16, 4, 0, 1>(
                lds, kH1, lane, acc1, a, [&](int ks) -> float { return fmaxf(accs[ks >> 4][ks & 15], 0.f); }, no_extra,
                [](f32x4(&)[4]) {});
