// The postprocess2 dot behind either head fragment: relu(acc1) . w2[q] over the 64 channels (32 per half-wave, joined by one shuffle) + bias,
// the same arithmetic at the four sites (the two layer bodies, the two arms of the tail share one).
// Expects: hb, Q, hq (= h * Q; the tail hands an opaque copy), acc1, and PWV_HEAD_STORE(q, part): the site's store of output q.  The site #undefs it.
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
                        PWV_HEAD_STORE(q, part);
                    }
