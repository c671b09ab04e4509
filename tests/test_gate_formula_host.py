"""CPU: what the fused gate must compute everywhere.  gate_act (csrc/pwv_layer_common.h) is the one function behind tanh(F) * sigmoid(G) in
every fused kernel; tests/util.gate_emulated restates it in numpy operation by operation.  Here: its worst error over tests/util.gate_plane()
at the stated accuracy of v_exp_f32 / v_rcp_f32 (the bars A, R of assert_gate_plane are 4 x that), five wrong gates that assert_gate_plane
must reject -- so the same assertions on a kernel's output (tests/test_gpu_gate_plane.py) would catch the same change in a kernel --, and the
share of saturated gates in every model the GPU route tests run with tests/util.saturating_weights."""
import numpy as np
import pytest

from oracle import iaf_oracle as O
from tests.util import (GATE_MUTANTS, SATURATED_KINDS, TOL_F32, assert_gate_plane, gate_bounds, gate_emulated, gate_errors, gate_exact,
                        gate_plane, gate_statistics, saturated_case, saturating_weights, small_cfg)


def test_the_plane_is_the_fixed_grid():
    F, G, perm = gate_plane()
    assert F.dtype == G.dtype == np.float32 and F.shape == G.shape == (16384,)
    assert sorted(perm.tolist()) == list(range(16384)) and not np.array_equal(perm, np.arange(16384))
    for axis in (F, G):
        vals = np.unique(axis)
        assert len(vals) == 128 and 0.0 in vals
        for v in (2.0 ** -20, 19.99, 20.0, 20.01, 22.17, 22.2, 39.99, 40.0, 40.01, 44.3, 44.4, 88.0, 1e4, 1e30):
            assert np.float32(v) in vals and np.float32(-v) in vals, v
    assert len(set(zip(F.tolist(), G.tolist()))) == 16384          # every pair of the grid, once
    F2, G2, _ = gate_plane()
    assert F2 is F and G2 is G


def test_emulated_gate_meets_its_own_bars_at_every_rounding():
    """The nine (exp_ulp, rcp_ulp) in {-1, 0, 1}^2: the worst absolute error is a few ulp of 1 (the cancellation in 1 - e1), the worst
    relative error a few ulp plus the rounding of Gs = fp32(G * kG) at |Gs| ~ 57 (2^-24 * 57 * ln 2 = 2.4e-6).  A and R = 4 x the maxima."""
    F, G, _ = gate_plane()
    A, R, worst_abs, worst_rel = gate_bounds()
    print('emulated gate over the plane: worst absolute %.3g, worst relative %.3g -> A = %.3g, R = %.3g' % (worst_abs, worst_rel, A, R))
    assert A == 4 * worst_abs and R == 4 * worst_rel
    # the bars stay what the number formats give: A within 32 ulp of 1, R within 4 x (8 ulp + the argument rounding at 57.7)
    assert 2.0 ** -24 <= worst_abs and A <= 32 * 2.0 ** -24, A
    assert 2.0 ** -24 <= worst_rel and R <= 4 * (8 * 2.0 ** -24 + 2.0 ** -24 * 57.7 * np.log(2)), R
    for e in (-1, 0, 1):
        for r in (-1, 0, 1):
            got = gate_emulated(F, G, e, r)
            a, rel = assert_gate_plane(got, F, G)
            assert (a, rel) == gate_errors(got, F, G) and a <= worst_abs and rel <= worst_rel


def test_reference_of_the_plane_is_tanh_times_sigmoid():
    F, G = np.array([0.0, 1.0, -1.0, 30.0, -30.0, 1e30, -1e30, 2.0]), np.array([0.0, -1.0, 2.0, 50.0, -50.0, -1e30, 1e30, -800.0])
    want = [0.0, np.tanh(1) / (1 + np.e), -np.tanh(1) / (1 + np.exp(-2.0)), 1.0, -np.exp(-50.0), 0.0, -1.0, 0.0]
    assert np.allclose(gate_exact(F, G), want, rtol=1e-15, atol=0)


@pytest.mark.parametrize('mutant', GATE_MUTANTS)
def test_a_wrong_gate_is_rejected(mutant):
    """(a) no clamp, (b) the clamp on Gs only, (c) the clamp at 128 instead of 57.7, (d) the two scale constants swapped, (e) 1 + e1 in place
    of 1 - e1: assert_gate_plane rejects each one's emulated output, and the points it breaks are printed for the record."""
    F, G, _ = gate_plane()
    got = gate_emulated(F, G, mutant=mutant).astype(np.float64)
    A = gate_bounds()[0]
    nonfinite = ~np.isfinite(got)
    wrong = ~nonfinite & (np.abs(np.where(nonfinite, 0, got) - gate_exact(F, G)) > A)
    print('%s: %d points not finite (F in [%s]), %d more beyond A (of 16384)'
          % (mutant, nonfinite.sum(), ', '.join('%g' % v for v in np.unique(F[nonfinite])[:12]), wrong.sum()))
    with pytest.raises(AssertionError):
        assert_gate_plane(got, F, G)
    if mutant in ('no_clamp', 'clamp_g_only', 'clamp_at_128'):
        # every point with Fs >= 128: e1 = inf, (1 - inf) * rcp(inf) = -inf * 0; without the Gs clamp also e2 = inf beside e1 = 0 (0 * inf
        # inside the fma); and finite but wrong where e1 * t overflows although tanh(F) * sigmoid(G) is far above A (F near -44, G in -13 .. 0)
        assert nonfinite[F <= np.float32(-44.4)].all() and not nonfinite[np.abs(F) < 44].any()
        assert nonfinite[(F >= 60) & (G <= -100)].all() == (mutant != 'clamp_g_only')
        assert wrong.any() and (F[wrong] <= np.float32(-39.99)).all()
    else:
        assert not nonfinite.any() and wrong.mean() > 0.25


def test_a_gate_without_the_clamp_fails_even_one_point():
    """The check does not lean on the number of bad points: the right gate with ONE value of the no-clamp gate in it is rejected."""
    F, G, _ = gate_plane()
    good, bad = gate_emulated(F, G), gate_emulated(F, G, mutant='no_clamp')
    i = int(np.flatnonzero(~np.isfinite(bad))[0])
    mixed = good.copy()
    mixed[i] = bad[i]
    assert_gate_plane(good, F, G)
    with pytest.raises(AssertionError, match='not finite'):
        assert_gate_plane(mixed, F, G)


def test_saturating_weights_touch_the_stack_biases_only():
    cfg = small_cfg()
    plain, sat = O.init_weights(cfg, seed=6), saturating_weights(cfg, 6)
    assert list(plain) == list(sat)
    for name in plain:
        leaf = name.rsplit('/', 1)[1]
        if '/dilated_stack/' in name and leaf in ('filter_bias', 'gate_bias'):
            assert sat[name].dtype == np.float32 and sat[name].shape == plain[name].shape
            assert np.abs(sat[name]).max() > 20 and np.abs(sat[name]).max() <= 70 and (np.abs(sat[name]) < 3).any(), name
        else:
            assert np.array_equal(plain[name], sat[name]), name
    again = saturating_weights(cfg, 6)
    assert all(np.array_equal(sat[k], again[k]) for k in sat)


@pytest.mark.parametrize('kind', SATURATED_KINDS)
def test_saturated_models_reach_the_clamp_and_stay_well_conditioned(kind):
    """Every model of the GPU route tests, on the fp64 oracle: at least 10 % of its gate pre-activations have |F| > 20 (tanh saturated, the
    Fs clamp engaged), at least 5 % have G < -40 (the Gs clamp), at least 10 % have both below 3 (the ordinary regime next to them) -- and
    the oracle's own fp32 arithmetic stays within TOL_F32 / 4 of fp64, so a kernel that misses TOL_F32 on these weights is wrong, not
    unlucky.  Conditions on the model, not tolerances: a model that misses them gets another seed."""
    cfg, w, mel, z = saturated_case(kind)
    y, big_f, low_g, ordinary, f_max = gate_statistics(w, mel, z, cfg)
    y32 = O.iaf_vocoder_forward(w, mel, z, cfg, dtype=np.float32)
    err32 = float(np.abs(y32 - y).max())
    print('%s: |F| > 20: %.1f %%, G < -40: %.1f %%, both below 3: %.1f %%, largest |F| %.1f, fp32 oracle against fp64 %.3g, max |y| %.3g'
          % (kind, 100 * big_f, 100 * low_g, 100 * ordinary, f_max, err32, np.abs(y).max()))
    assert np.isfinite(y).all() and big_f >= 0.10 and low_g >= 0.05 and ordinary >= 0.10, (big_f, low_g, ordinary)
    assert f_max > 44.4          # beyond Fs = 128: where a gate without its clamp returns NaN
    assert err32 <= TOL_F32 / 4, err32
