"""-m gpu: the stand-alone entry points through their engine wrappers inside poisoned, guard-banded buffers (tests/guarded.py), each
against the fp64 / numpy reference its own test already uses, at sizes that end in the middle of a block.  Every case asserts that no
band was touched and that no NaN (the poison of an `empty` output) is left where the op has to write."""
import contextlib

import numpy as np
import pytest
import torch

from oracle import iaf_oracle as O
from tests.guarded import guarded
from tests.util import gate_bounds, gate_exact

pytestmark = pytest.mark.gpu


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


class _Ctx(object):
    """(engine, g) = ctx; ctx.finish() ends a case: synchronise, no sticky word raised, no band touched."""

    def __init__(self, engine, guard):
        self.engine, self.guard = engine, guard

    def __iter__(self):
        return iter((self.engine, self.guard))

    def finish(self):
        torch.cuda.synchronize()
        assert not self.engine.range_flag_raised() and self.engine.persist_status() == 0
        self.guard.check()
        assert self.guard.allocations, 'nothing was allocated through the proxy'


@pytest.fixture()
def ctx(gpu):
    from pwv_amd import audio_frontend, engine, modules
    with guarded(engine, modules, audio_frontend) as g:
        c = _Ctx(engine, g)
        try:
            yield c
        finally:
            torch.cuda.synchronize()
            engine.clear_range_flag()
            engine.clear_persist_status()


@contextlib.contextmanager
def _unguarded(engine):
    """Inside the context: the real torch for a while (the reference run of an op against itself)."""
    proxy, engine.torch = engine.torch, torch
    try:
        yield
    finally:
        engine.torch = proxy


def _out(g, t):
    """`t` as numpy, after: it lies in a guarded allocation and holds no NaN."""
    assert g.holds(t), 'the output does not lie in a guarded allocation'
    a = t.cpu().numpy()
    assert not np.isnan(a.astype(np.float64)).any(), int(np.isnan(a.astype(np.float64)).sum())
    return a


@pytest.mark.parametrize('N,T,Cin,Cout,W,d', [(1, 1, 3, 3, 2, 1), (2, 33, 5, 7, 3, 40)], ids=['T1', 'dilation_beyond_T'])
def test_causal_conv(gpu, ctx, N, T, Cin, Cout, W, d):
    from pwv_amd.modules import causal_conv
    _, g = ctx
    rng = np.random.RandomState(0)
    x, f = rng.randn(N, T, Cin).astype(np.float32), rng.randn(W, Cin, Cout).astype(np.float32)
    want = O.causal_conv_literal(x.astype(np.float64), f.astype(np.float64), d)
    got = _out(g, causal_conv(_t(x, gpu), _t(f, gpu), d))
    assert got.shape == want.shape and np.abs(got - want).max() <= 1e-5 * max(1.0, np.abs(want).max())
    ctx.finish()


@pytest.mark.parametrize('M', [1, 33])
@pytest.mark.parametrize('precision', ['f32', 'f16x3'])
def test_linear(gpu, ctx, precision, M):
    engine, g = ctx
    rng = np.random.RandomState(1)
    K, Nout = 80, 132
    x, w, b = rng.randn(M, K).astype(np.float32), (rng.randn(K, Nout) / np.sqrt(K)).astype(np.float32), rng.randn(Nout).astype(np.float32)
    for relu, bias in ((False, True), (True, False)):
        want = x.astype(np.float64) @ w.astype(np.float64) + (b.astype(np.float64) if bias else 0)
        want = np.maximum(want, 0) if relu else want
        got = _out(g, engine.linear_op(_t(x, gpu), _t(w, gpu), _t(b, gpu) if bias else None, relu, precision=precision))
        assert got.shape == want.shape and np.abs(got - want).max() <= 1e-5
    ctx.finish()


def test_upsample_repeat_and_crop_time(gpu, ctx):
    engine, g = ctx
    rng = np.random.RandomState(2)
    n, t_mel, c, hop, offset, T = 2, 7, 12, 6, 3, 37               # odd T, 37 + 3 <= 7 * 6; the copy moves whole float4s of channels
    frames = rng.randn(n, t_mel, c).astype(np.float32)
    got = _out(g, engine.RepeatedCondition(_t(frames, gpu), hop, offset, T).materialize())
    assert np.array_equal(got, frames[:, (np.arange(T) + offset) // hop])
    x = rng.randn(n, T, c).astype(np.float32)
    got = _out(g, engine.crop_time_op(_t(x, gpu), 29, 3))
    assert np.array_equal(got, x[:, 3:32])
    ctx.finish()


@pytest.mark.parametrize('n', [1, 255, 257, 1025])
def test_noise(gpu, ctx, n):
    """The three forms of the sampler draw one stream: the plain op inside the context equals itself outside it, the capturable form
    (state in device memory) and the packed form (one stream per utterance) equal the plain op bit for bit."""
    engine, g = ctx
    seed, off = (1 << 63) + 12345, 1000
    with _unguarded(engine):                                        # the reference: the plain op as every other test runs it
        want = engine.logistic_noise_op((n,), gpu, seed=seed, offset=off).cpu().numpy()
    assert np.isfinite(want).all() and np.abs(want).max() <= 16.7
    assert np.array_equal(_out(g, engine.logistic_noise_op((n,), gpu, seed=seed, offset=off)), want)
    z = engine.torch.empty((n,), dtype=torch.float32, device=gpu)
    state = engine.torch.zeros((4,), dtype=torch.int64, device=gpu)
    state.copy_(torch.tensor([engine.as_int64_bits(seed), off, 0, 0], dtype=torch.int64))
    assert np.array_equal(_out(g, engine.logistic_noise_stream_op(z, state)), want)
    assert state.cpu().tolist() == [engine.as_int64_bits(seed), off + n, 0, 0]
    ctx.finish()


def test_noise_packed(gpu, ctx):
    engine, g = ctx
    rows, seeds, offs = [33, 1, 64], [5, (1 << 64) - 1, 7], [0, 31, 1 << 40]
    geom = engine.VarlenGeometry(rows, 1, gpu)
    got = _out(g, engine.logistic_noise_packed_op(geom.cu_rows, geom.stream_table(list(zip(seeds, offs))), geom.rows))
    assert got.shape == (98, 1)
    with _unguarded(engine):
        want = np.concatenate([engine.logistic_noise_op((r, 1), gpu, seed=s, offset=o).cpu().numpy() for r, s, o in zip(rows, seeds, offs)])
    assert np.array_equal(got, want)
    ctx.finish()


def _tile(x, C):
    """[rows, C] -> the tile32 order of include/pwv_hip.h, padded with zeros to whole blocks of 32 rows."""
    rows = x.shape[0]
    blocks = (rows + 31) // 32
    pad = np.zeros((blocks * 32, C), x.dtype)
    pad[:rows] = x
    return pad.reshape(blocks, 32, C // 4, 4).transpose(0, 2, 1, 3).reshape(-1)


def _untile(flat, rows, C):
    blocks = flat.size // (32 * C)
    return flat.reshape(blocks, C // 4, 32, 4).transpose(0, 2, 1, 3).reshape(blocks * 32, C)[:rows]


@pytest.mark.parametrize('C', [64, 80, 128])
def test_tile32_converters(gpu, ctx, C):
    """rows = 33: one row into the second block.  The rows of a block behind the last row are not the converter's to write."""
    from pwv_amd import _lib
    engine, g = ctx
    rows = 33
    x = np.random.RandomState(C).randn(1, rows, C).astype(np.float32)
    tiled = engine._cond_operand(_t(x, gpu), _lib.PREC_F32)          # pwv_rows_to_tile32_f32
    assert g.holds(tiled) and tiled.numel() == 64 * C
    got = _untile(tiled.cpu().numpy(), rows, C)
    assert not np.isnan(got).any() and np.array_equal(got, x[0])
    back = engine.torch.empty((rows, C), dtype=torch.float32, device=gpu)
    _lib.check(_lib.lib().pwv_tile32_to_rows_f32(tiled.data_ptr(), back.data_ptr(), rows, C, engine._stream()), 'pwv_tile32_to_rows_f32')
    assert np.array_equal(_out(g, back), x[0])
    ctx.finish()


def _untile_f16(flat, rows, C):
    """fp16 tile32 (include/pwv_hip.h): blocks of 32 rows as [C / 8 chunks][32 rows][8 halfs], chunk 2 s + h, half q = channel
    16 s + 8 (q >> 2) + 4 h + (q & 3)."""
    blocks = flat.size // (32 * C)
    perm = np.array([16 * s + 8 * (q >> 2) + 4 * h + (q & 3) for s in range(C // 16) for h in range(2) for q in range(8)])
    v = flat.reshape(blocks, C // 8, 32, 8).transpose(0, 2, 1, 3).reshape(blocks * 32, C)[:rows]
    out = np.zeros_like(v)
    out[:, perm] = v
    return out


@pytest.mark.parametrize('form', ['f16', 'split'])
def test_condition_to_f16(gpu, ctx, form):
    """pwv_cond_to_f16 / pwv_cond_split_f16 at rows = 33: hi = fp16(v), lo = fp16(v - hi) behind the hi plane."""
    from pwv_amd import _lib
    engine, g = ctx
    rows, C = 33, 80
    x = (np.random.RandomState(9).randn(1, rows, C) * 3).astype(np.float32)
    out = engine._cond_operand(_t(x, gpu), _lib.PREC_F16 if form == 'f16' else _lib.PREC_F16X3)
    floats = 64 * C
    assert g.holds(out) and out.dtype == torch.float16 and out.numel() == (floats if form == 'f16' else 2 * floats)
    flat = out.cpu().numpy()
    hi = x[0].astype(np.float16)
    got_hi = _untile_f16(flat[:floats], rows, C)
    assert not np.isnan(got_hi.astype(np.float32)).any() and np.array_equal(got_hi, hi)
    if form == 'split':
        got_lo = _untile_f16(flat[floats:], rows, C)
        assert not np.isnan(got_lo.astype(np.float32)).any() and np.array_equal(got_lo, (x[0] - hi.astype(np.float32)).astype(np.float16))
    ctx.finish()


@pytest.mark.parametrize('T', [1, 1000])
def test_instance_norm(gpu, ctx, T):
    engine, g = ctx
    rng = np.random.RandomState(T)
    n, c = 2, 64
    x = (rng.randn(n, T, c) * rng.uniform(0.01, 3.0, size=(1, 1, c)) + rng.uniform(-50, 50, size=(1, 1, c))).astype(np.float32)
    gamma, beta = rng.uniform(0.5, 1.5, c).astype(np.float32), rng.randn(c).astype(np.float32)
    x64 = x.astype(np.float64)
    want = gamma * (x64 - x64.mean(axis=1, keepdims=True)) / np.sqrt(x64.var(axis=1, keepdims=True) + 1e-8) + beta
    got = _out(g, engine.instance_norm_op(_t(x, gpu), _t(gamma, gpu), _t(beta, gpu)))
    assert np.abs(got - want).max() <= 2e-5 * max(1.0, np.abs(want).max())
    assert any(a.dtype == torch.uint8 for a in g.allocations)          # its workspace
    ctx.finish()


def test_channel_affine(gpu, ctx):
    """Plain rows (an odd channel count, 99 rows) and a tile32 buffer of 33 rows x 64 channels; one fp32 multiply-add per element:
    within 2^-22 of the fp64 value's magnitude."""
    engine, g = ctx
    rng = np.random.RandomState(4)
    x, s, b = rng.randn(3, 33, 5).astype(np.float32), rng.randn(5).astype(np.float32), rng.randn(5).astype(np.float32)
    want = np.maximum(x.astype(np.float64) * s + b, 0)
    got = _out(g, engine.channel_affine_op(_t(x, gpu), _t(s, gpu), _t(b, gpu), relu=True))
    assert np.abs(got - want).max() <= 2.0 ** -22 * max(1.0, np.abs(want).max())
    rows, C = 33, 64
    x, s, b = rng.randn(rows, C).astype(np.float32), rng.randn(C).astype(np.float32), rng.randn(C).astype(np.float32)
    out = engine.channel_affine_op(_t(_tile(x, C), gpu), _t(s, gpu), _t(b, gpu), tile32_rows=rows, channels=C)
    assert g.holds(out)
    got = _untile(out.cpu().numpy(), rows, C)
    want = x.astype(np.float64) * s + b
    assert not np.isnan(got).any() and np.abs(got - want).max() <= 2.0 ** -22 * max(1.0, np.abs(want).max())
    ctx.finish()


@pytest.mark.parametrize('n', [1, 4097])
def test_add_and_gate(gpu, ctx, n):
    engine, g = ctx
    rng = np.random.RandomState(n)
    a, b = (rng.randn(n) * 3).astype(np.float32), (rng.randn(n) * 3).astype(np.float32)
    assert np.array_equal(_out(g, engine.add_op(_t(a, gpu), _t(b, gpu))), a + b)
    got = _out(g, engine.gate_op(_t(a, gpu), _t(b, gpu)))
    assert np.abs(got - gate_exact(a, b)).max() <= gate_bounds()[0]
    ctx.finish()


def test_range_check(gpu, ctx):
    engine, g = ctx
    x = engine.add_op(_t(np.full(1027, 2.0), gpu), _t(np.full(1027, 1.0), gpu))       # 3.0 everywhere, in a guarded buffer
    engine.range_check_op(x, 3.0, kind=None)
    torch.cuda.synchronize()
    assert not engine.range_flag_raised()
    for bad in (3.5, float('inf'), float('nan')):
        x[-1] = bad
        engine.range_check_op(x, 3.0, kind=None)
        torch.cuda.synchronize()
        assert engine.range_flag_raised(), bad
        engine.clear_range_flag()
    ctx.finish()


def test_mel_front_end(gpu, ctx):
    from pwv_amd import audio_frontend as A
    from pwv_amd.hparam import hparam as hp
    _, g = ctx
    hp.set_hparam_yaml('default')
    s = hp.signal
    rng = np.random.RandomState(5)
    N, L = 2, 800
    t = np.arange(L) / s.sr
    wavs = np.stack([0.3 * np.sin(2 * np.pi * 220 * t) + 0.05 * rng.randn(L), 0.8 * rng.randn(L) * (t > 0.02)]).astype(np.float32)
    want = np.stack([A.wav2melspec_db(w, s.sr, s.n_fft, s.win_length, s.hop_length, s.n_mels, max_db=s.max_db, min_db=s.min_db) for w in wavs])
    got = _out(g, A.wav_to_mel_device(torch.from_numpy(wavs).to(gpu)))
    assert got.shape == want.shape == (N, 1 + L // s.hop_length, s.n_mels)
    assert np.abs(got - want).max() <= 1e-5
    ctx.finish()
