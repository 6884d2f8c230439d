"""The audio front end, hftt_logmel and hftt_resample (csrc/logmel.hip), against fp64 under the rounding-model criteria of
tests/frontend_emul.py (derivations there; tests/test_frontend_emul_bound.py shows on the CPU what they resolve, case by case).

Log-mel: twelve signals -- digital silence, unit impulses, a bin-centred tone at three amplitudes, a loud tone beside one at 1e-4, a
constant, the Nyquist alternation, noise at the log offset, test_logmel's own waveform -- crossed with lengths below hop, at and around
multiples of hop, odd, below and around n_fft; the output sits between two NaN guard rows.  A NaN sample stays inside the frames that
contain it.  Resampler: seven input rates, lengths from one sample to three workgroups of outputs, noise under the criterion and unit
impulses whose response is the kernel table to the bit.  Every case is a few frames / a few hundred outputs; the fp64 references are
evaluated once on the host.  Each test prints its worst error / bound (a measurement of the model's margin, not an assertion).
"""
import ctypes as C
import functools

import pytest
import torch

import frontend_emul as FE

pytestmark = pytest.mark.gpu
GUARD = -8192.0


def _lib():
    from hftt_hip import _capi
    return _capi, _capi.lib()


def _st(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _tables():
    return FE.logmel_tables()


@functools.lru_cache(maxsize=None)
def _logmel_ref(signal, n):
    x = FE.logmel_signal(signal, n)
    return x, FE.logmel_ref(x, _tables())


@pytest.fixture(scope='module')
def lm(dev):
    from hftt_hip import ops
    return ops.LogMel(dev)


def _logmel_guarded(lm, wave):
    """hftt_logmel writing into rows 1 .. n_frames of a NaN-filled [n_frames + 2, n_mels] buffer.  Returns (feat, guards bit-unchanged)."""
    capi, L = _lib()
    dev = lm.device
    wave = wave.to(dev).contiguous()
    n = wave.numel()
    F = 1 + n // lm.hop
    buf = torch.full((F + 2, lm.n_mels), float('nan'), device=dev)
    before = _bits(buf).clone()
    d = capi.LogmelDesc()
    d.wave, d.n_samples = wave.data_ptr(), n
    d.n_fft, d.hop, d.n_mels, d.n_frames = lm.n_fft, lm.hop, lm.n_mels, F
    d.window, d.twiddle = lm.window.data_ptr(), lm.twiddle.data_ptr()
    d.fb_start, d.fb_len, d.fb_off, d.fb_w = lm.fb_start.data_ptr(), lm.fb_len.data_ptr(), lm.fb_off.data_ptr(), lm.fb_w.data_ptr()
    d.log_offset = lm.log_offset
    d.feat = buf[1].data_ptr()
    capi.check(L.hftt_logmel(C.byref(d), _st(dev)), 'logmel')
    after = _bits(buf)
    return buf[1:F + 1].clone(), bool(torch.equal(after[0], before[0]) and torch.equal(after[F + 1], before[F + 1]))


def test_the_device_holds_the_tables_of_the_criterion(lm):
    t = _tables()
    for name in ('window', 'twiddle', 'fb_start', 'fb_len', 'fb_off', 'fb_w'):
        assert torch.equal(getattr(lm, name).cpu(), t[name]), name
    assert FE.f32(lm.log_offset) == t['log_offset'] and lm.hop == t['hop'] and lm.n_fft == t['n_fft'] and lm.n_mels == t['n_mels']


@pytest.mark.parametrize('signal', list(FE.LOGMEL_CASES))
def test_logmel_against_fp64(lm, signal):
    worst = 0.0
    for n in FE.LOGMEL_CASES[signal]:
        x, ref = _logmel_ref(signal, n)
        feat, guards_ok = _logmel_guarded(lm, x)
        assert feat.shape == (1 + n // 256, 256), (signal, n)
        assert guards_ok, (signal, n, 'a guard row was written')
        bad = FE.logmel_check(feat.cpu(), ref)
        print('logmel %s n = %d: worst error / bound %.3f' % (signal, n, FE.logmel_ratio(feat.cpu(), ref)))
        assert not bad, (signal, n, bad)
        worst = max(worst, FE.logmel_ratio(feat.cpu(), ref))
        out = lm(x.to(lm.device))              # the wrapper model/amt.py calls: the same launch, its own allocation
        assert out.shape == feat.shape and torch.equal(_bits(out), _bits(feat)), (signal, n)
    print('logmel %s: worst error / bound %.3f' % (signal, worst))


@pytest.mark.parametrize('n,s', [(4219, 1500), (4219, 4218), (2304, 1), (1025, 1023), (257, 129)])
def test_a_nan_sample_stays_in_the_frames_that_contain_it(lm, n, s):
    """Frame f holds the samples f hop - 1024 .. f hop + 1023.  With a NaN at sample s, the frames with |f hop - s| >= 1024 are bit-equal to
    the run without it, the others NaN in every mel with fb_len > 0.  (The positions are no multiples of hop: at f hop - s = 1024 exactly the
    sample is the frame's first, under window[0] = 0, and 0 * NaN = NaN -- in torch.stft as here -- which the first clause would not grant.)"""
    assert s % 256 != 0
    x = FE.logmel_signal('test_logmel_wave', n)
    clean, ok0 = _logmel_guarded(lm, x)
    y = x.clone(); y[s] = float('nan')
    dirty, ok1 = _logmel_guarded(lm, y)
    assert ok0 and ok1
    assert bool(torch.isfinite(clean).all())
    f = torch.arange(1 + n // 256)
    far = (f * 256 - s).abs() >= 1024
    assert int((~far).sum()) > 0 and (n < 2048 or int(far.sum()) > 0)
    assert torch.equal(_bits(dirty[far.to(dirty.device)]), _bits(clean[far.to(clean.device)])), (n, s)
    live = (lm.fb_len > 0)
    assert bool(torch.isnan(dirty[(~far).to(dirty.device)][:, live]).all()), (n, s)


# ================================================================================================ resampler
def _resample_guarded(dev, x, kd, up, down, width):
    """hftt_resample writing n_out = ceil(n up / down) samples between two guard elements.  Returns (out, guards untouched)."""
    capi, L = _lib()
    x = x.to(dev).contiguous()
    n = x.numel()
    n_out = FE.resample_n_out(n, up, down)
    buf = torch.full((n_out + 2,), GUARD, device=dev)
    d = capi.ResampleDesc()
    d.wave, d.n_in, d.kernel = x.data_ptr(), n, kd.data_ptr()
    d.up, d.down, d.width, d.taps = up, down, width, kd.shape[1]
    d.out, d.n_out = buf[1:].data_ptr(), n_out
    capi.check(L.hftt_resample(C.byref(d), _st(dev)), 'resample')
    return buf[1:n_out + 1].clone(), float(buf[0]) == GUARD and float(buf[-1]) == GUARD


@pytest.mark.parametrize('sr', FE.RESAMPLE_RATES)
def test_resample_against_fp64_and_the_table(dev, sr):
    from hftt_hip import ops
    kern, up, down, width = FE.resample_table(sr)
    kd = kern.to(dev)
    worst = 0.0
    for n in FE.resample_lengths(up, down, kern.shape[1]):
        x = FE.resample_noise(n, n)
        ref = FE.resample_ref(x, kern, up, down, width)
        got, guards_ok = _resample_guarded(dev, x, kd, up, down, width)
        assert got.numel() == -(-n * 16000 // sr), (sr, n)                     # the length contract: ceil(n up / down)
        assert guards_ok, (sr, n, 'a guard element was written')
        bad = FE.resample_check(got.cpu(), ref)
        assert not bad, (sr, n, bad)
        worst = max(worst, FE.resample_ratio(got.cpu(), ref))
        out = ops.resample(x.to(dev), sr, 16000)                               # the wrapper model/amt.py calls
        assert out.shape == got.shape and torch.equal(_bits(out), _bits(got)), (sr, n)
        for s in sorted({0, n // 2, n - 1}):                                   # unit impulses: the response is the table, to the bit
            imp = torch.zeros(n); imp[s] = 1.0
            got, guards_ok = _resample_guarded(dev, imp, kd, up, down, width)
            exp = FE.resample_impulse_expected(kern, up, down, width, n, s)
            assert guards_ok, (sr, n, s)
            assert got.shape == exp.shape and torch.equal(_bits(got.cpu()), _bits(exp)), (sr, n, s)
    print('resample %d -> 16000: worst error / bound %.3f' % (sr, worst))
