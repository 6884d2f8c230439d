"""The fp64 criteria of tests/frontend_emul.py separate right from wrong, without a GPU.

For every case of the GPU tests (tests/test_frontend_fp64_gpu.py reads the same tables of signals, lengths and rates) the defect-free fp32
restatement of each kernel passes its criterion; so does an independent fp32 implementation (oracle.logmel: torch.stft with torch's own
fp32 window, worst error / bound 0.76); every named defect fails it, the log-mel ones in cells whose bound is below 1e-3 log units.  The
fp64 references are held to the oracle's own fp64 paths (oracle.logmel_dft: pad + unfold and explicit DFT matrices; oracle.resample:
conv1d on the fp64 table) to the roundings in which those differ: the fp32 window resp. kernel table and an fp32 return value.  No
criterion excludes an element.  Each test prints its line of the tables below (pytest -s).

Log-mel, defect x signal: lengths at which the defect violates the criterion in a cell whose bound is below 1e-3 / lengths run.  Columns:
zeros, impulse first / last / mid, tone 1e-3 / 0.3 / 30, two tones, constant, nyquist, noise 1e-4, test_logmel's waveform.

    defect                            zero  imp0  impL  impM  t1e-3  t0.3  t30   two   const  nyq  noise  wave
    odd_sample_uses_even_window        0/4   0/4   2/5   3/4   3/3   3/3   3/3   3/3   3/4   4/4   4/4   4/4
    last_sample_dropped                0/4   0/4   2/5   0/4   1/3   1/3   1/3   1/3   1/4   1/4   1/4   1/4     (the last sample in an odd slot: even n)
    frame_start_off_by_one             0/4   4/4   5/5   4/4   3/3   3/3   3/3   3/3   4/4   4/4   4/4   4/4
    split_twiddle_conjugated           0/4   0/4   0/5   0/4   3/3   3/3   3/3   3/3   3/4   3/4   4/4   4/4     (an impulse's |X_k| does not depend on it)
    second_half_turn_sign              0/4   0/4   0/5   0/4   3/3   3/3   3/3   3/3   3/4   4/4   4/4   4/4
    mel_last_weight_dropped            0/4   4/4   5/5   4/4   3/3   3/3   3/3   3/3   4/4   4/4   4/4   4/4
    offset_inside_the_sum              4/4   2/4   3/5   2/4   3/3   0/3   0/3   0/3   0/4   0/4   4/4   0/4     (only at the floor: what no older test reached)
    frames_floor_of_n_minus_1          1/4   2/4   2/5   1/4   1/3   1/3   1/3   1/3   1/4   1/4   1/4   1/4     (n a multiple of hop)

Non-vacuity: the share of cells whose bound exceeds 1e-2 log units, per case (signal, then length: share).  These are the empty bins
beside a loud component, where fp32 itself is that far from fp64 (a constant 1.0: 5e-3 in 1 % of the cells).

    zeros              1: 0.000   256: 0.000   1025: 0.000   4219: 0.000
    impulse_first      1: 0.000   255: 0.000   1024: 0.000   2304: 0.000
    impulse_last       1: 0.000   257: 0.000   1024: 0.000   2047: 0.000   2304: 0.000
    impulse_mid        255: 0.000   1023: 0.000   2304: 0.000   4219: 0.000
    tone_1e-3          257: 0.000   1024: 0.000   4219: 0.000
    tone_0.3           255: 0.000   2304: 0.566   4219: 0.702
    tone_30            1023: 0.321   1024: 0.348   4219: 0.702
    two_tone           1025: 0.348   2304: 0.566   4219: 0.702
    constant           1: 0.000   256: 0.000   2047: 0.354   4219: 0.657
    nyquist            255: 0.000   256: 0.000   1025: 0.001   4219: 0.740
    noise_1e-4         257: 0.000   2047: 0.000   2304: 0.000   4219: 0.000
    test_logmel_wave   1023: 0.000   1024: 0.000   1025: 0.000   4219: 0.001
    all cases: 20090 of 84736 cells = 0.237     (asserted below one quarter; with the statistical l2 magnitude of frontend_emul: 0.118)

The restatement's worst error / bound is 0.70 (log-mel; 0.25 outside the cells that sit on the floor guard) and 0.37 (resampler).

Resampler, defect x input rate: cases (length x {noise, three impulses}) at which the defect violates the criterion or the bit-exact
impulse response / cases run.

    defect                           44100  48000  22050  32000   8000  11025  96000
    phase_row_off_by_one             40/40   0/36  40/40   0/32  24/24  36/36   0/40     (up = 1 has one row)
    window_base_ignores_width        40/40  36/36  40/40  32/32  24/24  36/36  40/40
    tail_taps_dropped                 0/40   0/36   2/40   0/32  12/24   1/36   0/40     (taps % 4 = 0 at 32000 / 96000; the outermost taps lie past the
                                                                                          window's end, where the table holds exact zeros)
    block_window_one_frame_short     17/40   0/36  23/40   0/32   0/24  20/36   0/40     (up = 1, 2: the taps lost are those exact zeros)

The oracle's own fp32 filterbank (oracle.mel_filterbank) is a second restatement of torchaudio's and not the device's table: a mel's weights
sum to within 8.5e-6 of the table's, its smallest weights differ by 2 %.  That is a difference between tables, outside the kernel's
arithmetic, and stays unpinned with torchaudio itself; the two oracle comparisons below therefore hand the oracle the device's table.
"""
import functools

import pytest
import torch

import util
import frontend_emul as FE

TIGHT, LOOSE = 1e-3, 1e-2          # log units: a defect must show where the bound is below TIGHT; a cell whose bound exceeds LOOSE is open


@functools.lru_cache(maxsize=None)
def _tables():
    return FE.logmel_tables()


@functools.lru_cache(maxsize=None)
def _logmel_case(signal, n):
    """(wave, fp64 reference, max(up, down) bound) -- computed once, shared by every test below and never written to"""
    x = FE.logmel_signal(signal, n)
    ref = FE.logmel_ref(x, _tables())
    assert all(bool(torch.isfinite(v).all()) for v in ref.values() if torch.is_tensor(v))
    up, down = FE.logmel_bound(ref)
    return x, ref, torch.maximum(up, down)


# ------------------------------------------------------------------------------------------------ log-mel
@pytest.mark.parametrize('signal', list(FE.LOGMEL_CASES))
def test_logmel_restatement_passes(signal):
    for n in FE.LOGMEL_CASES[signal]:
        x, ref, _ = _logmel_case(signal, n)
        got = FE.logmel_emul(x, _tables())
        assert got.shape == (1 + n // FE.HOP, 256)
        bad = FE.logmel_check(got, ref)
        assert not bad, (signal, n, bad)


def test_every_length_is_run_and_every_signal_meets_an_odd_length_and_a_multiple_of_hop():
    assert {n for ns in FE.LOGMEL_CASES.values() for n in ns} == set(FE.LOGMEL_LENGTHS)
    for s, ns in FE.LOGMEL_CASES.items():
        assert len(ns) >= 3 and any(n % 2 for n in ns) and any(n % FE.HOP == 0 for n in ns), s


def test_an_independent_fp32_fft_passes(monkeypatch):
    """oracle.logmel -- torch.stft in fp32 with torch's own fp32 hann window, a dense fp32 matmul -- given the device's filterbank.  (The
    oracle's own fp32 filterbank is another restatement of torchaudio's: a mel's weights sum to within 8.5e-6 of the device table's, its
    smallest weights differ by 2 %.  That is a difference of tables, not of arithmetic; the module docstring records it.)"""
    W32 = FE._fb_dense(_tables(), torch.float32)
    monkeypatch.setattr(util.O, 'mel_filterbank', lambda *a, **k: W32)
    worst = 0.0
    for signal, n in FE.logmel_cases():
        x, ref, _ = _logmel_case(signal, n)
        got = util.O.logmel(x)
        bad = FE.logmel_check(got, ref)
        assert not bad, (signal, n, bad)
        worst = max(worst, FE.logmel_ratio(got, ref))
    print('oracle.logmel (torch.stft, fp32): worst error / bound %.3f' % worst)


def test_the_reference_is_not_self_referential(monkeypatch):
    """oracle.logmel_dft (its own framing by pad + unfold, explicit cos / sin DFT matrices in fp64) against logmel_ref (gather + rfft).
    The two differ by what logmel_dft rounds differently: its window is the fp64 hann, the table's is that rounded to fp32 (1 U32 of
    sum |x w| on X_k, a deterministic perturbation: the l1 magnitude whatever the criterion uses), and its result is returned in fp32
    (1 U32 of |log|).  No other term of the criterion is granted: c_pow = 0, no rounding in the filterbank sum."""
    monkeypatch.setattr(util.O, 'mel_filterbank', lambda *a, **k: FE._fb_dense(_tables(), torch.float32))
    for signal, n in FE.logmel_cases():
        x, ref, _ = _logmel_case(signal, n)
        bad = FE.logmel_check(util.O.logmel_dft(x), ref, norm='l1', c_fft=1, c_pow=0, c_sum=0, c_log=1)
        assert not bad, (signal, n, bad)


def _defect_cells(signal, n, defect):
    """(cells violating, of those the ones whose bound is below TIGHT).  A missing frame counts as unwritten (NaN) cells."""
    x, ref, bound = _logmel_case(signal, n)
    got = FE.logmel_emul(x, _tables(), defect=defect).double()
    if got.shape != ref['out'].shape:
        assert FE.logmel_check(got, ref), 'a wrong shape must violate'
        pad = torch.full_like(ref['out'], float('nan'))
        pad[:got.shape[0]] = got
        got = pad
    up, down = FE.logmel_bound(ref)
    err = got - ref['out']
    bad = ~(torch.where(err >= 0, err <= up, -err <= down))
    assert bool(bad.any()) == bool(FE.logmel_check(FE.logmel_emul(x, _tables(), defect=defect), ref))
    return int(bad.sum()), int((bad & (bound < TIGHT)).sum())


@pytest.mark.parametrize('defect', FE.LOGMEL_DEFECTS)
def test_logmel_defect_fails_where_the_bound_is_tight(defect):
    row = []
    caught_tight = 0
    for signal, ns in FE.LOGMEL_CASES.items():
        hit = [_defect_cells(signal, n, defect) for n in ns]
        caught_tight += sum(1 for h in hit if h[1])
        row.append('%d/%d' % (sum(1 for h in hit if h[1]), len(ns)))
    print('    %-30s %s' % (defect, ' '.join('%5s' % r for r in row)))
    assert caught_tight, 'no case sees %s in a cell whose bound is below %g' % (defect, TIGHT)


def test_the_logmel_bound_is_not_vacuous():
    """the share of cells whose bound exceeds LOOSE, per case (printed) and over all cases together: below one quarter"""
    loose = total = 0
    for signal, ns in FE.LOGMEL_CASES.items():
        parts = []
        for n in ns:
            b = _logmel_case(signal, n)[2]
            k = int((b > LOOSE).sum())
            loose += k; total += b.numel()
            parts.append('%d: %.3f' % (n, k / b.numel()))
        print('    %-18s %s' % (signal, '   '.join(parts)))
    print('    all cases: %d of %d cells = %.3f' % (loose, total, loose / total))
    assert loose / total < 0.25


# ------------------------------------------------------------------------------------------------ resampler
@functools.lru_cache(maxsize=None)
def _rs_table(sr):
    return FE.resample_table(sr)


def _rs_signals(n):
    """noise, and unit impulses at the first, the last and a middle sample: (name, wave, impulse position or None)"""
    out = [('noise', FE.resample_noise(n, n), None)]
    for name, s in (('impulse_first', 0), ('impulse_last', n - 1), ('impulse_mid', n // 2)):
        x = torch.zeros(n); x[s] = 1.0
        out.append((name, x, s))
    return out


@pytest.mark.parametrize('sr', FE.RESAMPLE_RATES)
def test_resample_restatement_passes(sr):
    kern, up, down, width = _rs_table(sr)
    for n in FE.resample_lengths(up, down, kern.shape[1]):
        for name, x, s in _rs_signals(n):
            ref = FE.resample_ref(x, kern, up, down, width)
            got = FE.resample_emul(x, kern, up, down, width)
            assert got.numel() == -(-n * 16000 // sr)
            bad = FE.resample_check(got, ref)
            assert not bad, (sr, n, name, bad)
            if s is not None:                  # the impulse response is the table, to the bit
                exp = FE.resample_impulse_expected(kern, up, down, width, n, s)
                assert torch.equal(got.view(torch.int32), exp.view(torch.int32)), (sr, n, name)


@pytest.mark.parametrize('sr', FE.RESAMPLE_RATES)
def test_resample_reference_is_not_self_referential(sr):
    """oracle.resample (conv1d in fp64 on its own fp64 table) against resample_ref (gather on the fp32 table): they differ by the table's
    rounding, 1 U32 of sum |x k|, and by oracle.resample's fp32 return, 1 U32 of the result"""
    kern, up, down, width = _rs_table(sr)
    for n in FE.resample_lengths(up, down, kern.shape[1]):
        x = FE.resample_noise(n, n)
        ref = FE.resample_ref(x, kern, up, down, width)
        o = util.O.resample(x, sr, 16000)
        assert o.shape == ref['out'].shape
        assert not FE.violations('oracle.resample', o, ref['out'], FE.U32 * (ref['scale'] + ref['out'].abs()) + FE.F32_TINY), (sr, n)


@pytest.mark.parametrize('defect', FE.RESAMPLE_DEFECTS)
def test_resample_defect_fails(defect):
    row = []
    for sr in FE.RESAMPLE_RATES:
        kern, up, down, width = _rs_table(sr)
        hit = cases = 0
        for n in FE.resample_lengths(up, down, kern.shape[1]):
            for name, x, s in _rs_signals(n):
                ref = FE.resample_ref(x, kern, up, down, width)
                got = FE.resample_emul(x, kern, up, down, width, defect=defect)
                wrong = bool(FE.resample_check(got, ref))
                if s is not None and not wrong:
                    exp = FE.resample_impulse_expected(kern, up, down, width, n, s)
                    wrong = not torch.equal(got.view(torch.int32), exp.view(torch.int32))
                hit += wrong; cases += 1
        row.append('%d/%d' % (hit, cases))
    print('    %-30s %s' % (defect, ' '.join('%6s' % r for r in row)))
    assert any(not r.startswith('0/') for r in row), 'no case sees ' + defect
