"""What the criterion of tests/warp_emul.py resolves, on the CPU: the numpy fp32 restatement of the warp passes the derived per-sample bound around
the fp64 ideal on every file, step and delay that tests/test_warp_gpu.py runs on the device, and every planted defect fails it.  Then the host
oracle of the warped labels: the two fp64 operations on a note list, through corpus.conv_note2label."""
import numpy as np
import pytest

import clip_logmel_emul as CE
import frontend_emul as FE
import warp_emul as W

STEPS = (W.step_of(1.0), W.step_of(-2.0 + 0.3), 1 << 23, 1 << 25)
DELAYS = (0, int(0.37 * W.ONE), (FE.HOP - 1) << 24)


def _waves():
    return [w.numpy() for w in CE.scene_waves()]


def test_the_table_is_the_hosts_and_the_constants_are_the_headers():
    from hftt_hip import _capi, ops
    assert np.array_equal(W.proto_table().view(np.int32), ops.warp_table_host().view(np.int32))
    assert (W.Z, W.L, W.TABLE_LEN) == (_capi.WARP_ZEROS, _capi.WARP_TABLE_L, _capi.WARP_TABLE_LEN)
    assert (W.STEP_MIN, W.STEP_MAX) == (_capi.WARP_STEP_MIN, _capi.WARP_STEP_MAX)
    t = W.proto_table()
    assert t[0] == 1.0 and t[W.Z * W.L] == 0.0 and t[-1] == 0.0 and len(t) == W.Z * W.L + 2
    # the slope and curvature the bound's derivation assumes, on a grid eight times finer than the table
    u = np.arange(0, W.Z * W.L * 8 + 1) / (W.L * 8.0)
    p = W.proto(u)
    h = u[1] - u[0]
    assert np.abs(np.diff(p)).max() / h <= 1.7 and np.abs(np.diff(p, 2)).max() / h ** 2 <= 4.2
    assert int(np.float32(W.Z) / W.cut_of(1 << 25)) + 2 == W.H_MAX and W.cut_of(1 << 23) == np.float32(0.99)


@pytest.mark.parametrize('step', STEPS)
def test_the_restatement_passes_the_bound(step):
    worst = 0.0
    for delay in DELAYS:
        for f, x in enumerate(_waves()):
            j = np.arange(-5, W.warp_len(len(x), step, delay) + 5)
            got = W.wave_warp_emul(x, step, delay, j)
            ideal, bound = W.wave_warp_ideal(x, step, delay, j)
            bad = W.violations(got, ideal, bound)
            assert len(bad) == 0, (step, delay, f, bad[:4], got[bad[:4]], ideal[bad[:4]], bound[bad[:4]])
            assert not got[(j < 0) | (j >= W.warp_len(len(x), step, delay))].any()
            if bool((bound > 0).any()):
                worst = max(worst, float((np.abs(got - ideal)[bound > 0] / bound[bound > 0]).max()))
            # int16: the dequantised source is the source
            q = CE.dequantize(CE.quantize_i16(CE.scene_waves()[f])).numpy()
            gq = W.wave_warp_emul(q, step, delay, j)
            iq, bq = W.wave_warp_ideal(q, step, delay, j)
            assert len(W.violations(gq, iq, bq)) == 0, (step, delay, f, 'int16')
    print('warp restatement, step %d: worst error / bound %.3f' % (step, worst))


def test_the_staged_sample_passes_the_bound_under_gain_and_noise():
    x = _waves()[0]
    for step, delay in ((STEPS[0], DELAYS[1]), (STEPS[1], DELAYS[2]), (W.ONE, 3 << 24)):
        j = np.arange(-3, W.warp_len(len(x), step, delay) + 3)
        got = W.staged_emul(x, 0, step, delay, j, gain=1.75, noise_std=1e-3, seed=CE.SEED)
        ideal, bound = W.staged_ideal(x, 0, step, delay, j, gain=1.75, noise_std=1e-3, seed=CE.SEED)
        assert len(W.violations(got, ideal, bound)) == 0, (step, delay)


def test_the_identity_is_a_copy():
    x = _waves()[0]
    j = np.arange(-10, len(x) + 300)
    for D in (0, 3, FE.HOP):
        got = W.wave_warp_emul(x, W.ONE, D << 24, j)
        want = np.zeros(len(j), np.float32)
        ok = (j - D >= 0) & (j - D < len(x))
        want[ok] = x[(j - D)[ok]]
        assert np.array_equal(got.view(np.int32), want.view(np.int32))
        assert W.warp_len(len(x), W.ONE, D << 24) == len(x) + D


def test_refused_steps_and_delays_give_zeros():
    x = _waves()[0]
    j = np.arange(0, 50)
    for step, delay in (((1 << 23) - 1, 0), ((1 << 25) + 1, 0), (W.ONE, -1), (W.ONE, (1 << 48) + 1)):
        assert not W.wave_warp_emul(x, step, delay, j).any()


# (defect, file, step, delay): a scene on which the defect must show
PLANTED = [('taps_not_scaled_by_cut', 0, 1 << 25, 0), ('taps_not_scaled_by_cut', 0, STEPS[0], DELAYS[1]),
           ('delay_wrong_sign', 0, STEPS[1], DELAYS[1]), ('delay_wrong_sign', 0, STEPS[0], DELAYS[2]),
           ('n_warped_off_by_one', 3, STEPS[0], 0), ('n_warped_off_by_one', 3, 1 << 23, DELAYS[1]),
           ('neighbour_samples_at_border', CE.SILENT, STEPS[0], 0), ('neighbour_samples_at_border', CE.SILENT, 1 << 25, DELAYS[2]),
           ('noise_keyed_on_source_index', 0, STEPS[0], 0), ('noise_keyed_on_source_index', 0, STEPS[1], DELAYS[1]),
           ('identity_not_bypassed', 0, W.ONE, 0), ('identity_not_bypassed', 0, W.ONE, 3 << 24),
           ('rate_inverted', 0, STEPS[0], 0), ('rate_inverted', 0, STEPS[1], DELAYS[1])]


@pytest.mark.parametrize('defect,f,step,delay', PLANTED, ids=['%s-%d-%d' % (d, s, dl >> 20) for d, _, s, dl in PLANTED])
def test_every_planted_defect_fails_the_bound(defect, f, step, delay):
    waves = _waves()
    x = waves[f]
    j = np.arange(-5, W.warp_len(len(x), step, delay) + 5)
    kw = dict(gain=1.75, noise_std=1e-3, seed=CE.SEED)
    extra = dict(corpus=np.concatenate(waves), samp0=sum(len(w) for w in waves[:f])) if defect == 'neighbour_samples_at_border' else {}
    ideal, bound = W.staged_ideal(x, f, step, delay, j, **kw)
    assert len(W.violations(W.staged_emul(x, f, step, delay, j, **kw), ideal, bound)) == 0
    bad = W.violations(W.staged_emul(x, f, step, delay, j, defect=defect, **kw, **extra), ideal, bound)
    assert len(bad) > 0, defect
    assert set(d for d, *_ in PLANTED) == set(W.DEFECTS)


# ------------------------------------------------------------------------------------------------
CFG, NOTES = W.LABEL_CFG, W.LABEL_NOTES


def test_labels_oracle_is_note2label_under_the_two_operations():
    from corpus.conv_note2label import note2label_arrays
    a = note2label_arrays(CFG, NOTES, False)
    nf = a['onset'].shape[0]
    same = W.labels_oracle(CFG, NOTES, 0, 0.0, 1.0, 0, nf)             # (t + 0.0) * 1.0 = t
    for k, t in zip(('onset', 'offset', 'mpe', 'velocity'), same):
        assert np.array_equal(t, a[k]), k
    # k = 0 with a non-zero delay: the tracks move later by a fraction of a frame, so the onset peak changes but no pitch does
    step, delay = W.ONE, 100 << 24
    on, off, mpe, vel = W.labels_oracle(CFG, NOTES, 0, W.t_delay_of(delay, 16000), W.t_scale_of(step), 0, nf + 1)
    assert not np.array_equal(on[:nf], a['onset']) and np.array_equal(on.any(0), np.pad(a['onset'], ((0, 1), (0, 0))).any(0))
    # a shift moves the columns, the times follow the rate: +3 semitones plays 2^(3/12) times faster
    step = W.step_of(3.0)
    w = W.warp_notes(NOTES, 3, 0.0, W.t_scale_of(step), 21, 88)
    assert [n['pitch'] for n in w] == [63, 63, 26, 67, 63] and len(w) == len(NOTES) - 1          # 107 + 3 leaves the range
    assert abs(w[4 - 1]['offset'] - 0.900009 / 2 ** 0.25) < 1e-6
    # the flags of the warped and the unwarped list agree: equal times stay equal, distinct ones stay distinct
    for shift, d in ((-2, DELAYS[1]), (0, DELAYS[2]), (3, 0)):
        wl = W.warp_notes(NOTES, shift, W.t_delay_of(d, 16000), W.t_scale_of(W.step_of(shift + 0.2)), 21, 88)
        kept = [n for n in NOTES if 21 <= n['pitch'] + shift < 109]
        for a_, b_ in zip(kept, wl):
            fa = any(a_['offset'] == o['onset'] for o in kept if o['pitch'] == a_['pitch'])
            fb = any(b_['offset'] == o['onset'] for o in wl if o['pitch'] == b_['pitch'])
            assert fa == fb
