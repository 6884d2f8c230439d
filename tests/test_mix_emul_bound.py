"""What the label criterion of clip mixing resolves, shown without a GPU: tests/mix_emul.py (the per-cell walk of hftt_labels_render_mix in
numpy) is the reference's note2label with one source, is the reference on the concatenated list with two, and is NOT what max-combining two
separate renders gives -- the velocity track reads the combined onset track and a carried vel == 0 test.  And the host half of the draws:
WaveAugment's mix arguments, draw_mix on a CPU generator, and that mix_p = 0 leaves the other draws' streams alone."""
import numpy as np
import pytest
import torch

import mix_emul as M
import warp_emul as W

CFG = W.LABEL_CFG
PITCHES = (40, 41, 42)
TRACKS = ('onset', 'offset', 'mpe', 'velocity')


def _reference(notes, dt, length):
    from corpus.conv_note2label import note2label_arrays
    a = note2label_arrays(CFG, notes, dt)
    return tuple(a[k][:length] for k in TRACKS), a['onset'].shape[0]


def _two_lists(seed):
    rng = np.random.default_rng(seed)
    while True:
        a, b = M.draw_notes(rng, 40, PITCHES), M.draw_notes(rng, 40, PITCHES)
        if not M.cross_touch(a, b):
            return a, b


@pytest.mark.parametrize('dt', [False, True], ids=['tol50ms', 'duration_tolerance'])
def test_one_source_is_note2label(dt):
    for notes in (W.LABEL_NOTES, W.LABEL_NOTES_LONG, [], _two_lists(1)[0]):
        want, nf = _reference(notes, dt, None)
        got = M.mix_labels(CFG, {'notes': notes, 'start': 0}, None, nf, duration_tolerance=dt)
        for name, g, e in zip(TRACKS, got, want):
            assert g.dtype == e.dtype and np.array_equal(g, e), (name, int((g != e).sum()))
        # a window across both ends, frames outside the file zero
        got = M.mix_labels(CFG, {'notes': notes, 'start': -5}, None, nf + 9, duration_tolerance=dt)
        for g, e in zip(got, want):
            assert np.array_equal(g[5:5 + nf], e) and not g[:5].any() and not g[5 + nf:].any()


@pytest.mark.parametrize('dt', [False, True], ids=['tol50ms', 'duration_tolerance'])
def test_two_sources_are_note2label_of_the_joined_list_and_max_combining_is_not(dt):
    """40 + 40 notes over three pitches on a 1 / 1024 s grid: the partner walked behind the primary is the reference on A + B in all four tracks
    (frames below both files' counts); two separate renders combined by maximum differ from it in the velocity track"""
    carried = wrong = 0
    for seed in range(4):
        a, b = _two_lists(seed)
        nfa, nfb = _reference(a, dt, None)[1], _reference(b, dt, None)[1]
        length = min(nfa, nfb)
        want, _ = _reference(a + b, dt, length)
        A, B = {'notes': a, 'start': 0}, {'notes': b, 'start': 0}
        got = M.mix_labels(CFG, A, B, length, a_frames=length, duration_tolerance=dt)
        for name, g, e in zip(TRACKS, got, want):
            assert g.dtype == e.dtype and np.array_equal(g, e), (seed, name, int((g != e).sum()))
        alone = M.mix_labels(CFG, A, None, length, duration_tolerance=dt)
        carried += int((got[3] != alone[3]).sum())
        short = M.max_combined(CFG, A, B, length, a_frames=length, duration_tolerance=dt)
        assert all(np.array_equal(s, e) for s, e in zip(short[:3], want[:3]))       # onset, offset and mpe ARE maxima: the velocity is what is carried
        diff = int((short[3] != want[3]).sum())
        assert diff > 0, seed
        wrong += diff
    print('velocity cells that differ from the primary alone: %d; cells the max-combined render gets wrong: %d (4 draws)' % (carried, wrong))
    assert carried >= 100           # the comparison does exercise the carried state


def test_the_partner_is_gated_by_its_own_file_and_by_the_primarys_audio():
    a, b = W.LABEL_NOTES, W.LABEL_NOTES_LONG
    A = {'notes': a, 'start': 0}
    none = M.mix_labels(CFG, A, None, 80)
    # a_frames = 0: the partner never counts; a partner window behind its file's end neither
    for B, af in (({'notes': b, 'start': 0}, 0), ({'notes': b, 'start': 100000}, 80)):
        assert all(np.array_equal(x, y) for x, y in zip(M.mix_labels(CFG, A, B, 80, a_frames=af), none))
    # a silent primary (no notes: one label frame) does not hide an audible partner: a_frames, not nframe_A, gates it
    quiet = {'notes': [], 'start': 0}
    got = M.mix_labels(CFG, quiet, {'notes': b, 'start': 0}, 80, a_frames=50)
    want = M.mix_labels(CFG, {'notes': b, 'start': 0}, None, 80)
    assert got[0][:50].any() and all(np.array_equal(g[:50], w[:50]) and not g[50:].any() for g, w in zip(got, want))
    # the partner's start is an integer frame shift of its own file
    got = M.mix_labels(CFG, quiet, {'notes': b, 'start': 7}, 60, a_frames=60)
    assert all(np.array_equal(g, w[7:67]) for g, w in zip(got, M.mix_labels(CFG, {'notes': b, 'start': 0}, None, 80)))


def test_wave_augment_mix_arguments_and_draws():
    from hftt_hip import HfttError
    from training.dataset import WaveAugment
    a = WaveAugment()
    assert (a.mix_p, a.mix_gain_db, a.mixes) == (0.0, (-6.0, 0.0), False)
    assert WaveAugment(mix_p=0.25).mixes and not WaveAugment(mix_p=0.25).warps
    for kw, what in ((dict(mix_p=1.5), 'mix_p'), (dict(mix_p=-0.1), 'mix_p'), (dict(mix_gain_db=(0.0, -6.0)), 'mix_gain_db'),
                     (dict(mix_gain_db=(1.0,)), 'mix_gain_db'), (dict(mix_gain_db=None), 'mix_gain_db')):
        with pytest.raises(HfttError, match=what):
            WaveAugment(**kw)
    a = WaveAugment(mix_p=0.5, mix_gain_db=(-12.0, -3.0), seed=9)
    a.reset('cpu')
    on, partner, gain = a.draw_mix(256, 37)
    a.reset('cpu')
    on2, partner2, gain2 = a.draw_mix(256, 37)
    assert torch.equal(on, on2) and torch.equal(partner, partner2) and torch.equal(gain, gain2)          # reproducible
    assert on.dtype == torch.bool and partner.dtype == torch.int64 and gain.dtype == torch.float32
    assert 64 < int(on.sum()) < 192 and int(partner.min()) >= 0 and int(partner.max()) <= 36 and len(set(partner.tolist())) > 25
    db = 20 * torch.log10(gain.double())
    assert bool(((db >= -12.0 - 1e-4) & (db <= -3.0 + 1e-4)).all()) and float(db.max() - db.min()) > 6.0
    b = WaveAugment(mix_p=0.5, seed=10)
    b.reset('cpu')
    assert not torch.equal(b.draw_mix(256, 37)[1], partner)
    on1 = WaveAugment(mix_p=1.0)
    on1.reset('cpu')
    assert bool(on1.draw_mix(64, 5)[0].all())


def test_mix_p_zero_makes_no_draw():
    """the gain / noise draws and the warp draws of a batch come out the same whether or not draw_mix was asked in between"""
    from training.dataset import WaveAugment
    kw = dict(gain_db=(-6.0, 6.0), noise_dbfs=(-60.0, -40.0), pitch_semitones=(-2, 2), detune_cents=20, shift=True, seed=4)
    plain, zero, some = WaveAugment(**kw), WaveAugment(mix_p=0.0, **kw), WaveAugment(mix_p=0.5, **kw)
    outs = []
    for a in (plain, zero, some):
        a.reset('cpu')
        seq = []
        for _ in range(2):
            g, n, seed = a.draw(16)
            w = a.draw_warp(16, 256)
            m = a.draw_mix(16, 100)
            seq += [g, n, torch.tensor(seed), w.step_q24, w.delay_q24, w.shift]
        outs.append((seq, m))
    assert outs[0][1] is None and outs[1][1] is None and outs[2][1] is not None
    assert all(torch.equal(x, y) for x, y in zip(outs[0][0], outs[1][0]))
    assert all(torch.equal(x, y) for x, y in zip(outs[0][0][:6], outs[2][0][:6]))       # the first batch's draws come before the first mix draw
    assert not all(torch.equal(x, y) for x, y in zip(outs[0][0][6:], outs[2][0][6:]))   # ... and a mix draw does move what follows
