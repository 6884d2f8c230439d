"""The warp on the device: hftt_wave_warp, hftt_clip_logmel_warp, hftt_labels_render_warp and WaveClipStore.batch under WaveAugment's pitch
shift, detune and time offset.  What the criteria resolve is shown on the CPU by tests/test_warp_emul_bound.py.

  interpolation   hftt_wave_warp = the numpy fp32 restatement (tests/warp_emul.py) to the bit, and inside the derived bound around the fp64 ideal:
                  every step and delay of the issue, windows across both ends of a file and across the full-scale / silent border
  log-mel         hftt_clip_logmel_warp = hftt_clip_logmel on a table of the file's whole hftt_wave_warp output, to the bit (fp32 and int16, gain,
                  gain + noise: the noise is keyed on the warped sample in both), fill cells by bits
  identity        step 2^24 with a whole-sample delay = hftt_clip_logmel at the shifted window to the bit, among warped windows
  labels          hftt_labels_render_warp = corpus.conv_note2label on the warped note list (numpy fp64, the same two operations), bit for bit
  store           reproducible per seed; the null augmentation and p_warp = 0 are the plain batch to the bit; a one-note file's rendered onset
                  frame is where the log-mel energy rises; the semitone clamp keeps every sounding note labelled
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import clip_logmel_emul as CE
import frontend_emul as FE
import warp_emul as W

pytestmark = pytest.mark.gpu
GUARD = 7
HOP = FE.HOP
STEPS = (W.step_of(1.0), W.step_of(-2.0 + 0.3), 1 << 23, 1 << 25)
DELAYS = (0, int(0.37 * W.ONE), (HOP - 1) << 24)


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _quantized():
    return tuple(CE.quantize_i16(w) for w in CE.scene_waves())


@functools.lru_cache(maxsize=None)
def _host_waves(i16):
    return tuple((CE.dequantize(q) if i16 else w).numpy() for q, w in zip(_quantized(), CE.scene_waves()))


@pytest.fixture(scope='module')
def lm(dev):
    from hftt_hip import ops
    return ops.LogMel(dev)


@pytest.fixture(scope='module')
def corpus(dev):
    from hftt_hip import ops
    return {False: ops.WaveTable(CE.scene_waves(), dev, 'float32'), True: ops.WaveTable(_quantized(), dev, 'int16')}


def _warp(dev, steps, delays, shift=None):
    from hftt_hip import ops
    return ops.Warp(torch.tensor(steps, dtype=torch.int32, device=dev), torch.tensor(delays, dtype=torch.int64, device=dev),
                    None if shift is None else torch.tensor(shift, dtype=torch.int32, device=dev))


def _arena(n, dev):
    a = torch.full((n + 2 * GUARD,), float('nan'), device=dev)
    return a, _bits(a).clone()


def _check_arena(a, before, n):
    torch.cuda.synchronize(a.device)
    after = _bits(a)
    assert torch.equal(after[:GUARD], before[:GUARD]) and torch.equal(after[GUARD + n:], before[GUARD + n:]), 'the arena around the output was written'
    out = a[GUARD:GUARD + n].cpu()
    assert not bool(torch.isnan(out).any()), 'an element of the footprint was not written'
    return out


def _wave_warp(table, windows, length, warp):
    """hftt_wave_warp through the C ABI with `out` inside a NaN arena -> [B, length] on the host"""
    from hftt_hip import _capi
    dev = table.device
    B = len(windows)
    arena, before = _arena(B * length, dev)
    wf = torch.tensor([f for f, _ in windows], dtype=torch.int32, device=dev)
    ws = torch.tensor([s for _, s in windows], dtype=torch.int64, device=dev)
    d = _capi.WaveWarpDesc()
    d.wave, d.file_samp0, d.win_file, d.win_start = table.wave.data_ptr(), table.file_samp0.data_ptr(), wf.data_ptr(), ws.data_ptr()
    d.total_samples, d.wave_i16, d.n_files, d.B, d.len = table.total_samples, int(table.dtype == 'int16'), table.n_files, B, length
    d.warp, keep = warp._args('wave_warp', B, dev)
    d.out = arena[GUARD:].data_ptr()
    _capi.check(_capi.lib().hftt_wave_warp(C.byref(d), torch.cuda.current_stream(dev).cuda_stream), 'wave_warp')
    return _check_arena(arena, before, B * length).view(B, length)


def _clip(lm, table, windows, width, gain=None, noise_std=None, seed=0, warp=None):
    """hftt_clip_logmel / hftt_clip_logmel_warp through the C ABI with `out` inside a NaN arena -> [B, n_mels, width] on the host"""
    from hftt_hip import _capi
    dev = table.device
    B, M = len(windows), lm.n_mels
    arena, before = _arena(B * M * width, dev)
    wf = torch.tensor([f for f, _ in windows], dtype=torch.int32, device=dev)
    ws = torch.tensor([s for _, s in windows], dtype=torch.int32, device=dev)
    g = None if gain is None else torch.tensor(gain, dtype=torch.float32, device=dev)
    ns = None if noise_std is None else torch.tensor(noise_std, dtype=torch.float32, device=dev)
    w = _capi.ClipLogmelWarpDesc()
    d = w.base
    d.wave, d.file_samp0, d.win_file, d.win_start = table.wave.data_ptr(), table.file_samp0.data_ptr(), wf.data_ptr(), ws.data_ptr()
    d.total_samples, d.wave_i16, d.n_files, d.B, d.width = table.total_samples, int(table.dtype == 'int16'), table.n_files, B, width
    d.n_fft, d.hop, d.n_mels, d.log_offset = lm.n_fft, lm.hop, M, lm.log_offset
    d.window, d.twiddle = lm.window.data_ptr(), lm.twiddle.data_ptr()
    d.fb_start, d.fb_len, d.fb_off, d.fb_w = lm.fb_start.data_ptr(), lm.fb_len.data_ptr(), lm.fb_off.data_ptr(), lm.fb_w.data_ptr()
    d.fill, d.seed = CE.FILL, seed
    d.gain, d.noise_std = (None if g is None else g.data_ptr()), (None if ns is None else ns.data_ptr())
    d.out = arena[GUARD:].data_ptr()
    st = torch.cuda.current_stream(dev).cuda_stream
    if warp is None:
        _capi.check(_capi.lib().hftt_clip_logmel(C.byref(d), st), 'clip_logmel')
    else:
        w.warp, keep = warp._args('clip_logmel', B, dev)
        _capi.check(_capi.lib().hftt_clip_logmel_warp(C.byref(w), st), 'clip_logmel_warp')
    return _check_arena(arena, before, B * M * width).view(B, M, width)


# ------------------------------------------------------------------------------------------------
LEN = 600          # samples per window: three workgroups, the last one partly filled


def _interp_windows(step, delay):
    """(file, first warped sample): across the start and the end of file 0, the end of the full-scale file 3, the start of the silent file 4
    behind it, and the one-sample file 1"""
    n = [len(w) for w in CE.scene_waves()]
    end = lambda f: W.warp_len(n[f], step, delay)
    return [(0, -7), (0, end(0) - LEN + 250), (3, end(3) - 200), (CE.SILENT, -50), (1, -3)]


@pytest.mark.parametrize('i16', [False, True], ids=['fp32', 'int16'])
@pytest.mark.parametrize('step', STEPS)
def test_interpolation_is_the_restatement_to_the_bit_and_the_ideal_within_the_bound(dev, corpus, step, i16):
    from hftt_hip import ops
    worst = 0.0
    for delay in DELAYS:
        wins = _interp_windows(step, delay)
        warp = _warp(dev, [step] * 5, [delay] * 5)
        assert warp.cut().cpu().tolist() == [float(W.cut_of(step))] * 5
        got = _wave_warp(corpus[i16], wins, LEN, warp).numpy()
        for b, (f, s) in enumerate(wins):
            x = _host_waves(i16)[f]
            j = s + np.arange(LEN)
            want = W.wave_warp_emul(x, step, delay, j)
            assert np.array_equal(got[b].view(np.int32), want.view(np.int32)), (step, delay, b, int((got[b] != want).sum()))
            ideal, bound = W.wave_warp_ideal(x, step, delay, j)
            bad = W.violations(got[b], ideal, bound)
            assert len(bad) == 0, (step, delay, b, bad[:4])
            if bool((bound > 0).any()):
                worst = max(worst, float((np.abs(got[b] - ideal)[bound > 0] / bound[bound > 0]).max()))
        assert not got[3].any(), 'the full-scale neighbour bleeds into the silent file'
        out = ops.wave_warp(corpus[i16], [f for f, _ in wins], [s for _, s in wins], LEN, warp)          # the wrapper: the same launch
        assert torch.equal(_bits(out.cpu()), _bits(torch.from_numpy(got)))
    print('wave_warp step %d %s: worst error / bound %.3f' % (step, 'int16' if i16 else 'fp32', worst))


def test_mixed_windows_refused_warps_and_unknown_files_are_zeros(dev, corpus):
    """one launch, every window its own step and delay; a step or delay outside the contract and a file outside the table give zeros"""
    steps = [STEPS[0], W.ONE, (1 << 23) - 1, STEPS[3], STEPS[1], (1 << 25) + 1, W.ONE]
    delays = [DELAYS[1], 5 << 24, 0, DELAYS[2], 0, 0, (1 << 48) + 1]
    wins = [(0, 100), (0, -2), (0, 0), (6, 300), (8, 0), (0, 0), (0, 0)]
    got = _wave_warp(corpus[False], wins, 333, _warp(dev, steps, delays)).numpy()
    for b in (2, 4, 5, 6):
        assert not got[b].any(), b
    for b in (0, 1, 3):
        want = W.wave_warp_emul(_host_waves(False)[wins[b][0]], steps[b], delays[b], wins[b][1] + np.arange(333))
        assert want.any() and np.array_equal(got[b].view(np.int32), want.view(np.int32)), b


# ------------------------------------------------------------------------------------------------
def _logmel_windows(width, k, steps, delays):
    """the files of clip_logmel_emul's scene, each under its own warp: across the first frame, across the last frame of the WARPED file, from
    frame 0, wholly before, wholly behind"""
    n = [len(w) for w in CE.scene_waves()]
    wins = []
    for b, (f, _) in enumerate(CE.SCENES[width][k]):
        nf = 1 + W.warp_len(n[f], steps[b], delays[b]) // HOP
        wins.append((f, (-3, nf - (width + 1) // 2, 0, -width, nf)[b]))
    return wins


def _whole_file_table(dev, table, f, step, delay):
    """a WaveTable whose file f is the whole hftt_wave_warp output of `table`'s file f (the other files empty: the noise key keeps its file)"""
    from hftt_hip import ops
    n = int(table.file_nsamp_host[f])
    whole = ops.wave_warp(table, [f], [0], W.warp_len(n, step, delay), _warp(dev, [step], [delay]))[0]
    files = [torch.zeros(0)] * table.n_files
    files[f] = whole.cpu()
    return ops.WaveTable(files, dev, 'float32')


@pytest.mark.parametrize('i16', [False, True], ids=['fp32', 'int16'])
@pytest.mark.parametrize('width', [1, 21])
def test_logmel_is_the_unwarped_kernel_on_the_warped_file_to_the_bit(dev, lm, corpus, width, i16):
    steps = [STEPS[0], STEPS[1], STEPS[2], STEPS[3], STEPS[0]]
    delays = [DELAYS[1], DELAYS[2], DELAYS[0], DELAYS[1], DELAYS[2]]
    for k in range(len(CE.SCENES[width])):
        wins = _logmel_windows(width, k, steps, delays)
        warp = _warp(dev, steps, delays)
        for name, kw in (('gain', dict(gain=CE.GAIN)), ('gain+noise', dict(gain=CE.GAIN, noise_std=CE.NOISE_STD, seed=CE.SEED))):
            got = _clip(lm, corpus[i16], wins, width, warp=warp, **kw)
            valid = 0
            for b, (f, s) in enumerate(wins):
                ref = _clip(lm, _whole_file_table(dev, corpus[i16], f, steps[b], delays[b]), [(f, s)], width,
                            **{key: ([v[b]] if key != 'seed' else v) for key, v in kw.items()})
                assert torch.equal(_bits(ref[0]), _bits(got[b])), (width, k, name, b)
                valid += int((_bits(got[b]) != _bits(torch.tensor(CE.FILL))).sum())
            assert valid > 0 or width == 1
        from hftt_hip import ops
        out = ops.clip_logmel(corpus[i16], lm, [f for f, _ in wins], [s for _, s in wins], width, CE.FILL, gain=CE.GAIN, noise_std=CE.NOISE_STD,
                              seed=CE.SEED, warp=warp)
        assert torch.equal(_bits(out.cpu()), _bits(got)), (width, k)


def test_identity_windows_are_the_unwarped_kernel_among_warped_ones(dev, lm, corpus):
    """step 2^24: with delay 0 the same window (noise included: j is the source index), with a delay of two hops the window two frames earlier
    (without noise, which is keyed on the warped index)"""
    steps = [W.ONE, W.ONE, STEPS[0], W.ONE, STEPS[1]]
    delays = [0, (2 * HOP) << 24, DELAYS[1], 0, 0]
    wins = [(0, 3), (0, 5), (0, 3), (CE.SILENT, -3), (6, 0)]
    warp = _warp(dev, steps, delays)
    for i16 in (False, True):
        kw = dict(gain=CE.GAIN, noise_std=CE.NOISE_STD, seed=CE.SEED)
        got = _clip(lm, corpus[i16], wins, 21, warp=warp, **kw)
        plain = _clip(lm, corpus[i16], wins, 21, **kw)
        for b in (0, 3):
            assert torch.equal(_bits(got[b]), _bits(plain[b])), (i16, b)
        assert not torch.equal(_bits(got[2]), _bits(plain[2]))
        got = _clip(lm, corpus[i16], wins, 21, warp=warp, gain=CE.GAIN)
        plain = _clip(lm, corpus[i16], [(0, 3), (0, 3), (0, 3), (CE.SILENT, -3), (6, 0)], 21, gain=CE.GAIN)
        for b in (0, 1, 3):
            assert torch.equal(_bits(got[b]), _bits(plain[b])), (i16, b)
        # the delayed file is two frames longer: its last frames are frames, not fill
        n0 = len(CE.scene_waves()[0])
        tail = _clip(lm, corpus[i16], [(0, CE.n_frames(n0) + 1)] * 5, 1, warp=_warp(dev, [W.ONE] * 5, [(2 * HOP) << 24] * 5))
        assert not bool((_bits(tail) == _bits(torch.tensor(CE.FILL))).any())


# ------------------------------------------------------------------------------------------------
LAB_LEN = 300      # two chunks of 256 frames


@pytest.fixture(scope='module')
def note_table(dev):
    from hftt_hip import ops
    return ops.labels_table([W.LABEL_NOTES, [], W.LABEL_NOTES_LONG], W.LABEL_CFG, dev)


def _nframe(notes, t_delay, t_scale):
    if not notes:
        return 1
    end = max(n['offset'] for n in notes)
    return int(((end + t_delay) * t_scale) * 62.5 + 0.5) + 1


@pytest.mark.parametrize('dt', [False, True], ids=['tol50ms', 'duration_tolerance'])
@pytest.mark.parametrize('form', ['train', 'store'])
def test_labels_are_note2label_of_the_warped_list(dev, note_table, form, dt):
    from hftt_hip import ops
    files = [W.LABEL_NOTES, [], W.LABEL_NOTES_LONG]
    # (file, shift, step, delay): shifts -2, 0, +3; k = 0 with a non-zero delay; +3 drops pitches 107 / 108 and -2 drops pitch 21, none the last to end
    warps = [(0, -2, W.step_of(-2 + 0.3), DELAYS[1]), (0, 0, W.ONE, 100 << 24), (0, 3, W.step_of(3.0), 0), (0, 3, W.step_of(3.2), DELAYS[2]),
             (2, 0, W.step_of(0.3), 0), (2, -2, W.step_of(-2.0), DELAYS[2]), (2, 3, W.step_of(2.8), DELAYS[1]), (1, 3, STEPS[0], DELAYS[1])]
    warp = _warp(dev, [w[2] for w in warps], [w[3] for w in warps], [w[1] for w in warps])
    td, tsc = [W.t_delay_of(w[3], 16000) for w in warps], [W.t_scale_of(w[2]) for w in warps]
    assert warp.t_delay(16000).cpu().tolist() == td and warp.t_scale().cpu().tolist() == tsc      # the device's fp64 quotients are the host's
    nf = [_nframe(files[w[0]], td[b], tsc[b]) for b, w in enumerate(warps)]
    # windows: across the first frame (and, for the short file, the last), across the last frame, behind the file, wholly before it
    for starts in ([-10] * 8, [n - 5 for n in nf], [n + 3 for n in nf], [-LAB_LEN] * 8, [0, -1, nf[2] - LAB_LEN, 1, 40, -7, nf[6] - 256, 0]):
        got = ops.labels_render(note_table, [w[0] for w in warps], starts, LAB_LEN, form=form, duration_tolerance=dt, warp=warp)
        torch.cuda.synchronize(dev)
        for b, w in enumerate(warps):
            want = W.labels_oracle(W.LABEL_CFG, files[w[0]], w[1], td[b], tsc[b], starts[b], LAB_LEN, dt)
            for name, g, e in zip(('onset', 'offset', 'mpe', 'velocity'), got, want):
                g = g[b].cpu().numpy()
                if form == 'train':
                    assert g.dtype == (np.int64 if name == 'velocity' else np.float32)
                    e = e.astype(g.dtype)
                else:
                    assert g.dtype == e.dtype, (name, g.dtype, e.dtype)
                assert np.array_equal(g.view(np.uint8), np.ascontiguousarray(e).view(np.uint8)), (starts[b], b, name, int((g != e).sum()))
    # the unwarped entry point is what it was: shift 0, rate 1, no delay is the same render
    plain = ops.labels_render(note_table, [0, 2], [-3, 100], LAB_LEN, form=form, duration_tolerance=dt)
    ident = ops.labels_render(note_table, [0, 2], [-3, 100], LAB_LEN, form=form, duration_tolerance=dt, warp=_warp(dev, [W.ONE] * 2, [0] * 2, [0, 0]))
    for a, b_ in zip(plain, ident):
        assert torch.equal(a, b_)


# ------------------------------------------------------------------------------------------------
def _note(pitch, onset, offset, velocity=64):
    return {'pitch': pitch, 'onset': onset, 'offset': offset, 'velocity': velocity}


@functools.lru_cache(maxsize=None)
def _store_corpus():
    """(config, waves, notes): a one-note file; a file whose notes touch both ends of the range; a file with a few notes in the middle"""
    from corpus import synth_audio as SA
    from corpus.make_dataset import assemble_wave_store, finalize_config, prepare_config
    config = finalize_config(prepare_config(SA.default_config()))
    notes = [[_note(60, 0.700001, 1.100002, 100)],
             [_note(21, 0.100003, 0.500004, 90), _note(108, 0.300005, 0.700006, 90)],
             [_note(50, 0.050007, 0.400008, 80), _note(64, 0.200009, 0.900011, 70), _note(71, 0.500012, 0.800013, 60)]]
    waves = [SA.pluck_wave(a, dur=d).numpy() for a, d in zip(notes, (1.6, 1.0, 1.2))]
    return config, assemble_wave_store(waves, notes, config)


def _same(a, b):
    return all(torch.equal(_bits(x) if x.dtype == torch.float32 else x, _bits(y) if y.dtype == torch.float32 else y) for x, y in zip(a, b))


def test_store_batches_are_reproducible_and_the_null_warp_is_the_plain_batch(dev):
    from training.dataset import WaveAugment, WaveClipStore
    config, store = _store_corpus()
    ids = list(range(0, len(store['clip_file']), max(1, len(store['clip_file']) // 8)))[:8]
    plain = WaveClipStore(store, config, dev).batch(ids)
    null = WaveClipStore(store, config, dev, augment=WaveAugment(pitch_semitones=(0, 0), detune_cents=0, shift=False)).batch(ids)
    never = WaveClipStore(store, config, dev, augment=WaveAugment(pitch_semitones=(-2, 2), detune_cents=20, shift=True, p_warp=0.0)).batch(ids)
    assert _same(plain, null) and _same(plain, never)                   # (`never` runs the warped kernels: every window takes the identity bypass)
    runs = []
    for seed in (3, 3, 4):
        s = WaveClipStore(store, config, dev, augment=WaveAugment(pitch_semitones=(-2, 2), detune_cents=20, shift=True, seed=seed))
        runs.append([s.batch(ids), s.batch(ids)])
    assert _same(runs[0][0], runs[1][0]) and _same(runs[0][1], runs[1][1])
    assert not _same(runs[0][0], runs[2][0]) and not _same(runs[0][0], runs[0][1]) and not _same(runs[0][0], plain)
    assert all(bool(torch.isfinite(t.float()).all()) for t in runs[0][0])


@pytest.mark.parametrize('k', [-2, 2])
def test_the_rendered_onset_is_where_the_energy_rises(dev, k):
    """one plucked note (it starts at full amplitude): the frame that gains the most linear energy over its predecessor is the frame whose
    window centre passes the attack, which is the onset's frame up to the half-frame between a frame's centre and the attack -- within one frame"""
    from training.dataset import WaveAugment, WaveClipStore
    config, store = _store_corpus()
    mb = config['input']['margin_b']
    s = WaveClipStore(store, config, dev, wave_dtype='float32', augment=WaveAugment(pitch_semitones=(k, k), detune_cents=20, shift=True, seed=11))
    ids = [i for i in range(len(store['clip_file'])) if store['clip_file'][i] == 0 and store['clip_frame'][i] in (0, 10, 30)]
    assert len(ids) == 3
    spec, onset, offset, mpe, velocity = s.batch(ids)
    col = 60 - 21 + k
    assert bool((onset[:, :, col].max(1).values > 0.5).all()) and int((onset.sum(1) > 0).sum()) == 3      # the shifted pitch, and only it
    on_f = onset[:, :, col].argmax(1).cpu()
    energy = torch.exp(spec.double()).sum(1).cpu()                        # [B, margin + frames + margin]
    rise = (energy[:, 1:] - energy[:, :-1]).argmax(1) + 1 - mb           # in label frames
    assert bool(((on_f - rise).abs() <= 1).all()), (on_f.tolist(), rise.tolist())
    # the pitch moved with the label: the strongest mel bin of the frames behind the onset lies above (k > 0) / below (k < 0) the unwarped clip's
    plain = WaveClipStore(store, config, dev, wave_dtype='float32').batch(ids)
    peak = lambda sp, f: int(sp[0, :, mb + int(f) + 4].argmax())
    assert (peak(spec, on_f[0]) - peak(plain[0], plain[1][0, :, 60 - 21].argmax())) * k > 0


def test_the_semitone_clamp_keeps_every_sounding_note_labelled(dev):
    from training.dataset import WaveAugment, WaveClipStore
    config, store = _store_corpus()
    s = WaveClipStore(store, config, dev, augment=WaveAugment(pitch_semitones=(-2, 2), shift=True, seed=2))
    both = [i for i in range(len(store['clip_file'])) if store['clip_file'][i] == 1][:8]
    mid = [i for i in range(len(store['clip_file'])) if store['clip_file'][i] == 2][:8]
    moved = set()
    for _ in range(3):
        mpe = s.batch(both)[3]
        assert set(mpe.sum((0, 1)).nonzero().flatten().tolist()) == {0, 87}          # pitches 21 and 108: only k = 0 keeps both
        cols = [tuple(m.sum(0).nonzero().flatten().tolist()) for m in s.batch(mid)[3]]
        for c in cols:
            assert len(c) in (2, 3) and set(c) <= {p - 21 + k for p in (50, 64, 71) for k in range(-2, 3)}
            moved.add(c[-1] - (71 - 21) if len(c) == 3 else None)
    assert len(moved - {None}) >= 3                                                   # unclamped files do move
