"""Clip mixing on the device: hftt_clip_logmel_mix / _mix_warp, hftt_labels_render_mix and WaveClipStore.batch under WaveAugment's mix_p.
What the label criterion resolves is shown on the CPU by tests/test_mix_emul_bound.py.

  audio    every mix_file = -1: the un-mixed kernels to the bit.  With partners (later / earlier start, a partner that ends inside the window, an
           empty partner, the primary's own file at another start, indices out of range, a long partner on a short primary): hftt_clip_logmel on
           a table whose file is the host's premix fl(fl(a g) + fl(b gb)) over the primary's length, to the bit, with and without noise; warped:
           the premix of hftt_wave_warp's output of both sources, to the bit.  Output inside a NaN arena.
  labels   all four tracks np.array_equal to the numpy walker (tests/mix_emul.py): a partner of 300 notes on one pitch (two filter passes),
           partner offsets of both signs, a partner window behind its file, a primary without notes under a_frames, a_frames cutting the
           partner off, either source under a map, both output forms; no partner: hftt_labels_render[_warp] to the bit
  store    mix_p = 0 is the un-mixed store batch for batch; mix_p = 1 trains; a batch's labels are the walker's for the drawn partners
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import mix_emul as M
import util
import warp_emul as W

pytestmark = pytest.mark.gpu
GUARD = 7
HOP = 256
FILL = -18.420681
LENS = (0, 1, 255, 2304, 4219)
SEED = 0x1234_5678_9ABC_DEF1


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _waves():
    """fp32 files of LENS samples: two tones and a little noise, below full scale"""
    r = np.random.RandomState(3)
    out = []
    for k, n in enumerate(LENS):
        t = np.arange(n, dtype=np.float64)
        out.append(torch.from_numpy((0.4 * np.sin(2 * np.pi * (440.0 + 97.0 * k) / 16000.0 * t) + 0.2 * np.sin(2 * np.pi * 1234.5 / 16000.0 * t + k)
                                     + 0.01 * r.standard_normal(n)).astype(np.float32)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _quantized():
    return tuple(torch.round(w.double() * 32768.0).clamp(-32768, 32767).to(torch.int16) for w in _waves())


@functools.lru_cache(maxsize=None)
def _host(i16):
    return tuple((q.float() * (1.0 / 32768.0)).numpy() if i16 else w.numpy() for q, w in zip(_quantized(), _waves()))


@pytest.fixture(scope='module')
def lm(dev):
    from hftt_hip import ops
    return ops.LogMel(dev, n_mels=8)


@pytest.fixture(scope='module')
def corpus(dev):
    from hftt_hip import ops
    return {False: ops.WaveTable(_waves(), dev, 'float32'), True: ops.WaveTable(_quantized(), dev, 'int16')}


def _warp(dev, steps, delays, shift=None):
    from hftt_hip import ops
    return ops.Warp(torch.tensor(steps, dtype=torch.int32, device=dev), torch.tensor(delays, dtype=torch.int64, device=dev),
                    None if shift is None else torch.tensor(shift, dtype=torch.int32, device=dev))


def _clip(lm, table, windows, width, gain=None, noise_std=None, seed=0, warp=None, mix=None, mix_warp=None):
    """the four entry points through the C ABI with `out` inside a NaN arena -> [B, n_mels, width] on the host.  windows: [(file, first frame)];
    mix: [(file, first frame, gain)] or None; warp / mix_warp: ops.Warp or None (with a mix both or neither)"""
    from hftt_hip import _capi
    dev = table.device
    B, M_ = len(windows), lm.n_mels
    n = B * M_ * width
    arena = torch.full((n + 2 * GUARD,), float('nan'), device=dev)
    before = _bits(arena).clone()
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    wf, ws = i32([f for f, _ in windows]), i32([s for _, s in windows])
    g = None if gain is None else torch.tensor(gain, dtype=torch.float32, device=dev)
    ns = None if noise_std is None else torch.tensor(noise_std, dtype=torch.float32, device=dev)
    cls = {(False, False): _capi.ClipLogmelDesc, (True, False): _capi.ClipLogmelWarpDesc, (False, True): _capi.ClipLogmelMixDesc,
           (True, True): _capi.ClipLogmelMixWarpDesc}[(warp is not None, mix is not None)]
    w = cls()
    d = w if cls is _capi.ClipLogmelDesc else w.base
    d.wave, d.file_samp0, d.win_file, d.win_start = table.wave.data_ptr(), table.file_samp0.data_ptr(), wf.data_ptr(), ws.data_ptr()
    d.total_samples, d.wave_i16, d.n_files, d.B, d.width = table.total_samples, int(table.dtype == 'int16'), table.n_files, B, width
    d.n_fft, d.hop, d.n_mels, d.log_offset = lm.n_fft, lm.hop, M_, lm.log_offset
    d.window, d.twiddle = lm.window.data_ptr(), lm.twiddle.data_ptr()
    d.fb_start, d.fb_len, d.fb_off, d.fb_w = lm.fb_start.data_ptr(), lm.fb_len.data_ptr(), lm.fb_off.data_ptr(), lm.fb_w.data_ptr()
    d.fill, d.seed = FILL, seed
    d.gain, d.noise_std = (None if g is None else g.data_ptr()), (None if ns is None else ns.data_ptr())
    d.out = arena[GUARD:].data_ptr()
    keep = []
    if warp is not None:
        w.warp, k = warp._args('clip_logmel', B, dev)
        keep.append(k)
    if mix is not None:
        mf, ms = i32([m[0] for m in mix]), i32([m[1] for m in mix])
        mg = torch.tensor([m[2] for m in mix], dtype=torch.float32, device=dev)
        w.mix.mix_file, w.mix.mix_start, w.mix.mix_gain = mf.data_ptr(), ms.data_ptr(), mg.data_ptr()
        if warp is not None:
            w.mix_warp, k = mix_warp._args('clip_logmel', B, dev)
            keep.append(k)
    name = 'hftt_clip_logmel' + ('_mix' if mix is not None else '') + ('_warp' if warp is not None else '')
    _capi.check(getattr(_capi.lib(), name)(C.byref(w), torch.cuda.current_stream(dev).cuda_stream), name)
    torch.cuda.synchronize(dev)
    after = _bits(arena)
    assert torch.equal(after[:GUARD], before[:GUARD]) and torch.equal(after[GUARD + n:], before[GUARD + n:]), 'the arena around the output was written'
    out = arena[GUARD:GUARD + n].cpu()
    assert not bool(torch.isnan(out).any()), 'an element of the footprint was not written'
    return out.view(B, M_, width)


# (primary file, first frame), (partner file, first frame): file 0 empty, 1 one sample, 2 255 samples, 3 2304 (10 frames), 4 4219 (17 frames)
CASES = [((4, -2), (3, 3)),        # the partner starts later in its file
         ((4, 5), (3, -4)),        # ... earlier: its first samples fall in the middle of the window
         ((4, 0), (2, 0)),         # a partner that ends inside the window
         ((3, 1), (0, 0)),         # an empty partner: + 0 * gain
         ((4, 2), (4, 7)),         # the primary's own file at another start
         ((3, 0), (5, 0)),         # index out of range: no partner
         ((3, 0), (-3, 2)),        # ... negative
         ((2, -1), (4, 3)),        # a long partner on a short primary: added onto the primary's extent only
         ((1, 0), (3, 2)),         # ... on a one-sample primary
         ((0, 0), (4, 0))]         # ... on an empty primary: one frame of exact zeros
GAIN = (0.5, 1.75, 1.0, 0.25, 3.0, 0.7, 1.3, 2.0, 0.9, 1.1)
MIX_GAIN = (0.8, 0.25, 1.0, 0.5, 0.33, 0.6, 0.6, 1.5, 0.75, 0.4)
NOISE_STD = (1e-2, 1e-3, 0.0, 1e-4, 3e-2, 1e-3, 1e-3, 1e-2, 1e-3, 1e-2)


def _one_file_table(dev, f, samples):
    """a float32 WaveTable whose file f holds `samples` (the other files empty: the noise key keeps its file index)"""
    from hftt_hip import ops
    files = [torch.zeros(0)] * len(LENS)
    files[f] = torch.as_tensor(samples, dtype=torch.float32)
    return ops.WaveTable(files, dev, 'float32')


def _premix(a, g, b, gb):
    """fl(fl(a g) + fl(b gb)), one fp32 rounding per operation; g None: no product; b None: no partner, no sum"""
    s = a.astype(np.float32)
    if g is not None:
        s = s * np.float32(g)
    if b is not None:
        s = s + b.astype(np.float32) * np.float32(gb)
    return s.astype(np.float32)


def _at(x, first, n):
    """x[first : first + n] with zeros outside x"""
    out = np.zeros(n, np.float32)
    i = first + np.arange(n, dtype=np.int64)
    v = (i >= 0) & (i < len(x))
    out[v] = x[i[v]]
    return out


@pytest.mark.parametrize('i16', [False, True], ids=['fp32', 'int16'])
@pytest.mark.parametrize('width', [1, 21])
def test_no_partner_is_the_unmixed_kernel_to_the_bit(dev, lm, corpus, width, i16):
    wins = [c[0] for c in CASES]
    B = len(wins)
    none = [(-1, 5, 0.5)] * B
    kw = dict(gain=GAIN, noise_std=NOISE_STD, seed=SEED)
    assert torch.equal(_bits(_clip(lm, corpus[i16], wins, width, mix=none, **kw)), _bits(_clip(lm, corpus[i16], wins, width, **kw)))
    assert torch.equal(_bits(_clip(lm, corpus[i16], wins, width, mix=none)), _bits(_clip(lm, corpus[i16], wins, width)))
    steps = [W.step_of(1.0), W.step_of(-1.7), 1 << 23, 1 << 25, W.ONE] * 2
    delays = [0, int(0.37 * W.ONE), (HOP - 1) << 24, 7, 2 * HOP << 24] * 2
    warp = _warp(dev, steps, delays)
    got = _clip(lm, corpus[i16], wins, width, warp=warp, mix=none, mix_warp=_warp(dev, steps[::-1], delays[::-1]), **kw)
    assert torch.equal(_bits(got), _bits(_clip(lm, corpus[i16], wins, width, warp=warp, **kw)))


@pytest.mark.parametrize('i16', [False, True], ids=['fp32', 'int16'])
@pytest.mark.parametrize('width', [1, 21])
def test_partners_are_the_plain_kernel_on_the_premixed_file_to_the_bit(dev, lm, corpus, width, i16):
    from hftt_hip import ops
    wins = [c[0] for c in CASES]
    mix = [(c[1][0], c[1][1], gb) for c, gb in zip(CASES, MIX_GAIN)]
    host = _host(i16)
    plain = _clip(lm, corpus[i16], wins, width, gain=GAIN)
    for name, kw in (('gain', dict(gain=GAIN)), ('gain+noise', dict(gain=GAIN, noise_std=NOISE_STD, seed=SEED)), ('noise', dict(noise_std=NOISE_STD, seed=SEED))):
        got = _clip(lm, corpus[i16], wins, width, mix=mix, **kw)
        for b, ((f, s), (fb, sb, gb)) in enumerate(zip(wins, mix)):
            a = host[f]
            part = _at(host[fb], (sb - s) * HOP, len(a)) if 0 <= fb < len(LENS) else None
            pre = _premix(a, GAIN[b] if 'gain' in kw else None, part, gb)
            rkw = {'noise_std': [NOISE_STD[b]], 'seed': SEED} if 'noise_std' in kw else {}
            ref = _clip(lm, _one_file_table(dev, f, pre), [(f, s)], width, **rkw)
            assert torch.equal(_bits(ref[0]), _bits(got[b])), (width, name, b)
        if name == 'gain':          # the partner is audible where it should be, and only there
            differs = [not torch.equal(_bits(got[b]), _bits(plain[b])) for b in range(len(wins))]
            if width == 21:
                assert differs == [True, True, True, False, True, False, False, True, True, False], differs
    out = ops.clip_logmel(corpus[i16], lm, [f for f, _ in wins], [s for _, s in wins], width, FILL, gain=GAIN, noise_std=NOISE_STD, seed=SEED,
                          mix=ops.Mix(torch.tensor([m[0] for m in mix], device=dev), torch.tensor([m[1] for m in mix], device=dev),
                                      torch.tensor([m[2] for m in mix], device=dev)))          # the wrapper: the same launch
    assert torch.equal(_bits(out.cpu()), _bits(_clip(lm, corpus[i16], wins, width, mix=mix, gain=GAIN, noise_std=NOISE_STD, seed=SEED)))


@pytest.mark.parametrize('i16', [False, True], ids=['fp32', 'int16'])
def test_warped_partners_are_the_plain_kernel_on_the_premix_of_the_warped_files(dev, lm, corpus, i16):
    """both sources through hftt_wave_warp, premixed on the host: windows counted in the primary's WARPED file, the partner read at the
    primary's warped position moved by the frame difference; an identity warp on one side keeps that side's samples exact"""
    from hftt_hip import ops
    width = 21
    wins = [c[0] for c in CASES]
    mix = [(c[1][0], c[1][1], gb) for c, gb in zip(CASES, MIX_GAIN)]
    B = len(wins)
    steps = [W.step_of(1.0), W.step_of(-1.7), W.ONE, 1 << 25, W.step_of(0.3), W.ONE, 1 << 23, W.step_of(2.0), W.ONE, W.step_of(-0.4)]
    delays = [0, int(0.37 * W.ONE), 0, 7, (HOP - 1) << 24, 0, 100 << 24, 0, 3 << 24, 0]
    steps_b = [W.step_of(-2.0), W.ONE, W.step_of(0.7), W.step_of(1.0), W.step_of(-0.3), W.ONE, W.ONE, (1 << 25) + 1, 1 << 25, W.ONE]
    delays_b = [int(0.5 * W.ONE), 2 * HOP << 24, 0, 0, 9 << 24, 0, 0, 5 << 24, 0, 0]                   # (partner 7's step is out of range: no partner)
    wa, wb = _warp(dev, steps, delays), _warp(dev, steps_b, delays_b)
    table = corpus[i16]
    for name, kw in (('gain', dict(gain=GAIN)), ('gain+noise', dict(gain=GAIN, noise_std=NOISE_STD, seed=SEED))):
        got = _clip(lm, table, wins, width, warp=wa, mix=mix, mix_warp=wb, **kw)
        for b, ((f, s), (fb, sb, gb)) in enumerate(zip(wins, mix)):
            one = lambda w, k: _warp(dev, [w.step_q24[k].item()], [w.delay_q24[k].item()])
            na = W.warp_len(LENS[f], steps[b], delays[b])
            if na == 0:
                a = np.zeros(0, np.float32)
            else:
                a = ops.wave_warp(table, [f], [0], na, one(wa, b))[0].cpu().numpy()
            part = None
            if 0 <= fb < len(LENS) and (1 << 23) <= steps_b[b] <= (1 << 25):
                part = ops.wave_warp(table, [fb], [(sb - s) * HOP], na, one(wb, b))[0].cpu().numpy() if na else np.zeros(0, np.float32)
            pre = _premix(a, GAIN[b], part, gb)
            rkw = {'noise_std': [NOISE_STD[b]], 'seed': SEED} if 'noise_std' in kw else {}
            ref = _clip(lm, _one_file_table(dev, f, pre), [(f, s)], width, **rkw)
            assert torch.equal(_bits(ref[0]), _bits(got[b])), (name, b)
    # one side warped only, through the wrapper: the missing side runs under the identity
    m = lambda w: ops.Mix(torch.tensor([x[0] for x in mix], device=dev), torch.tensor([x[1] for x in mix], device=dev), torch.tensor([x[2] for x in mix], device=dev), warp=w)
    ident = _warp(dev, [W.ONE] * B, [0] * B)
    args = (table, lm, [f for f, _ in wins], [s for _, s in wins], width, FILL)
    assert torch.equal(_bits(ops.clip_logmel(*args, gain=GAIN, warp=wa, mix=m(None))), _bits(ops.clip_logmel(*args, gain=GAIN, warp=wa, mix=m(ident))))
    assert torch.equal(_bits(ops.clip_logmel(*args, gain=GAIN, mix=m(wb))), _bits(ops.clip_logmel(*args, gain=GAIN, warp=ident, mix=m(wb))))
    # ... and with the identity on both sides the warped form is the unwarped one
    assert torch.equal(_bits(ops.clip_logmel(*args, gain=GAIN, warp=ident, mix=m(ident))), _bits(ops.clip_logmel(*args, gain=GAIN, mix=m(None))))


# ------------------------------------------------------------------------------------------------
def _note(pitch, onset, offset, velocity=64):
    return {'pitch': pitch, 'onset': onset, 'offset': offset, 'velocity': velocity}


def _cfg(N):
    return {'feature': {'sr': 16000, 'hop_sample': 256}, 'midi': {'note_min': 21, 'num_note': N}}


@functools.lru_cache(maxsize=None)
def _label_files(N):
    """file 0: notes over every pitch, with a repeated note (no offset target) and overlapping onsets; file 1: 300 notes on ONE pitch (two filter
    passes of 256) and a few elsewhere; file 2: no notes; file 3: a short file.  Decimal times a microsecond apart: no accidental ties."""
    r = np.random.RandomState(11 + N)
    top = 21 + N - 1
    f0 = [_note(22, 0.100001, 0.400002, 70), _note(22, 0.400002, 0.650003, 50), _note(top, 0.020004, 0.300005, 90), _note(22, 0.640011, 0.700012, 20)]
    f0 += [_note(int(r.randint(21, top + 1)), round(float(t), 6) + 1e-6 * i, round(float(t + d), 6) + 1e-6 * i + 3e-7, int(v))
           for i, (t, d, v) in enumerate(zip(r.uniform(0.0, 5.0, 40), r.uniform(0.02, 0.6, 40), r.randint(1, 128, 40)))]
    f1 = [_note(23, 0.013 * i + 1e-6 * i, 0.013 * i + 0.03 + 1e-6 * i + 2e-7, 1 + i % 127) for i in range(300)]
    f1 += [_note(top, 0.5, 4.9, 99), _note(21, 1.000004, 1.200005, 5)]
    f3 = [_note(22, 0.050007, 0.400008, 80), _note(top, 0.200009, 0.900011, 70)]
    return f0, f1, [], f3


# (primary file, start, partner file, partner start, a_frames): None = the window's length (the audio covers it)
LABEL_WINDOWS = [(0, -3, 1, 5, None), (0, 10, 1, -7, None), (0, 0, 1, 100000, None), (2, 0, 1, 0, None), (3, 0, -1, 0, None), (0, 0, 0, 9, None),
                 (3, 2, 1, 0, 10), (2, -4, 3, 0, None), (1, 250, 0, -250, None), (0, 4, 7, 0, None), (3, 0, 1, 3, 0)]
#   shift, step, delay per window for either source (None: that source has no map)
MAP_A = [(0, W.step_of(0.3), 0), (1, W.step_of(1.0), 5 << 24), (0, W.ONE, 0), (0, W.step_of(-0.2), 0), (-1, W.step_of(-1.0), 0), (0, W.ONE, 100 << 24),
         (1, W.step_of(1.2), 0), (0, W.ONE, 0), (0, W.step_of(0.4), 77), (0, W.ONE, 0), (0, W.ONE, 0)]
MAP_B = [(1, W.step_of(1.0), 0), (0, W.step_of(-0.3), 3 << 24), (0, W.ONE, 0), (-1, W.step_of(-0.8), 255 << 24), (0, W.ONE, 0), (1, W.step_of(0.9), 0),
         (0, W.ONE, 0), (0, W.step_of(0.2), 0), (-1, W.step_of(-1.1), 0), (0, W.ONE, 0), (0, W.step_of(0.1), 0)]


def _src(notes, start, m):
    if m is None:
        return {'notes': notes, 'start': start}
    return {'notes': notes, 'start': start, 'shift': m[0], 't_delay': W.t_delay_of(m[2], 16000), 't_scale': W.t_scale_of(m[1])}


@functools.lru_cache(maxsize=None)
def _label_reference(N, length, dt, maps):
    """the walker's tracks of every window, computed once per case: [(onset, offset, mpe, velocity)] * B"""
    files = _label_files(N)
    out = []
    for b, (fa, sa, fb, sb, af) in enumerate(LABEL_WINDOWS):
        A = _src(files[fa], sa, MAP_A[b] if maps[0] else None)
        B_ = _src(files[fb], sb, MAP_B[b] if maps[1] else None) if 0 <= fb < len(files) else None
        out.append(M.mix_labels(_cfg(N), A, B_, length, a_frames=max(0, sa + length) + 5 if af is None else af, duration_tolerance=dt))
    return out


@pytest.mark.parametrize('maps', [(False, False), (True, True), (False, True), (True, False)], ids=['plain', 'both-warped', 'partner-warped', 'primary-warped'])
@pytest.mark.parametrize('length', [1, 21, 300])
@pytest.mark.parametrize('N', [6, 88])
def test_labels_are_the_walker(dev, N, length, maps):
    from hftt_hip import ops
    files = _label_files(N)
    table = ops.labels_table(list(files), _cfg(N), dev)
    B = len(LABEL_WINDOWS)
    mk = lambda ms: _warp(dev, [m[1] for m in ms], [m[2] for m in ms], [m[0] for m in ms])
    wa, wb = (mk(MAP_A) if maps[0] else None), (mk(MAP_B) if maps[1] else None)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    af = torch.tensor([max(0, w[1] + length) + 5 if w[4] is None else w[4] for w in LABEL_WINDOWS], dtype=torch.int64, device=dev)
    mix = ops.Mix(i32([w[2] for w in LABEL_WINDOWS]), i32([w[3] for w in LABEL_WINDOWS]), torch.ones(B, device=dev), warp=wb)
    wf, ws = [w[0] for w in LABEL_WINDOWS], [w[1] for w in LABEL_WINDOWS]
    partner_cells = 0
    for dt in (False, True):
        want = _label_reference(N, length, dt, maps)
        for form in ('train', 'store'):
            got = ops.labels_render(table, wf, ws, length, form=form, duration_tolerance=dt, warp=wa, mix=mix, a_frames=af)
            torch.cuda.synchronize(dev)
            for b in range(B):
                for name, g, e in zip(('onset', 'offset', 'mpe', 'velocity'), got, want[b]):
                    g = g[b].cpu().numpy()
                    if form == 'train':
                        assert g.dtype == (np.int64 if name == 'velocity' else np.float32)
                        e = e.astype(g.dtype)
                    else:
                        assert g.dtype == e.dtype, (name, g.dtype, e.dtype)
                    assert np.array_equal(g.view(np.uint8), np.ascontiguousarray(e).view(np.uint8)), (N, length, maps, dt, form, b, name, int((g != e).sum()))
            # no partner: the un-mixed entry points to the bit, whatever a_frames says
            none = ops.Mix(i32([-1] * B), i32([w[3] for w in LABEL_WINDOWS]), torch.ones(B, device=dev), warp=wb)
            alone = ops.labels_render(table, wf, ws, length, form=form, duration_tolerance=dt, warp=wa)
            for x, y in zip(ops.labels_render(table, wf, ws, length, form=form, duration_tolerance=dt, warp=wa, mix=none, a_frames=af), alone):
                assert torch.equal(x, y)
            partner_cells += sum(int((g != a).sum()) for g, a in zip(got, alone))
    assert partner_cells > 0 or length == 1


def test_the_label_cases_hold_what_they_claim():
    """(host only) the 300-note pitch needs two filter passes; the silent primary shows its partner; the window behind the partner's end and the
    a_frames = 0 window show the primary alone; a_frames = 10 cuts the partner off at the primary's frame 10"""
    N, L = 88, 300
    files = _label_files(N)
    assert sum(n['pitch'] == 23 for n in files[1]) == 300 > 256 and not files[2]
    ref = _label_reference(N, L, False, (False, False))
    alone = lambda b: M.mix_labels(_cfg(N), {'notes': files[LABEL_WINDOWS[b][0]], 'start': LABEL_WINDOWS[b][1]}, None, L)
    assert ref[3][0].any() and not alone(3)[0].any()
    for b in (2, 4, 9, 10):
        assert all(np.array_equal(x, y) for x, y in zip(ref[b], alone(b)))
    b = 6
    full = M.mix_labels(_cfg(N), {'notes': files[3], 'start': 2}, {'notes': files[1], 'start': 0}, L, a_frames=L + 5)
    assert all(np.array_equal(x[:8], y[:8]) for x, y in zip(ref[b], full)) and not np.array_equal(ref[b][0][8:], full[0][8:])
    assert all(np.array_equal(x[8:], y[8:]) for x, y in zip(ref[b], alone(b)))


# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mini():
    """(config, note lists, store) at the tiny test model's sizes: three short plucked files"""
    from corpus import synth_audio as SA
    from corpus.make_dataset import assemble_wave_store
    c = util.MINI
    config = {'feature': {'mel_bins': c.n_bin, 'n_bins': c.n_bin, 'fft_bins': 2048, 'window_length': 2048, 'log_offset': 1e-8, 'sr': 16000, 'hop_sample': 256},
              'input': {'margin_b': c.n_margin, 'margin_f': c.n_margin, 'num_frame': c.n_frame, 'min_value': -18.420681, 'max_value': 0.0},
              'midi': {'note_min': 21, 'num_note': c.n_note, 'num_velocity': c.n_velocity}}
    notes = [[_note(21 + (3 * i) % c.n_note, 0.050001 + 0.06 * i, 0.200002 + 0.06 * i, 1 + i % (c.n_velocity - 1)) for i in range(10)],
             [_note(22 + (i % 2), 0.100003 + 0.11 * i, 0.250004 + 0.11 * i, 2 + i) for i in range(4)], [_note(23, 0.300005, 0.450006, 3)]]
    waves = [SA.pluck_wave(a, dur=d).numpy() for a, d in zip(notes, (0.9, 0.7, 0.6))]
    return config, notes, assemble_wave_store(waves, notes, config)


def _same(a, b):
    return all(torch.equal(_bits(x) if x.dtype == torch.float32 else x, _bits(y) if y.dtype == torch.float32 else y) for x, y in zip(a, b))


def test_mix_p_zero_is_the_unmixed_store_batch_for_batch(dev):
    from training.dataset import WaveAugment, WaveClipStore
    config, _, store = _mini()
    kw = dict(gain_db=(-6.0, 6.0), noise_dbfs=(-60.0, -40.0), pitch_semitones=(-1, 1), detune_cents=20, shift=True, seed=3)
    old, new = WaveClipStore(store, config, dev, augment=WaveAugment(**kw)), WaveClipStore(store, config, dev, augment=WaveAugment(mix_p=0.0, **kw))
    mixed = WaveClipStore(store, config, dev, augment=WaveAugment(mix_p=1.0, **kw))
    ids = list(range(0, len(old), max(1, len(old) // 6)))[:6]
    for k in range(3):
        a, b, c = old.batch(ids), new.batch(ids), mixed.batch(ids)
        assert _same(a, b), k
        if k == 0:                  # the first batch's gain, noise and primary warp are drawn before the first mix draw
            assert not _same(a, c) and all(bool(torch.isfinite(t.float()).all()) for t in c)
    assert _same(WaveClipStore(store, config, dev).batch(ids), WaveClipStore(store, config, dev, augment=WaveAugment(mix_p=0.0)).batch(ids))


@pytest.mark.parametrize('warps', [False, True], ids=['plain', 'warped'])
def test_store_labels_are_the_walker_fed_the_drawn_partners(dev, warps):
    """a second store with the same seed replays the draws in batch()'s order; the walker renders every clip from the note lists"""
    from hftt_hip import ops
    from training.dataset import WaveAugment, WaveClipStore
    config, notes, store = _mini()
    kw = dict(seed=8, mix_p=0.7, mix_gain_db=(-9.0, -1.0), **(dict(pitch_semitones=(-1, 1), detune_cents=15, shift=True) if warps else {}))
    s, shadow = WaveClipStore(store, config, dev, augment=WaveAugment(**kw)), WaveClipStore(store, config, dev, augment=WaveAugment(**kw))
    T, n_clips = config['input']['num_frame'], len(s)
    seen_on = seen_off = 0
    for ids in (list(range(0, n_clips, max(1, n_clips // 8)))[:8], list(range(n_clips - 1, -1, -max(1, n_clips // 5)))[:5]):
        got = s.batch(ids)
        B = len(ids)
        file, frame = shadow.clip_file[ids], shadow.clip_frame[ids]
        shadow.augment.draw(B)
        wa = wb = None
        if warps:
            wa = shadow._draw_warp(file)
            frame = shadow._warped_frame(frame, wa)
        on, partner, gain = shadow.augment.draw_mix(B, n_clips)
        pfile, pframe = shadow.clip_file[partner], shadow.clip_frame[partner]
        if warps:
            wb = shadow._draw_warp(pfile)
            pframe = shadow._warped_frame(pframe, wb)
        af = ops.audio_frames(shadow.waves, HOP, file, wa).tolist()
        nsamp = shadow.waves.file_nsamp_host
        m = lambda w, b: None if w is None else (int(w.shift[b]), int(w.step_q24[b]), int(w.delay_q24[b]))
        for b in range(B):
            fa, fb = int(file[b]), int(pfile[b])
            assert af[b] == 1 + (W.warp_len(int(nsamp[fa]), int(wa.step_q24[b]), int(wa.delay_q24[b])) if warps else int(nsamp[fa])) // HOP
            B_ = _src(notes[fb], int(pframe[b]), m(wb, b)) if bool(on[b]) else None
            want = M.mix_labels(config, _src(notes[fa], int(frame[b]), m(wa, b)), B_, T, a_frames=af[b])
            for name, g, e in zip(('onset', 'offset', 'mpe', 'velocity'), got[1:], want):
                assert np.array_equal(g[b].cpu().numpy(), e.astype(g[b].cpu().numpy().dtype)), (ids[b], name)
        seen_on += int(on.sum()); seen_off += int((~on).sum())
    assert seen_on > 0 and seen_off > 0


def test_three_training_steps_on_mixed_batches(dev):
    from hftt_hip.trainer import TrainStep
    from training.dataset import WaveAugment, WaveClipStore
    c = util.MINI
    config, _, store = _mini()
    s = WaveClipStore(store, config, dev, augment=WaveAugment(gain_db=(-3.0, 3.0), noise_dbfs=(-60.0, -50.0), pitch_semitones=(-1, 1), shift=True, mix_p=1.0, seed=1))
    model = util.build_model(c, 5).to(dev)
    model.hftt_precision = 'x3'
    model.train()
    step = TrainStep(model, lr=1e-4)
    losses = []
    for i, batch in enumerate(s.loader(2, shuffle=True, seed=2)):
        if i == 3:
            break
        assert batch[0].shape == (2, c.n_bin, c.n_frame + 2 * c.n_margin)
        losses.append(step(batch[0], *batch[1:]).clone())
    assert len(losses) == 3 and all(bool(torch.isfinite(l).all()) for l in losses)
