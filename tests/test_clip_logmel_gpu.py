"""hftt_clip_logmel (csrc/clip_logmel.hip) on the device, under the per-cell criterion of tests/clip_logmel_emul.py (what it resolves:
tests/test_clip_logmel_emul_bound.py, on the CPU, on the same scenes).

The corpus is eight signals of frontend_emul.logmel_signal back to back (1 .. 4219 samples; a full-scale constant directly in front of a silent
file), the requests B = 5 windows of width 1, 21 and 192: negative starts, windows across a file's last frame, wholly before and behind a file,
overlapping windows of one file, window order against file order.  The output lies inside an arena of NaN that must come back untouched around
a footprint written in every element.  Valid cells: within the bound hftt_logmel carries around the fp64 reference; fill cells: the fill's
bits.  int16 input, gain and gain + noise are bit-equal to runs on the waveform converted / multiplied / mixed beforehand.  Against hftt_logmel
of each whole file: within the sum of the two bounds, and equal to the bit: the two kernels call one frame transform (csrc/logmel_frame.h).
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import frontend_emul as FE
import clip_logmel_emul as CE

pytestmark = pytest.mark.gpu
GUARD = 7          # arena elements in front of and behind the output (odd: the output is not 16-byte aligned)


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _tables():
    return FE.logmel_tables()


@functools.lru_cache(maxsize=None)
def _quantized():
    return tuple(CE.quantize_i16(w) for w in CE.scene_waves())


@functools.lru_cache(maxsize=None)
def _expect(width, k, i16=False):
    return CE.clip_logmel_expect(_quantized() if i16 else CE.scene_waves(), _tables(), CE.SCENES[width][k], width, wave_i16=i16)


@pytest.fixture(scope='module')
def lm(dev):
    from hftt_hip import ops
    return ops.LogMel(dev)


@pytest.fixture(scope='module')
def corpus(dev):
    """the scene's files as an fp32 table, an int16 table, and an fp32 table of the dequantised int16 values"""
    from hftt_hip import ops
    q = _quantized()
    return {'f32': ops.WaveTable(CE.scene_waves(), dev, 'float32'), 'i16': ops.WaveTable(q, dev, 'int16'),
            'deq': ops.WaveTable([CE.dequantize(w) for w in q], dev, 'float32')}


def _run(lm, table, windows, width, gain=None, noise_std=None, seed=0, fill=CE.FILL):
    """hftt_clip_logmel through the C ABI with `out` inside a NaN arena; asserts the arena around the footprint untouched and the footprint
    written in every element; returns out [B, n_mels, width] on the host"""
    from hftt_hip import _capi
    dev = table.device
    B, M = len(windows), lm.n_mels
    n = B * M * width
    arena = torch.full((n + 2 * GUARD,), float('nan'), device=dev)
    before = _bits(arena).clone()
    wf = torch.tensor([f for f, _ in windows], dtype=torch.int32, device=dev)
    ws = torch.tensor([s for _, s in windows], dtype=torch.int32, device=dev)
    g = None if gain is None else torch.tensor(gain, dtype=torch.float32, device=dev)
    ns = None if noise_std is None else torch.tensor(noise_std, dtype=torch.float32, device=dev)
    d = _capi.ClipLogmelDesc()
    d.wave, d.file_samp0, d.win_file, d.win_start = table.wave.data_ptr(), table.file_samp0.data_ptr(), wf.data_ptr(), ws.data_ptr()
    d.total_samples, d.wave_i16, d.n_files, d.B, d.width = table.total_samples, int(table.dtype == 'int16'), table.n_files, B, width
    d.n_fft, d.hop, d.n_mels, d.log_offset = lm.n_fft, lm.hop, M, lm.log_offset
    d.window, d.twiddle = lm.window.data_ptr(), lm.twiddle.data_ptr()
    d.fb_start, d.fb_len, d.fb_off, d.fb_w = lm.fb_start.data_ptr(), lm.fb_len.data_ptr(), lm.fb_off.data_ptr(), lm.fb_w.data_ptr()
    d.fill, d.seed = fill, seed
    d.gain, d.noise_std = (None if g is None else g.data_ptr()), (None if ns is None else ns.data_ptr())
    d.out = arena[GUARD:].data_ptr()
    _capi.check(_capi.lib().hftt_clip_logmel(C.byref(d), torch.cuda.current_stream(dev).cuda_stream), 'clip_logmel')
    torch.cuda.synchronize(dev)
    after = _bits(arena)
    assert torch.equal(after[:GUARD], before[:GUARD]) and torch.equal(after[GUARD + n:], before[GUARD + n:]), 'the arena around the output was written'
    out = arena[GUARD:GUARD + n].view(B, M, width).cpu()
    assert not bool(torch.isnan(out).any()), 'an element of the footprint was not written'
    return out


@pytest.mark.parametrize('i16', [False, True], ids=['fp32', 'int16'])
@pytest.mark.parametrize('width', CE.WIDTHS)
def test_against_fp64_and_the_fill(lm, corpus, width, i16):
    floor = torch.log(torch.tensor(FE.f32(FE.LOG_OFFSET), dtype=torch.float32))
    worst = 0.0
    for k, wins in enumerate(CE.SCENES[width]):
        exp = _expect(width, k, i16)
        got = _run(lm, corpus['i16' if i16 else 'f32'], wins, width)
        bad = CE.clip_logmel_check(got, exp, CE.FILL)
        worst = max(worst, CE.clip_logmel_ratio(got, exp))
        assert not bad, (width, k, bad)
        for b, (f, _) in enumerate(wins):                # a window over the silent file: the floor, to the bit, in every valid frame
            if f == CE.SILENT:
                assert bool((got[b][:, exp['valid'][b]] == floor).all()), (width, k, b, 'the neighbouring file bleeds into the silent one')
        # the wrapper: the same launch, its own allocation
        from hftt_hip import ops
        out = ops.clip_logmel(corpus['i16' if i16 else 'f32'], lm, [f for f, _ in wins], [s for _, s in wins], width, CE.FILL)
        assert torch.equal(_bits(out.cpu()), _bits(got)), (width, k)
    print('clip_logmel width %d %s: worst error / bound %.3f' % (width, 'int16' if i16 else 'fp32', worst))


@pytest.mark.parametrize('width', CE.WIDTHS)
def test_int16_gain_and_noise_are_the_premixed_waveform_to_the_bit(dev, lm, corpus, width):
    from hftt_hip import ops
    for k, wins in enumerate(CE.SCENES[width]):
        assert torch.equal(_bits(_run(lm, corpus['i16'], wins, width)), _bits(_run(lm, corpus['deq'], wins, width))), (width, k, 'int16')
        gained = _run(lm, corpus['f32'], wins, width, gain=CE.GAIN)
        mixed = _run(lm, corpus['f32'], wins, width, gain=CE.GAIN, noise_std=CE.NOISE_STD, seed=CE.SEED)
        for b, (f, s) in enumerate(wins):                # the file of window b multiplied / mixed in fp32 on the host, every other file as it is
            for name, got, std in (('gain', gained, None), ('gain+noise', mixed, CE.NOISE_STD[b])):
                pre = list(CE.scene_waves())
                pre[f] = CE.mix(pre[f], f, CE.GAIN[b], std, CE.SEED)
                ref = _run(lm, ops.WaveTable(pre, dev, 'float32'), [wins[b]], width)
                assert torch.equal(_bits(ref[0]), _bits(got[b])), (width, k, b, name)
        exp = CE.clip_logmel_expect(CE.scene_waves(), _tables(), wins, width, gain=CE.GAIN, noise_std=CE.NOISE_STD, seed=CE.SEED)
        assert not CE.clip_logmel_check(mixed, exp, CE.FILL), (width, k)


def test_overlapping_windows_see_the_same_noise(lm, corpus):
    """two windows of one file under the same gain and noise level: the frames they share are bit-equal (the noise is keyed on the sample)"""
    wins = [(0, 0), (0, 5), (0, -4), (4, 0), (4, 2)]
    got = _run(lm, corpus['f32'], wins, 21, gain=[0.5] * 5, noise_std=[1e-3] * 5, seed=CE.SEED)
    assert torch.equal(_bits(got[0][:, 5:17]), _bits(got[1][:, 0:12])) and torch.equal(_bits(got[0][:, 0:17]), _bits(got[2][:, 4:21]))
    assert torch.equal(_bits(got[3][:, 2:10]), _bits(got[4][:, 0:8]))
    other = _run(lm, corpus['f32'], wins, 21, gain=[0.5] * 5, noise_std=[1e-3] * 5, seed=CE.SEED + 1)
    assert not torch.equal(_bits(other), _bits(got))


def test_against_hftt_logmel_of_each_whole_file(dev, lm, corpus):
    """every frame of every file through both kernels: within the sum of the two kernels' bounds around the fp64 reference (a - b = (a - ref) -
    (b - ref): up + down either way), and no cell differs bitwise: both kernels call the frame transform of csrc/logmel_frame.h."""
    t = _tables()
    differ = cells = 0
    worst = 0.0
    for f, x in enumerate(CE.scene_waves()):
        whole = lm(x.to(dev)).cpu()                      # [frames, n_mels]
        nf = whole.shape[0]
        assert nf == CE.n_frames(len(x))
        r = FE.logmel_ref(x, t)
        up, down = FE.logmel_bound(r)
        wins = [(f, s) for s in (0, -3, nf - 21, 4, -20)]
        got = _run(lm, corpus['f32'], wins, 21)
        for b, (_, s) in enumerate(wins):
            fr = s + torch.arange(21)
            v = (fr >= 0) & (fr < nf)
            a, w = got[b][:, v].T, whole[fr[v]]
            assert bool(((a.double() - w.double()).abs() <= (up + down)[fr[v]]).all()), (f, s)
            assert bool((got[b][:, ~v] == torch.tensor(CE.FILL, dtype=torch.float32)).all())
            if bool(v.any()):
                worst = max(worst, float(((a.double() - r['out'][fr[v]]).abs() / torch.where(a.double() >= r['out'][fr[v]], up[fr[v]], down[fr[v]])).max()))
            differ += int((_bits(a) != _bits(w)).sum()); cells += a.numel()
    assert cells > 0
    print('clip_logmel against hftt_logmel: %d of %d cells differ bitwise; worst error / bound against fp64 %.3f' % (differ, cells, worst))
    assert differ == 0


def test_37_mels(dev):
    """n_mels = 37 (no multiple of the 16 rows a store pass covers) with the tables ops.LogMel.tables makes for it"""
    from hftt_hip import ops
    lm37 = ops.LogMel(dev, n_mels=37)
    t = ops.LogMel.tables(16000, FE.N_FFT, 37)
    t.update(hop=FE.HOP, n_fft=FE.N_FFT, n_mels=37, log_offset=FE.f32(FE.LOG_OFFSET))
    table = ops.WaveTable(CE.scene_waves(), dev, 'float32')
    for width in (21, 192):
        wins = CE.SCENES[width][0]
        got = _run(lm37, table, wins, width)
        assert got.shape == (5, 37, width)
        exp = CE.clip_logmel_expect(CE.scene_waves(), t, wins, width)
        assert not CE.clip_logmel_check(got, exp, CE.FILL), width
        print('clip_logmel 37 mels width %d: worst error / bound %.3f' % (width, CE.clip_logmel_ratio(got, exp)))


def test_a_file_index_outside_the_table_is_fill(lm, corpus):
    got = _run(lm, corpus['f32'], [(-1, 0), (8, 0), (0, 0), (1 << 20, 3), (4, 0)], 21)
    fill = torch.tensor(CE.FILL, dtype=torch.float32)
    for b in (0, 1, 3):
        assert bool((got[b] == fill).all()), b
    assert not bool((got[2][:, :17] == fill).any())
