"""The room augmentation on the device: hftt_clip_room, ops.clip_logmel(room=...) and WaveClipStore.batch under WaveAugment's room_p.  What
the pseudo-file tables are worth and what the bound allows is shown on the CPU by tests/test_room_emul_bound.py.

  values   every scratch sample within gamma(taps) sum |h| |dry| + taps 2^-126 of the fp64 convolution of the same fp32 dry samples (the
           worst-case dot-product bound: no margin), L = 1, 5, 300, 2049, 4096, one response shorter than L with garbage behind; a warped
           case against hftt_wave_warp's samples.  Output inside a NaN arena; what lies behind a pseudo-file is not written.
  exact    h = [1] and a dry window are the dry samples; a delta at tap d is the dry path on the file with d zeros in front; all-delta
           responses without noise are today's clip_logmel in all four forms -- bit for bit
  window   the wet samples of one window over all of file 0 are those of the six windows where they overlap, bit for bit, at L = 2049
  end to end   clip_logmel(room=...) is clip_logmel on a table built from the whole-file wet signals, fill columns included; the tables are the emulator's
  store    equal seeds with and without a room: equal labels, equal spectrograms for the clips drawn dry, others differ; reproducible; trains

Largest error / bound seen on an MI355X (float32 / int16 corpus): 0.978 / 0.985 at L = 1 (one product: half an ulp of it is the bound), 0.854 /
0.842 at L = 5, 0.017 / 0.018 at L = 300, 0.0022 / 0.0028 at L = 2049, 0.0014 / 0.0017 at L = 4096, 0.011 warped at L = 300 -- the figures an fp32
numpy convolution gives in the CPU test; see DESIGN.md section 10."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import room_emul as R
import util
import warp_emul as W

pytestmark = pytest.mark.gpu
GUARD = 7
FILES, STARTS = [f for f, _ in R.WINDOWS], [s for _, s in R.WINDOWS]
GAIN = (0.5, 1.75, 1.0, 0.25, 3.0, 0.7)
B = len(R.WINDOWS)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@functools.lru_cache(maxsize=None)
def _host(i16):
    """the files as the kernel reads them, fp32"""
    waves = R.corpus_waves()
    return tuple(R.dequantize(R.quantize_i16(w)) for w in waves) if i16 else tuple(waves)


@pytest.fixture(scope='module')
def lm(dev):
    from hftt_hip import ops
    return ops.LogMel(dev, n_mels=8)


@pytest.fixture(scope='module')
def corpus(dev):
    from hftt_hip import ops
    waves = R.corpus_waves()
    return {False: ops.WaveTable([torch.from_numpy(w) for w in waves], dev, 'float32'),
            True: ops.WaveTable([torch.from_numpy(R.quantize_i16(w)) for w in waves], dev, 'int16')}


def _bank(dev, rows, taps=None):
    from hftt_hip import ops
    return ops.RoomBank(np.stack(rows).astype(np.float32), dev, taps=taps)


def _room(table, bank, index, files=FILES, starts=STARTS, width=R.WIDTH, gain=None, warp=None, n_prime=None):
    """hftt_clip_room through the C ABI with `out` inside a NaN arena -> (the pseudo-files' samples per window, the emulator's tables, which the
    kernel's must equal).  n_prime: the windows' (warped) file lengths when they are not the table's."""
    from hftt_hip import _capi
    dev = table.device
    n = len(files)
    span = R.span_of(width)
    arena = torch.full((n * span + 2 * GUARD,), float('nan'), device=dev)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    wf, ws, ix = i32(files), i32(starts), i32(index)
    samp0 = torch.full((2 * n + 1,), -7, dtype=torch.int64, device=dev)
    ofile, ostart = i32([-7] * n), i32([-7] * n)
    g = None if gain is None else torch.tensor(gain, dtype=torch.float32, device=dev)
    d = _capi.ClipRoomDesc()
    d.wave, d.file_samp0, d.win_file, d.win_start = table.wave.data_ptr(), table.file_samp0.data_ptr(), wf.data_ptr(), ws.data_ptr()
    d.total_samples, d.wave_i16, d.n_files, d.B, d.width = table.total_samples, int(table.dtype == 'int16'), table.n_files, n, width
    d.n_fft, d.hop, d.n_ir, d.L, d.span = R.NFFT, R.HOP, bank.n_ir, bank.L, span
    d.gain = None if g is None else g.data_ptr()
    d.ir, d.ir_taps, d.ir_index = bank.ir.data_ptr(), bank.taps.data_ptr(), ix.data_ptr()
    d.out, d.out_samp0, d.out_win_file, d.out_win_start = arena[GUARD:].data_ptr(), samp0.data_ptr(), ofile.data_ptr(), ostart.data_ptr()
    if warp is not None:
        d.warp, keep = warp._args('clip_room', n, dev)
    _capi.check(_capi.lib().hftt_clip_room(C.byref(d), torch.cuda.current_stream(dev).cuda_stream), 'clip_room')
    torch.cuda.synchronize(dev)
    a = arena.cpu().numpy()
    assert np.isnan(a[:GUARD]).all() and np.isnan(a[GUARD + n * span:]).all(), 'the arena around the scratch was written'
    rows = a[GUARD:GUARD + n * span].reshape(n, span)
    if n_prime is None:
        n_prime = [R.LENS[f] if 0 <= f < len(R.LENS) and r < bank.n_ir else -1 for f, r in zip(files, index)]
    t = R.pseudo_tables(n_prime, starts, width)
    assert np.array_equal(samp0.cpu().numpy(), t['samp0']) and np.array_equal(ofile.cpu().numpy(), t['win_file']) and np.array_equal(ostart.cpu().numpy(), t['win_start'])
    out = []
    for b in range(n):
        m = int(t['e'][b] - t['o'][b])
        assert not np.isnan(rows[b, :m]).any(), 'a sample of pseudo-file %d was not written' % (2 * b)
        assert np.isnan(rows[b, m:]).all(), 'the remainder of row %d was written' % b
        out.append(rows[b, :m].copy())
    return out, t


def _check_values(got, t, dry, rows, taps, index, what):
    """got[b] against the fp64 convolution of dry[b] (the window's whole dry file, fp32) with its response, inside the worst-case bound"""
    worst = 0.0
    for b in range(len(got)):
        if t['win_file'][b] < 0:
            assert len(got[b]) == 0
            continue
        r = index[b]
        ref, mag = R.wet_ref(dry[b], rows[r], taps[r])
        o, e = int(t['o'][b]), int(t['e'][b])
        bound = R.wet_bound(mag[o:e], taps[r])
        err = np.abs(got[b].astype(np.float64) - ref[o:e])
        assert (err <= bound).all(), (what, b, float((err / bound).max()))
        if len(err):
            worst = max(worst, float((err / bound).max()))
    print('%s: largest error / bound %.3g' % (what, worst))
    return worst


@pytest.mark.parametrize('i16', [False, True], ids=['float32', 'int16'])
@pytest.mark.parametrize('L', [1, 5, 300, 2049, 4096])
def test_values_against_fp64(dev, corpus, L, i16):
    r = np.random.RandomState(L)
    short = max(1, L // 2)
    rows = [r.standard_normal(L), r.standard_normal(L)]
    rows[1][short:] = 1e30                                    # garbage behind ir_taps: not read
    rows = [x.astype(np.float32) for x in rows]
    taps = [L, short]
    index = [0, 1, 0, 1, 0, 1]
    got, t = _room(corpus[i16], _bank(dev, rows, taps), index)
    host = _host(i16)
    dry = [host[f] if f >= 0 else None for f in FILES]
    _check_values(got, t, dry, rows, taps, index, 'L = %d, %s' % (L, 'int16' if i16 else 'float32'))


def test_ir_taps_outside_their_range_are_clamped_and_an_index_beyond_the_bank_is_a_window_without_a_file(dev, corpus):
    from hftt_hip import ops
    r = np.random.RandomState(2)
    rows = [r.standard_normal(9).astype(np.float32) for _ in range(3)]
    bank = ops.RoomBank(np.stack(rows), dev)
    bank.taps = torch.tensor([0, 100, -5], dtype=torch.int32, device=dev)          # (RoomBank refuses them: set behind its back)
    index = [0, 1, 2, 3, 2, 7]
    got, t = _room(corpus[False], bank, index)
    assert t['win_file'].tolist() == [0, 2, -1, -1, 8, -1]
    host = _host(False)
    _check_values(got, t, [host[f] if f >= 0 else None for f in FILES], rows, [1, 9, 1], index, 'clamped taps')


def test_values_under_a_warp(dev, corpus):
    """k = +2 semitones and a delay: the dry samples are hftt_wave_warp's, the windows count frames of the warped file"""
    from hftt_hip import ops
    step, delay = W.step_of(2.0), int(100.37 * W.ONE)
    files, starts = [0, 0, 1, 2], [-3, 22, 0, 0]
    n_prime = [W.warp_len(R.LENS[f], step, delay) for f in files]
    assert n_prime[1] // R.HOP + 1 > 22 + 4 > 22 and n_prime[3] == 0
    warp = ops.Warp(torch.tensor([step] * 4, dtype=torch.int32, device=dev), torch.tensor([delay] * 4, dtype=torch.int64, device=dev))
    whole = ops.wave_warp(corpus[True], files, [0] * 4, max(n_prime), warp).cpu().numpy()
    dry = [whole[b, :n_prime[b]] for b in range(4)]
    r = np.random.RandomState(8)
    rows, taps, index = [r.standard_normal(300).astype(np.float32)], [300], [0] * 4
    got, t = _room(corpus[True], _bank(dev, rows), index, files, starts, warp=warp, n_prime=n_prime)
    assert _check_values(got, t, dry, rows, taps, index, 'warped, L = 300') > 0.0


def test_one_tap_and_a_dry_window_are_the_dry_samples(dev, corpus):
    for i16 in (False, True):
        host = _host(i16)
        one, t = _room(corpus[i16], _bank(dev, [np.ones(1)]), [0] * B, gain=GAIN)
        dry, t2 = _room(corpus[i16], _bank(dev, [np.full(5, 3.0)]), [-1] * B, gain=GAIN)
        assert np.array_equal(t['win_file'], t2['win_file'])
        for b, f in enumerate(FILES):
            if t['win_file'][b] < 0:
                continue
            want = (host[f] * np.float32(GAIN[b]))[t['o'][b]:t['e'][b]]
            assert np.array_equal(_bits(one[b]), _bits(want)) and np.array_equal(_bits(dry[b]), _bits(want)), (i16, b)


@pytest.mark.parametrize('d', [7, 300])
def test_a_delta_at_tap_d_is_the_dry_path_on_the_file_with_d_zeros_in_front(dev, corpus, d):
    from hftt_hip import ops
    h = np.zeros(d + 1)
    h[d] = 1.0
    shifted = ops.WaveTable([torch.from_numpy(np.concatenate([np.zeros(d, np.float32), w])[:len(w)]) for w in _host(True)], dev, 'float32')
    wet, t = _room(corpus[True], _bank(dev, [h]), [0] * B, gain=GAIN)
    dry, t2 = _room(shifted, _bank(dev, [h]), [-1] * B, gain=GAIN)
    assert np.array_equal(t['samp0'], t2['samp0'])
    for b in range(B):
        assert np.array_equal(_bits(wet[b]), _bits(dry[b])), b
    assert sum(len(x) for x in wet) > 9000


def test_delta_responses_are_todays_clip_logmel_in_all_four_forms(dev, corpus, lm):
    from hftt_hip import ops
    bank = _bank(dev, [np.eye(1, 5)[0], np.concatenate([[1.0], np.full(4, 1e30)])], taps=[5, 1])
    index = torch.tensor([0, 1, -1, 0, 1, 0], dtype=torch.int32, device=dev)
    step, delay = W.step_of(2.0), int(100.37 * W.ONE)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    warp = ops.Warp(i32([step, W.ONE, step, step, W.ONE, step]), torch.tensor([delay, 0, 0, delay, 3 * W.ONE, 0], dtype=torch.int64, device=dev))
    pwarp = ops.Warp(i32([W.ONE, step, step, W.step_of(-1.0), step, step]), torch.tensor([0, delay, 0, 0, 0, 0], dtype=torch.int64, device=dev))
    gain = torch.tensor(GAIN, device=dev)
    for i16 in (False, True):
        for w, with_mix, mw in ((None, False, None), (warp, False, None), (None, True, None), (warp, True, pwarp)):      # plain, warp, mix, mix + warp
            mix = ops.Mix(i32([1, 0, 0, 0, 1, 2]), i32([0, 3, 1, -2, 0, 0]), torch.tensor([0.5, 0.25, 1.0, 2.0, 0.5, 1.0], device=dev), mw) if with_mix else None
            want = ops.clip_logmel(corpus[i16], lm, FILES, STARTS, R.WIDTH, R.FILL, gain=gain, warp=w, mix=mix)
            got = ops.clip_logmel(corpus[i16], lm, FILES, STARTS, R.WIDTH, R.FILL, gain=gain, warp=w, mix=mix, room=(bank, index))
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (i16, w is not None, with_mix)
            assert bool((want != R.FILL).any())


@functools.lru_cache(maxsize=None)
def _responses(L=2049):
    r = np.random.RandomState(77)
    env = np.exp(-np.arange(L) / 400.0)
    return tuple((r.standard_normal(L) * env).astype(np.float32) for _ in range(2))


@pytest.fixture(scope='module')
def whole(dev, corpus):
    """{int16?: the whole-file wet signals at L = 2049 under GAIN_OF_FILE -- file 0 (response 0) from one window over all of it, file 1 (response
    1) from its window, file 2 empty}: computed once, shared by the two tests below"""
    out = {}
    for i16 in (False, True):
        got, t = _room(corpus[i16], _bank(dev, list(_responses())), [0, 1], [0, 1], [0, 0], width=40, gain=[GAIN_OF_FILE[0], GAIN_OF_FILE[1]])
        assert t['o'].tolist() == [0, 0] and t['e'].tolist() == [R.LENS[0], R.LENS[1]]
        out[i16] = (got[0], got[1], np.zeros(0, np.float32))
    return out


GAIN_OF_FILE = (0.5, 1.75, 3.0)
INDEX_OF_FILE = (0, 1, 0)


@pytest.mark.parametrize('i16', [False, True], ids=['float32', 'int16'])
def test_the_wet_samples_do_not_depend_on_the_window(dev, corpus, whole, i16):
    """L = 2049: tap groups, tile borders (2,048 outputs) and the windows' different first samples all fall inside the compared spans"""
    gain = [GAIN_OF_FILE[f] if f >= 0 else 1.0 for f in FILES]
    index = [INDEX_OF_FILE[f] if f >= 0 else 0 for f in FILES]
    got, t = _room(corpus[i16], _bank(dev, list(_responses())), index, gain=gain)
    seen = 0
    for b, f in enumerate(FILES):
        if t['win_file'][b] < 0:
            continue
        assert np.array_equal(_bits(got[b]), _bits(whole[i16][f][t['o'][b]:t['e'][b]])), b
        seen += len(got[b])
    assert seen == (19 * 256 + 1024 - 3 * 256) + (9000 - 21 * 256) + 700


@pytest.mark.parametrize('i16', [False, True], ids=['float32', 'int16'])
def test_end_to_end_is_clip_logmel_on_the_wet_files(dev, corpus, whole, lm, i16):
    from hftt_hip import ops
    wet_table = ops.WaveTable([torch.from_numpy(w) for w in whole[i16]], dev, 'float32')
    gain = torch.tensor([GAIN_OF_FILE[f] if f >= 0 else 1.0 for f in FILES], device=dev)
    index = torch.tensor([INDEX_OF_FILE[f] if f >= 0 else 0 for f in FILES], dtype=torch.int32, device=dev)
    bank = _bank(dev, list(_responses()))
    want = ops.clip_logmel(wet_table, lm, FILES, STARTS, R.WIDTH, R.FILL)
    got = ops.clip_logmel(corpus[i16], lm, FILES, STARTS, R.WIDTH, R.FILL, gain=gain, room=(bank, index))
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    fill = (want == R.FILL).all(dim=1).sum(dim=1).tolist()
    # the file start, its end, behind it, the short file, the empty file (its one frame of zeros is log(1e-8), which IS the fill value), no file
    assert fill == [3, 9, R.WIDTH, R.WIDTH - 3, R.WIDTH, R.WIDTH]
    # the tables ops.clip_room returns are the emulator's
    wet, samp0, ofile, ostart = ops.clip_room(corpus[i16], FILES, STARTS, R.WIDTH, bank, index, R.HOP, gain=gain)
    t = R.pseudo_tables([R.LENS[f] if f >= 0 else -1 for f in FILES], STARTS, span=wet.shape[1])
    assert wet.shape == (B, R.span_of()) and np.array_equal(samp0.cpu().numpy(), t['samp0'])
    assert np.array_equal(ofile.cpu().numpy(), t['win_file']) and np.array_equal(ostart.cpu().numpy(), t['win_start'])
    # noise under a room is the second launch's: the same call is reproducible, and the noise is there
    a, b = (ops.clip_logmel(corpus[i16], lm, FILES, STARTS, R.WIDTH, R.FILL, gain=gain, noise_std=torch.full((B,), 1e-2, device=dev), seed=5, room=(bank, index)) for _ in range(2))
    assert torch.equal(a, b) and not torch.equal(a, got) and torch.equal(a == R.FILL, got == R.FILL)


def _note(pitch, onset, offset, velocity=64):
    return {'pitch': pitch, 'onset': onset, 'offset': offset, 'velocity': velocity}


def test_store_under_a_room(dev):
    from corpus import synth_audio as SA
    from corpus.make_dataset import assemble_wave_store
    from hftt_hip import ops
    from hftt_hip.trainer import TrainStep
    from training.dataset import WaveAugment, WaveClipStore
    c = util.MINI
    config = {'feature': {'mel_bins': c.n_bin, 'n_bins': c.n_bin, 'fft_bins': 2048, 'window_length': 2048, 'log_offset': 1e-8, 'sr': 16000, 'hop_sample': 256},
              'input': {'margin_b': c.n_margin, 'margin_f': c.n_margin, 'num_frame': c.n_frame, 'min_value': -18.420681, 'max_value': 0.0},
              'midi': {'note_min': 21, 'num_note': c.n_note, 'num_velocity': c.n_velocity}}
    notes = [[_note(21 + (3 * i) % c.n_note, 0.05 + 0.06 * i, 0.2 + 0.06 * i, 1 + i % (c.n_velocity - 1)) for i in range(10)], [_note(25, 0.1, 0.3, 5)]]
    waves = [SA.pluck_wave(a, dur=d).numpy() for a, d in zip(notes, (0.9, 0.5))]
    store = assemble_wave_store(waves, notes, config)
    ir, taps = SA.synth_room_bank(4, 16000, taps=1024, rt60=(0.05, 0.2), seed=2)
    bank = ops.RoomBank(ir, dev, taps=taps)
    ids = [i % len(WaveClipStore(store, config, dev)) for i in range(6)]

    def draws(seed):
        """the room draws of the first batch under `seed`, as the store makes them: behind the gain draw"""
        aug = WaveAugment(room_p=0.5, room_bank=bank, gain_db=(-3.0, 3.0), seed=seed)
        aug.reset(dev)
        aug.draw(len(ids))
        return aug.draw_room(len(ids)).cpu()
    seed = next(s for s in range(64) if 0 < int((draws(s) < 0).sum()) < len(ids))          # a seed with dry and wet clips in one batch
    kw, index = dict(gain_db=(-3.0, 3.0), seed=seed), draws(seed)

    def batch(**more):
        return WaveClipStore(store, config, dev, augment=WaveAugment(**kw, **more)).batch(ids)
    room, again, plain = batch(room_p=0.5, room_bank=bank), batch(room_p=0.5, room_bank=bank), batch()
    for k in range(1, 5):
        assert torch.equal(room[k], plain[k]), k                 # the labels of every clip
    for b in range(len(ids)):
        assert torch.equal(room[0][b], plain[0][b]) == bool(index[b] < 0), (b, int(index[b]))
    assert all(torch.equal(x, y) for x, y in zip(room, again)) and bool(torch.isfinite(room[0]).all())
    wet = WaveClipStore(store, config, dev, augment=WaveAugment(room_p=1.0, room_bank=bank, noise_dbfs=(-60.0, -50.0), **kw))
    model = util.build_model(c, 5).to(dev)
    model.hftt_precision = 'x3'
    model.train()
    step = TrainStep(model, lr=1e-4)
    losses = []
    for i, b in enumerate(wet.loader(2, shuffle=True, seed=2)):
        if i == 3:
            break
        losses.append(step(b[0], *b[1:]).clone())
    assert len(losses) == 3 and all(bool(torch.isfinite(l).all()) for l in losses)
