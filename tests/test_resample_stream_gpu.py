"""hftt_resample_stream (csrc/resample_stream.hip) and the wave side of NoteStream on the device.

The kernel: every push's outputs torch.equal the carried-state model of tests/resample_stream_emul.py, every stream's concatenated outputs
torch.equal the whole-file kernel ops.resample, S streams in the same launches, inside a NaN arena that stays untouched outside the planned
footprint.  The frames: ops.stream_logmel over the resampled store torch.equal ops.LogMel of the whole resampled file, in a store whose slot
is the chunk plus a constant.  The model: audio at 44.1 / 48 kHz pushed in pieces into amt.open_stream(sr=...) gives exactly
transcript_notes(wave2feature(whole, sr)); launch counts per push_wave do not depend on the number of streams."""
import os

import pytest
import torch

import frontend_emul as F
import resample_stream_emul as E
import util

pytestmark = pytest.mark.gpu

GUARD = 4096


def _arena_store(dev, S, slot_len):
    arena = torch.full((2 * GUARD + S * slot_len,), float('nan'), device=dev)
    return arena, arena[GUARD:GUARD + S * slot_len].view(S, slot_len)


def _drive(dev, sr, waves, chunk, skips=(), close_with_last=()):
    """push `waves` (host tensors) in pieces of `chunk` through one ResampleStream; streams in `skips` get nothing in every second call;
    streams in `close_with_last` close in the call of their last piece, the others in a call of their own.  Every call's outputs are held
    against the model; -> the state, the arena, each stream's concatenated outputs (host)."""
    from hftt_hip import ops
    kern, up, down, width = F.resample_table(sr)
    S = len(waves)
    slot_len = max(F.resample_n_out(w.numel(), up, down) for w in waves) + 2048 + 512
    arena, store = _arena_store(dev, S, slot_len)
    rs = ops.ResampleStream(S, sr, 16000, dev, store=store)
    emul = [E.StreamEmul(kern, up, down, width) for _ in range(S)]
    pos, outs, k = [0] * S, [[] for _ in range(S)], 0
    while not all(rs.closed):
        chunks, closing = [None] * S, [False] * S
        for s in range(S):
            if rs.closed[s] or (s in skips and k % 2):
                continue
            n = waves[s].numel()
            if pos[s] < n:
                chunks[s] = waves[s][pos[s]:pos[s] + chunk]
                pos[s] += chunk
                closing[s] = s in close_with_last and pos[s] >= n
            else:
                closing[s] = True
        res = ops.resample_stream(rs, chunks, closing)
        for s in range(S):
            if chunks[s] is None and not closing[s]:
                assert res[s][1] == 0
                continue
            want = emul[s]._step(chunks[s], closing[s])
            got = rs.read(s, *res[s]).cpu()
            assert res[s] == (emul[s].n_done - want.numel(), want.numel()), (s, k, res[s])
            assert torch.equal(got, want), (s, k, res[s])
            outs[s].append(got)
        k += 1
        assert k < 10000
    return rs, arena, [torch.cat(o) for o in outs]


def _check_whole_and_arena(dev, sr, rs, arena, waves, outs):
    from hftt_hip import ops
    S, L = rs.S, rs.slot_len
    assert torch.isnan(arena[:GUARD]).all() and torch.isnan(arena[GUARD + S * L:]).all()
    for s, w in enumerate(waves):
        wf = w.float() * (1.0 / 32768.0) if w.dtype == torch.int16 else w
        whole = ops.resample(wf.to(dev), sr, 16000)
        n_out = whole.numel()
        assert outs[s].numel() == n_out and torch.equal(outs[s], whole.cpu()), s
        fill = rs.fill_of(n_out)
        assert 1024 - 256 < fill <= 1024
        assert torch.equal(rs.store[s, :n_out], whole), s                                   # nothing slid here: the slot holds the file
        assert (rs.store[s, n_out:n_out + fill] == 0).all() and torch.isnan(rs.store[s, n_out + fill:]).all(), s


@pytest.mark.parametrize('chunk', ['37', 'down', 'taps', '4096'])
def test_three_streams_in_the_same_launches(dev, chunk):
    sr = 44100
    kern, up, down, width = F.resample_table(sr)
    taps = kern.shape[1]
    n = 3 * down + 2 * taps + 7
    chunk = {'37': 37, 'down': down, 'taps': taps, '4096': 4096}[chunk]
    waves = [F.resample_noise(n, 11), F.resample_noise(n // 2, 12), F.resample_noise(n, 13)]
    rs, arena, outs = _drive(dev, sr, waves, chunk, skips=(2,), close_with_last=(0,))      # stream 1 ends midway, the others go on
    _check_whole_and_arena(dev, sr, rs, arena, waves, outs)


@pytest.mark.parametrize('sr', [48000, 8000, 22050])
def test_one_stream_at_other_rates(dev, sr):
    kern, up, down, width = F.resample_table(sr)
    taps = kern.shape[1]
    n = 3 * down + 2 * taps + 7
    for chunk in (37, down, taps, 4096):
        waves = [F.resample_noise(n, sr + chunk)]
        rs, arena, outs = _drive(dev, sr, waves, chunk)
        _check_whole_and_arena(dev, sr, rs, arena, waves, outs)


@pytest.mark.parametrize('sr', [44100, 8000])
def test_int16_chunks(dev, sr):
    kern, up, down, width = F.resample_table(sr)
    n = 3 * down + 2 * kern.shape[1] + 7
    for chunk in (37, 4096):
        waves = [torch.round(F.resample_noise(m, 5 + chunk + s) * 32768.0).clamp(-32768, 32767).to(torch.int16) for s, m in enumerate((n, n // 3))]
        rs, arena, outs = _drive(dev, sr, waves, chunk, close_with_last=(1,))
        _check_whole_and_arena(dev, sr, rs, arena, waves, outs)
    # a floating-point chunk beside int16 ones in one call: the int16 pieces are converted on the host side, to the same values
    waves = [waves[0], F.resample_noise(n, 99)]
    rs, arena, outs = _drive(dev, sr, waves, 300)
    _check_whole_and_arena(dev, sr, rs, arena, waves, outs)


def _logmel(dev):
    from hftt_hip import ops
    return ops.LogMel(dev, sr=16000, n_fft=2048, hop=256, n_mels=256, log_offset=1e-8)


@pytest.mark.parametrize('sr', [44100, 16000])
def test_frames_over_the_store_equal_the_offline_logmel_in_bounded_memory(dev, sr):
    """two streams of different lengths, 1000-sample pushes: the frames of all pushes equal LogMel of the whole resampled file; the slot is
    the chunk's outputs plus n_fft + n_fft / 2 and a frame's worth of slack, whatever the stream's age (the store is fixed: a push that
    needed more would raise); a first frame sees zeros to its left, and nothing outside the store is written"""
    from hftt_hip import ops
    chunk = 1000
    if sr == 16000:
        up, down = 1, 1
    else:
        _, up, down, _ = F.resample_table(sr)
    slot_len = 2048 + -(-chunk * up // down) + 2 * up + 1024
    arena, store = _arena_store(dev, 2, slot_len)
    rs = ops.ResampleStream(2, sr, 16000, dev, store=store)
    lm = _logmel(dev)
    waves = [F.resample_noise(23 * chunk + 17, 1), F.resample_noise(9 * chunk, 2)]
    frames = [[], []]
    for k in range(24):
        chunks = [w[k * chunk:(k + 1) * chunk] if k * chunk < w.numel() else None for w in waves]
        closing = [k == 23, k == 9]
        ops.resample_stream(rs, chunks, closing)
        for s, f in enumerate(ops.stream_logmel(rs, lm)):
            if f is not None:
                frames[s].append(f.clone())
    assert all(rs.closed) and rs.slot_len == slot_len and rs.store.data_ptr() == store.data_ptr()
    assert torch.isnan(arena[:GUARD]).all() and torch.isnan(arena[GUARD + 2 * slot_len:]).all()
    for s, w in enumerate(waves):
        whole = ops.resample(w.to(dev), sr, 16000) if sr != 16000 else w.to(dev)
        want = lm(whole)
        got = torch.cat(frames[s])
        assert got.shape == want.shape and torch.equal(got, want), s


def test_a_stream_closed_without_samples_is_one_silent_frame(dev):
    from hftt_hip import ops
    lm = _logmel(dev)
    for sr in (44100, 16000):
        rs = ops.ResampleStream(2, sr, 16000, dev)
        assert ops.resample_stream(rs, [None, None], [True, False]) == [(0, 0), (0, 0)]
        f = ops.stream_logmel(rs, lm)
        assert f[1] is None and f[0].shape == (1, 256) and torch.equal(f[0], lm(torch.zeros(1, device=dev)))
        assert rs.n_done == [0, 0] and rs.closed == [True, False]
        with pytest.raises(ops.HfttError, match='closed'):
            ops.resample_stream(rs, [torch.zeros(5), None])
        assert ops.resample_stream(rs, [None, torch.zeros(0)]) == [(0, 0), (0, 0)]         # nothing to do: no launch, no error


# ---------------------------------------------------------------------- the model
@pytest.fixture(scope='module')
def trained(dev):
    """the tiny trained model, a 44.1 kHz recording made from the synthetic pluck without new fixtures, and its offline transcription"""
    from corpus import synth_audio as SA
    from hftt_hip import ops
    from model.amt import AMT
    amt = AMT(SA.default_config(), os.path.join(util.ROOT, 'tests', 'golden', 'config5_tiny_trained.pkl'), batch_size=2)
    for seed in (1234, 4321):
        x = ops.resample(SA.pluck_wave(SA.pluck_notes(seed, 5.0), 5.0).to(dev), 16000, 44100).cpu()
        want = amt.transcript_notes(amt.wave2feature(x[None], 44100, on_device=True))
        if want:
            break
    return amt, x, want


def _stream_all(st, pieces):
    notes = []
    for p in pieces:
        notes += st.push_wave(p)
    early = len(notes)
    notes += st.close()
    return sorted(sorted(notes, key=lambda x: x['pitch']), key=lambda x: x['onset']), early


@pytest.mark.parametrize('n_samples', [1000, 4410, 12345])
def test_44k_pushes_equal_transcript_notes(dev, trained, n_samples):
    amt, x, want = trained
    st = amt.open_stream(sr=44100)
    got, early = _stream_all(st, [x[i:i + n_samples] for i in range(0, x.numel(), n_samples)])
    assert got == want and len(want) > 0 and early > 0


def test_44k_int16_and_two_channel_chunks(dev, trained):
    amt, x, _ = trained
    x16 = torch.round(x * 32768.0).clamp(-32768, 32767).to(torch.int16)
    want = amt.transcript_notes(amt.wave2feature((x16.float() * (1.0 / 32768.0))[None], 44100, on_device=True))
    got, early = _stream_all(amt.open_stream(sr=44100), [x16[i:i + 4410] for i in range(0, x16.numel(), 4410)])
    assert got == want and len(want) > 0 and early > 0
    two = torch.stack([x, 0.5 * torch.roll(x, 441) + 0.01 * F.resample_noise(x.numel(), 3)])          # the channels differ
    want = amt.transcript_notes(amt.wave2feature(two, 44100, on_device=True))
    got, early = _stream_all(amt.open_stream(sr=44100), [two[:, i:i + 12345] for i in range(0, two.shape[1], 12345)])
    assert got == want and len(want) > 0 and early > 0
    two16 = torch.stack([x16, torch.roll(x16, 441) // 2])
    want = amt.transcript_notes(amt.wave2feature(two16.float() * (1.0 / 32768.0), 44100, on_device=True))
    got, early = _stream_all(amt.open_stream(sr=44100), [two16[:, i:i + 12345] for i in range(0, two16.shape[1], 12345)])
    assert got == want and len(want) > 0


def test_two_recordings_at_48k_in_one_object(dev, trained):
    from corpus import synth_audio as SA
    from hftt_hip import HfttError, ops
    amt, _, _ = trained
    xa = ops.resample(SA.pluck_wave(SA.pluck_notes(1234, 5.0), 5.0).to(dev), 16000, 48000).cpu()
    xb = ops.resample(SA.pluck_wave(SA.pluck_notes(4321, 5.0), 5.0).to(dev), 16000, 48000).cpu()[:150001]
    want = [amt.transcript_notes(amt.wave2feature(w[None], 48000, on_device=True)) for w in (xa, xb)]
    st = amt.open_stream(n_streams=2, sr=48000)
    a = [xa[i:i + 9600] for i in range(0, xa.numel(), 9600)]
    b = [xb[i:i + 20011] for i in range(0, xb.numel(), 20011)]
    notes = [[], []]
    for k in range(max(len(a), len(b))):
        if k == len(b):
            for s, got in enumerate(st.close(which=[1])):
                notes[s] += got
        got = st.push_wave([a[k] if k < len(a) else None, b[k] if k < len(b) else None], sr=48000)
        for s in range(2):
            notes[s] += got[s]
    with pytest.raises(HfttError, match='closed'):
        st.push_wave([None, xb[:5]])
    for s, got in enumerate(st.close()):
        notes[s] += got
    srt = lambda x: sorted(sorted(x, key=lambda n: n['pitch']), key=lambda n: n['onset'])
    assert srt(notes[0]) == want[0] and srt(notes[1]) == want[1] and len(want[0]) > 0 and len(want[1]) > 0


def test_an_empty_stream_closes_without_notes(dev, trained):
    amt, _, _ = trained
    st = amt.open_stream(sr=44100)
    assert st.push_wave(torch.zeros(0)) == []
    assert st.close() == []


def test_launch_counts_do_not_depend_on_the_number_of_streams(dev, trained, monkeypatch):
    from hftt_hip import ops
    amt, x, _ = trained
    calls = {'resample_stream': 0, 'clip_logmel': 0, 'slide': 0, 'WaveTable': 0}

    def counting(name, fn):
        def wrapper(*a, **kw):
            calls[name] += 1
            return fn(*a, **kw)
        return wrapper
    monkeypatch.setattr(ops, 'resample_stream', counting('resample_stream', ops.resample_stream))
    monkeypatch.setattr(ops, 'clip_logmel', counting('clip_logmel', ops.clip_logmel))
    monkeypatch.setattr(ops, 'resample_stream_slide', counting('slide', ops.resample_stream_slide))
    monkeypatch.setattr(ops, 'WaveTable', counting('WaveTable', ops.WaveTable))
    S = 8
    st = amt.open_stream(n_streams=S, sr=44100)
    for k in range(4):
        before = dict(calls)
        st.push_wave([x[(s + k) * 5000:(s + k) * 5000 + 4000 + 100 * s] if (s + k) % 3 else None for s in range(S)])
        assert calls['resample_stream'] - before['resample_stream'] == 1
        assert calls['clip_logmel'] - before['clip_logmel'] <= 1 and calls['slide'] - before['slide'] <= 1
    assert calls['clip_logmel'] >= 2 and calls['WaveTable'] == 0
    st.close()
    assert calls['WaveTable'] == 0


def test_refusals(dev, trained):
    from hftt_hip import HfttError
    amt, x, _ = trained
    with pytest.raises(HfttError, match='rate'):
        amt.open_stream(sr=44100).push_wave(x[:100], sr=48000)
    with pytest.raises(HfttError, match='rate'):
        amt.open_stream().push_wave(x[:100], sr=44100)
    with pytest.raises(HfttError, match='rate'):
        amt.open_stream(sr=16001)
    st = amt.open_stream(sr=44100)
    with pytest.raises(HfttError, match='int16 or floating point'):
        st.push_wave(torch.zeros(10, dtype=torch.int32))
    with pytest.raises(HfttError, match='mono'):
        st.push_wave(torch.zeros(2, 2, 10))
