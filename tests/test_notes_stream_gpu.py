"""The streaming note decoder on the device (csrc/notes_stream.hip: hftt_notes_stream_step; ops.notes_stream_step; AMT.open_stream) against
AMT.mpe2note and against its numpy model (tests/notes_stream_emul.py) step by step, and end to end against AMT.transcript_notes.  Records
and times are compared with ==.  Overflow and capacity are statuses; no test provokes a fault."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import util
import notes_stream_emul as E

pytestmark = pytest.mark.gpu

HOP, THR = E.HOP, E.THR


def _host(on, off, mpe, vel, mv):
    from model.amt import AMT
    amt = AMT({'feature': {'sr': 16000, 'hop_sample': 256}, 'midi': {'note_min': 21, 'num_note': on.shape[1]}}, None, device='cpu')
    return amt.mpe2note(a_onset=on, a_offset=off, a_mpe=mpe, a_velocity=vel, thred_onset=THR[0], thred_offset=THR[1], thred_mpe=THR[2],
                        mode_velocity=mv, mode_offset='shorter')


class Dev:
    """S streams on the device next to one numpy model each, fed the same rows"""

    def __init__(self, dev, S, N, H, mv):
        from hftt_hip import ops
        self.st = ops.notes_stream_state(S, N, H, dev)
        self.em = [E.StreamEmul(N, H, HOP, *THR, mode_velocity=mv) for _ in range(S)]
        self.mv, self.S, self.N, self.H, self.dev = mv, S, N, H, dev

    def deliver(self, rows, close):
        """rows[s]: (on, off, mpe, vel) slices or None"""
        new = [0] * self.S
        for s, r in enumerate(rows):
            n = 0 if r is None else len(r[0])
            if n:
                idx = torch.from_numpy((self.st.row_end[s] + np.arange(n)) % self.H).to(self.dev)
                for ring, a in zip(self.st.rings, r):
                    ring[s, idx] = torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
            if r is not None or close[s]:
                z = np.zeros((0, self.N), np.float32)
                self.em[s].deliver(*(r if r is not None else (z, z, z, z.astype(np.int8))), close=close[s])
            new[s] = n
        self.st.deliver(new, close)

    def records(self):
        """the state's records as int64 [S, N, 8]: word 0 = commit frame, 1 = row_end, 2 = head + 1"""
        n = 64 * self.S * self.N
        return self.st.state[:n].cpu().numpy().view(np.int64).reshape(self.S, self.N, 8)

    def step(self, **kw):
        """one step of both; the device's notes per stream, checked against the models' with =="""
        from hftt_hip import ops
        pitch, vel, t_on, t_off, heads, overflow = (x.numpy() for x in ops.notes_stream_step(
            self.st, HOP, thred_onset=THR[0], thred_offset=THR[1], thred_mpe=THR[2], mode_velocity=self.mv, **kw))
        assert pitch.dtype == np.int32 and vel.dtype == np.int32 and t_on.dtype == np.float64 and t_off.dtype == np.float64
        assert heads[0] == 0 and heads[-1] == len(pitch) and (np.diff(heads) >= 0).all()
        out = []
        for s in range(self.S):
            a, b = int(heads[s]), int(heads[s + 1])
            got = [(int(pitch[q]), int(vel[q]), float(t_on[q]), float(t_off[q])) for q in range(a, b)]
            want, total = self.em[s].step()
            assert bool(overflow[s]) == self.em[s].overflow, (s, overflow[s])
            assert got == want, (s, got[:3], want[:3])                                          # order included: pitch-major, ascending onset frame
            out.append(got)
        rec = self.records()
        for s in range(self.S):
            if not self.em[s].overflow:
                assert (rec[s, :, 0] == self.em[s].st['c']).all() and (rec[s, :, 2] == self.em[s].st['head']).all(), s
        return out


def _run(dev, tr, H, mv, sizes):
    on, off, mpe, vel = tr
    F, N = on.shape
    d = Dev(dev, 1, N, H, mv)
    notes, r, k, early = [], 0, 0, 0
    while True:
        n = min(d.em[0].room(), F - r) if sizes == 'room' else sizes[k]
        last = r + n == F if sizes == 'room' else k == len(sizes) - 1
        d.deliver([tuple(a[r:r + n] for a in tr)], [last])
        r += n
        k += 1
        if last:
            early = len(notes)
        notes += d.step()[0]
        if last:
            break
    assert r == F and E.as_dicts(notes) == _host(on, off, mpe, vel, mv)
    return len(notes), early


@pytest.mark.parametrize('N', [1, 8, 88])
def test_random_tracks_every_split(dev, N):
    total = early = 0
    for F in (1, 2, 3, 7, 64, 257):
        tr = E.tracks(7 * F + N, F, N)
        for q, (kind, sizes) in enumerate(E.splits(F, 64, F).items()):
            if N == 88 and F == 257 and kind == 'rows':
                continue                                                                        # the model's slowest case: N = 8 holds it
            n, e = _run(dev, tr, 64, ('ignore_zero', 'org')[(q + F) % 2], sizes)
            if F == 257:
                total += n
                early += e
        _run(dev, tr, max(F, 4), 'org', [F])                                                    # everything in the closing step
    assert 257 > 3 * 64                                                                         # the ring wrapped more than three times
    if N >= 8:
        assert total > 50 and early >= 0.9 * total


def test_hand_built_and_constant_tracks(dev):
    for tr, H in ((E.hand_scene(), 128), (E.constant_scene(131), 192)):
        F = len(tr[0])
        for mv in ('ignore_zero', 'org'):
            for kind, sizes in E.splits(F, H, F).items():
                if kind == 'rows' and mv == 'org':
                    continue
                assert _run(dev, tr, H, mv, sizes)[0] > 20


def test_three_streams_of_different_lengths_in_the_same_launches(dev):
    N, H = 8, 64
    files = [E.tracks(31, 200, N), E.tracks(32, 77, N), E.tracks(33, 131, N)]
    d = Dev(dev, 3, N, H, 'ignore_zero')
    pos, notes, sizes = [0, 0, 0], [[], [], []], (13, 0, 29, 7)
    k = 0
    while not all(d.st.closed):
        rows, close = [], []
        for s, tr in enumerate(files):
            F = len(tr[0])
            if d.st.closed[s]:
                rows.append(None); close.append(False)
                continue
            n = min(sizes[(k + s) % 4], F - pos[s])
            rows.append(tuple(a[pos[s]:pos[s] + n] for a in tr))
            pos[s] += n
            close.append(pos[s] == F)
        d.deliver(rows, close)
        for s, got in enumerate(d.step()):
            notes[s] += got
        k += 1
    assert d.step() == [[], [], []]                                                              # closed and decoded: nothing more
    for s, tr in enumerate(files):
        assert E.as_dicts(notes[s]) == _host(*tr, 'ignore_zero') and len(notes[s]) > 5           # each as when decoded alone


def test_overflow_is_a_status(dev):
    """an onset plateau at the threshold that outgrows the ring: the notes in front of it are right, the flag is set, nothing follows"""
    N, H, F = 4, 32, 120
    on, off, mpe, vel = E.scene(F, N)
    on[5, 0] = 0.9; off[9, 0] = 0.9
    on[12, 1] = 0.9; mpe[15, 1] = 0.1
    on[30:, 2] = 0.7                                                                            # open from row 30 on, never decided
    on[100, 3] = 0.9
    d = Dev(dev, 1, N, H, 'org')
    notes, flagged = [], None
    for r in range(0, F, 8):
        d.deliver([(on[r:r + 8], off[r:r + 8], mpe[r:r + 8], vel[r:r + 8])], [False])
        notes += d.step()[0]                                                                    # == the model's, flag included
        if d.em[0].overflow and flagged is None:
            flagged = r
    assert flagged is not None and 30 + H <= flagged + 8 <= 30 + H + 8
    host = [x for x in _host(on[:30], off[:30], mpe[:30], vel[:30], 'org')]
    assert E.as_dicts(notes) == host and len(host) == 2


def _raw_step(d, cap, guard=64):
    """hftt_notes_stream_step through the C ABI with caller-owned outputs inside one arena: [guard | state copy | guard | counts ... | guard],
    every guard and every output pre-filled with a sentinel"""
    from hftt_hip import _capi
    st, S = d.st, d.S
    L = _capi.lib()
    dev = d.dev
    pitch = torch.full((cap + guard,), -77, dtype=torch.int32, device=dev)
    velocity = torch.full((cap + guard,), -78, dtype=torch.int32, device=dev)
    onset = torch.full((cap + guard,), -79.0, dtype=torch.float64, device=dev)
    offset = torch.full((cap + guard,), -80.0, dtype=torch.float64, device=dev)
    ints = torch.full((guard + 2 * S + 2 + guard,), -81, dtype=torch.int32, device=dev)        # n_notes, stream_notes [S + 1], overflow [S]
    nb = st.state.numel()
    arena = torch.full((guard + nb + guard,), 0x5A, dtype=torch.int8, device=dev)
    arena[guard:guard + nb] = st.state
    q = _capi.NotesStreamDesc()
    q.S, q.N, q.H, q.note_min, q.cap, q.max_new, q.hop_sec = S, d.N, d.H, 21, cap, st.max_new, HOP
    q.onset, q.offset, q.mpe, q.velocity = (t.data_ptr() for t in st.rings)
    q.row_end, q.closed = st.tables.data_ptr(), st.tables.data_ptr() + 8 * S
    q.thred_onset, q.thred_offset, q.thred_mpe = (float(np.float32(x)) for x in THR)
    q.mode_velocity, q.mode_offset = (0 if d.mv == 'ignore_zero' else 1), 0
    q.state, q.state_bytes = arena.data_ptr() + guard, nb
    q.out_pitch, q.out_velocity, q.out_onset, q.out_offset = pitch.data_ptr(), velocity.data_ptr(), onset.data_ptr(), offset.data_ptr()
    base = ints.data_ptr() + 4 * guard
    q.n_notes, q.stream_notes, q.overflow = base, base + 4, base + 4 * (S + 2)
    _capi.check(L.hftt_notes_stream_step(C.byref(q), torch.cuda.current_stream(dev).cuda_stream), 'notes_stream_step')
    torch.cuda.synchronize(dev)
    a = arena.cpu().numpy()
    i = ints.cpu().numpy()
    assert (a[:guard] == 0x5A).all() and (a[guard + nb:] == 0x5A).all()                         # nothing around the state
    assert (i[:guard] == -81).all() and (i[guard + 2 * S + 2:] == -81).all()                    # nothing around the counts
    return dict(total=int(i[guard]), heads=i[guard + 1:guard + S + 2], overflow=i[guard + S + 2:guard + 2 * S + 2], state=a[guard:guard + nb],
                out=(pitch.cpu().numpy(), velocity.cpu().numpy(), onset.cpu().numpy(), offset.cpu().numpy()))


def test_capacity_and_the_sentinel_arena(dev):
    N, H = 8, 128
    tr = E.tracks(41, 100, N)
    d = Dev(dev, 2, N, H, 'org')
    d.deliver([tuple(a[:60] for a in tr), tuple(a[:45] for a in tr)], [False, False])
    before = d.st.state.cpu().numpy().copy()
    assert not before.any()                                                                     # fresh streams: all zero
    full = _raw_step(d, 4096)
    n = full['total']
    assert n > 10 and full['heads'][0] == 0 and full['heads'][2] == n and not full['overflow'].any()
    for a, sentinel in zip(full['out'], (-77, -78, -79.0, -80.0)):
        assert (a[n:] == sentinel).all() and (a[:n] != sentinel).all()
    assert (full['state'] != before).any() and not full['state'][64 * 2 * N:].any()             # committed; the counts are zero between calls
    for cap in (0, 1, n - 1):
        got = _raw_step(d, cap)
        assert got['total'] == n and (got['heads'] == full['heads']).all()                      # the count that exists
        for a, sentinel in zip(got['out'], (-77, -78, -79.0, -80.0)):
            assert (a == sentinel).all()                                                        # nothing written, in front of cap or behind it
        assert (got['state'] == before).all()                                                   # the state stays bit-identical
    assert (d.st.state.cpu().numpy() == before).all()                                           # (the arena held a copy: the stream's own is untouched)
    from hftt_hip import HfttError, ops
    kw = dict(thred_onset=THR[0], thred_offset=THR[1], thred_mpe=THR[2], mode_velocity='org')
    with pytest.raises(HfttError, match='capacity'):
        ops.notes_stream_step(d.st, HOP, capacity=n - 1, **kw)
    assert (d.st.state.cpu().numpy() == before).all()
    got = d.step(capacity=n)                                                                    # the repeat gives the full result (== the models')
    assert sum(len(x) for x in got) == n
    exact = _raw_step(d, 0)                                                                     # behind the committed step nothing is pending
    assert exact['total'] == 0
    with pytest.raises(HfttError, match="'shorter'"):
        ops.notes_stream_step(d.st, HOP, mode_offset='longer')


# ---------------------------------------------------------------------- end to end
@pytest.fixture(scope='module')
def trained(dev):
    from corpus import synth_audio as SA
    from model.amt import AMT
    amt = AMT(SA.default_config(), os.path.join(util.ROOT, 'tests', 'golden', 'config5_tiny_trained.pkl'), batch_size=2)
    waves, feats = [], []
    for seed in (1234, 4321):
        wave = SA.pluck_wave(SA.pluck_notes(seed, 5.0), 5.0)
        waves.append(wave)
        feats.append(amt.wave2feature(wave.unsqueeze(0), SA.SR, on_device=True))
    return amt, waves, feats


def _stream_all(st, pieces, push):
    notes, early = [], 0
    for p in pieces:
        notes += push(p)
    early = len(notes)
    notes += st.close()
    return sorted(sorted(notes, key=lambda x: x['pitch']), key=lambda x: x['onset']), early


def _cut(a, n):
    return [a[i:i + n] for i in range(0, len(a), n)]


@pytest.mark.parametrize('n_frames', [1, 37, 128, 300])
def test_feature_pushes_equal_transcript_notes(dev, trained, n_frames):
    amt, waves, feats = trained
    feat = feats[0]
    T = amt.config['input']['num_frame']
    assert -(-feat.shape[0] // T) == 3                                                          # three clips
    before = amt.transcript_notes(feat)
    forms = [dict()] if n_frames == 1 else [dict(), dict(output='A'), dict(n_offset=T // 4), dict(n_offset=T // 4, output='A'),
                                            dict(thred_onset=0.4, thred_offset=0.3, thred_mpe=0.45, mode_velocity='org')]
    for kw in forms:
        want = amt.transcript_notes(feat, **kw)
        st = amt.open_stream(**kw)
        src = feat.cpu().numpy() if n_frames == 37 else feat                                    # numpy arrays and device tensors
        got, early = _stream_all(st, _cut(src, n_frames), st.push)
        assert got == want and len(want) > 0, kw
        if 'n_offset' in kw or n_frames < 300:
            assert early > 0, kw                                                                # notes in front of the close
    assert amt.transcript_notes(feat) == before                                                 # the AMT itself is as it was


@pytest.mark.parametrize('n_samples', [1000, 4096, 12345])
def test_wave_pushes_equal_transcript_notes(dev, trained, n_samples):
    from corpus import synth_audio as SA
    amt, waves, feats = trained
    want = amt.transcript_notes(feats[0])
    st = amt.open_stream()
    wave = waves[0] if n_samples != 4096 else torch.round(waves[0] * 32768.0).clamp(-32768, 32767).to(torch.int16)
    if n_samples == 4096:
        want = amt.transcript_notes(amt.wave2feature((wave.float() / 32768.0).unsqueeze(0), SA.SR, on_device=True))
    got, early = _stream_all(st, _cut(wave, n_samples), lambda p: st.push_wave(p, sr=SA.SR))
    assert got == want and early > 0 and len(want) > 0
    from hftt_hip import HfttError
    with pytest.raises(HfttError, match='rate'):
        amt.open_stream().push_wave(wave[:100], sr=44100)


def test_two_recordings_in_one_stream_object(dev, trained):
    from hftt_hip import HfttError
    amt, waves, feats = trained
    want = [amt.transcript_notes(f) for f in feats]
    st = amt.open_stream(n_streams=2)
    notes = [[], []]
    a, b = _cut(feats[0], 50), _cut(feats[1][:200], 90)                                         # different lengths, different chunkings
    for k in range(max(len(a), len(b))):
        if k == len(b):
            for s, got in enumerate(st.close(which=[1])):
                notes[s] += got
        got = st.push([a[k] if k < len(a) else None, b[k] if k < len(b) else None])
        for s in range(2):
            notes[s] += got[s]
    with pytest.raises(HfttError, match='closed'):
        st.push([None, feats[1][:5]])
    for s, got in enumerate(st.close()):
        notes[s] += got
    srt = lambda x: sorted(sorted(x, key=lambda n: n['pitch']), key=lambda n: n['onset'])
    assert srt(notes[0]) == want[0]
    assert srt(notes[1]) == amt.transcript_notes(feats[1][:200])
