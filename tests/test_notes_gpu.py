"""The device note decoder (csrc/notes.hip: hftt_stitch, hftt_notes_decode; AMT.transcript_notes) against the host path it restates:
AMT.transcript / transcript_stride / mpe2note, which tests/golden/amt.npz pins to the reference.  Times are compared with ==."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import util

pytestmark = pytest.mark.gpu

HOP = 256 / 16000
MODES = [(mv, mo) for mv in ('ignore_zero', 'org') for mo in ('shorter', 'longer', 'offset')]


def _amt(N, note_min=21):
    from model.amt import AMT
    return AMT({'feature': {'sr': 16000, 'hop_sample': 256}, 'midi': {'note_min': note_min, 'num_note': N}}, None)


def _device_notes(dev, on, off, mpe, vel, note_min=21, **kw):
    """ops.notes_decode on the device + the host sort of AMT.transcript_notes -> the list of dicts mpe2note returns"""
    from hftt_hip import ops
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (on, off, mpe, vel)]
    pitch, velocity, onset, offset = (x.cpu().numpy() for x in ops.notes_decode(*t, HOP, note_min=note_min, **kw))
    assert pitch.dtype == np.int32 and velocity.dtype == np.int32 and onset.dtype == np.float64 and offset.dtype == np.float64
    # the order in front of the sort: pitch-major, ascending onset FRAME (onset times of one pitch may tie or cross by the refinement)
    assert (np.diff(pitch) >= 0).all()
    order = np.lexsort((pitch, onset))
    return [{'pitch': int(pitch[i]), 'onset': float(onset[i]), 'offset': float(offset[i]), 'velocity': int(velocity[i])} for i in order]


def _same(dev, on, off, mpe, vel, modes=MODES, thr=(0.6, 0.55, 0.5)):
    """device == AMT.mpe2note, exactly, for every mode pair; returns the number of notes compared"""
    amt = _amt(on.shape[1])
    total = 0
    for mv, mo in modes:
        kw = dict(thred_onset=thr[0], thred_offset=thr[1], thred_mpe=thr[2], mode_velocity=mv, mode_offset=mo)
        host = amt.mpe2note(a_onset=on, a_offset=off, a_mpe=mpe, a_velocity=vel, **kw)
        got = _device_notes(dev, on, off, mpe, vel, **kw)
        assert len(got) == len(host), (mv, mo, len(got), len(host))
        for a, b in zip(got, host):
            assert a == b, (mv, mo, a, b)            # pitch, velocity ints; onset, offset doubles compared with ==
        total += len(host)
    return total


def _tracks(seed, F, N):
    """the generator recipe of tests/golden/make_golden.py::make_amt at any F, N: smoothed noise quantised to 1/20 (plateaus, exact ties)"""
    r = np.random.RandomState(seed)

    def track():
        x = r.rand(F + 8, N).astype(np.float32)
        k = np.ones(5, np.float32) / 5
        x = np.stack([np.convolve(x[:, j], k, mode='valid') for j in range(N)], 1)[:F]
        x = (x - x.min()) / max(x.max() - x.min(), np.float32(1e-6))
        return (np.round(x * 20) / 20).astype(np.float32)
    on, off, mpe = track(), track(), track()
    vel = r.randint(0, 128, size=(F, N)).astype(np.int8)
    vel[r.rand(F, N) < 0.1] = 0
    return on, off, mpe, vel


def test_reference_goldens(dev):
    g = util.golden('amt')
    amt = _amt(88)
    total = 0
    for case in range(2):
        on, off, mpe, vel = (g[f'm2n.{case}.{k}'] for k in ('onset', 'offset', 'mpe', 'velocity'))
        assert on.shape == (160, 88)
        for mv, mo in MODES:
            kw = dict(thred_onset=0.6, thred_offset=0.55, thred_mpe=0.5, mode_velocity=mv, mode_offset=mo)
            got = _device_notes(dev, on, off, mpe, vel, **kw)
            ref = g[f'm2n.{case}.{mv}.{mo}']
            assert len(got) == len(ref), (case, mv, mo)
            arr = np.array([[x['pitch'], x['onset'], x['offset'], x['velocity']] for x in got]).reshape(-1, 4)
            np.testing.assert_array_equal(arr[:, [0, 3]], ref[:, [0, 3]])
            np.testing.assert_allclose(arr[:, 1:3], ref[:, 1:3], rtol=0, atol=2e-6)     # the reference's float64 against the float32 refinement
            host = amt.mpe2note(a_onset=on, a_offset=off, a_mpe=mpe, a_velocity=vel, **kw)
            assert got == host, (case, mv, mo)
            total += len(got)
    assert total > 1000


def _chunk():
    from hftt_hip import _capi
    return _capi.NOTES_CHUNK


@pytest.mark.parametrize('N', [1, 8, 88])
@pytest.mark.parametrize('Fk', ['1', '2', '3', '7', '64', 'chunk-1', 'chunk', 'chunk+1', '2chunk+1'])
def test_random_tracks_at_the_smallest_shapes(dev, Fk, N):
    ch = _chunk()
    F = {'chunk-1': ch - 1, 'chunk': ch, 'chunk+1': ch + 1, '2chunk+1': 2 * ch + 1}.get(Fk) or int(Fk)
    total = 0
    for seed in range(3):
        on, off, mpe, vel = _tracks(1000 * seed + 7 * F + N, F, N)
        total += _same(dev, on, off, mpe, vel, modes=MODES if seed == 0 else [MODES[(seed + F) % 6]])
    if F >= 64 and N >= 8:
        assert total > 0


def _scene(F, N=8):
    on = np.full((F, N), 0.1, np.float32)
    off = np.full((F, N), 0.1, np.float32)
    mpe = np.full((F, N), 0.9, np.float32)
    vel = np.full((F, N), 64, np.int8)
    return on, off, mpe, vel


def test_constant_tracks_at_and_just_below_the_threshold(dev):
    """a constant track at the threshold: every frame is an onset (F notes, N * F capacity), each trimmed to the next one's onset; just
    below: none.  The same for the offset track, and an mpe track that is below everywhere."""
    ch = _chunk()
    F = ch + 3
    on, off, mpe, vel = _scene(F, 4)
    thr = np.float32(0.6)
    on[:, 0] = thr
    on[:, 1] = np.nextafter(thr, np.float32(0))
    on[:, 2] = thr; off[:, 2] = np.float32(0.55)            # every frame an onset AND an offset peak
    on[:, 3] = thr; mpe[:, 3] = 0.2                         # every frame an onset, mpe below everywhere
    vel[5::7, 2] = 0
    n = _same(dev, on, off, mpe, vel)
    amt = _amt(4)
    assert len(amt.mpe2note(a_onset=on, a_offset=off, a_mpe=mpe, a_velocity=vel, thred_onset=0.6, thred_offset=0.55, mode_velocity='org')) == 3 * F
    assert n > 3 * F * 3
    # all pitches full: the capacity bound N * F is reached, not N * F / 2
    on[:] = thr
    got = _device_notes(dev, on, off, mpe, vel, thred_onset=0.6, thred_offset=0.55, mode_velocity='org')
    assert len(got) == 4 * F


def test_hand_built_tracks(dev):
    ch = _chunk()
    F = 2 * ch + 1
    on, off, mpe, vel = _scene(F)
    # pitch 0: plateaus over the chunk border -- a peak plateau, one with a higher left neighbour, one with a higher right neighbour
    on[ch - 3:ch + 4, 0] = 0.8
    on[2 * ch - 2:2 * ch, 0] = 0.8; on[2 * ch - 3, 0] = 0.95                                # higher value left of the plateau: only it peaks
    off[ch - 1:ch + 1, 0] = 0.7                                                             # an offset plateau over the border
    # pitch 1: a plateau longer than a chunk (starts in chunk 0, ends in chunk 2) and a plateau running to the last frame on the offset track
    on[ch - 2:2 * ch + 1, 1] = 0.7
    off[F - 5:, 1] = 0.9
    # pitch 2: a plateau running to the last frame; single peaks at frame 0 and (pitch 3) at F - 1 with unequal neighbours
    on[F - 5:, 2] = 0.9
    on[0, 2] = 0.9; on[1, 2] = 0.3
    on[F - 1, 3] = 0.9; on[F - 2, 3] = 0.4
    off[0, 3] = 0.8; off[F - 1, 3] = 0.8
    # pitch 3 too: l == r ties, and both signs of the refinement
    on[10, 3] = 0.9; on[9, 3] = on[11, 3] = 0.4
    on[20, 3] = 0.9; on[19, 3] = 0.3; on[21, 3] = 0.5
    on[30, 3] = 0.9; on[29, 3] = 0.5; on[31, 3] = 0.3
    off[25, 3] = 0.9; off[24, 3] = 0.2; off[26, 3] = 0.3
    # pitch 4: an onset whose offset peak lies beyond the next onset (clipped), an mpe dip at loc_onset + 1, velocity 0
    on[10, 4] = 0.9; on[20, 4] = 0.9; off[30, 4] = 0.9
    on[40, 4] = 0.9; mpe[41, 4] = 0.1
    on[50, 4] = 0.9; vel[50, 4] = 0
    on[52, 4] = 0.9; off[51, 4] = 0.9; mpe[60, 4] = 0.1                                      # offset peak AT / before the onset does not count
    on[70, 4] = 0.9; off[75, 4] = 0.9; mpe[73, 4] = 0.1                                      # both flags: shorter / longer / offset differ
    on[80, 4] = 0.9; off[83, 4] = 0.9; mpe[86, 4] = 0.1
    on[90, 4] = 0.9; off[93, 4] = 0.9; mpe[93, 4] = 0.1                                      # loc_offset == loc_mpe
    on[ch - 1, 4] = 0.9; off[ch, 4] = 0.9; mpe[ch + 1, 4] = 0.1                              # the three lists on different sides of the border
    # pitch 5: no onset at all, between pitches that have some;  pitch 6: velocity 0 only;  pitch 7: overlapping notes (the trim) with a dropped
    # note in between -- the trim is between KEPT notes
    on[15, 6] = 0.9; vel[15, 6] = 0
    on[100, 7] = 0.9; on[104, 7] = 0.9; on[108, 7] = 0.9; vel[104, 7] = 0; off[200, 7] = 0.9
    on[2 * ch - 1, 7] = 0.9; on[2 * ch, 7] = 0.3
    n = _same(dev, on, off, mpe, vel)
    assert n > 6 * 20
    amt = _amt(8)
    host = amt.mpe2note(a_onset=on, a_offset=off, a_mpe=mpe, a_velocity=vel, thred_onset=0.6, thred_offset=0.55, thred_mpe=0.5, mode_velocity='org')
    pitches = {x['pitch'] for x in host}
    assert 21 + 5 not in pitches and {21 + 4, 21 + 6, 21 + 7} <= pitches
    assert len([x for x in host if x['pitch'] == 22]) == ch + 3                              # the long plateau: one note per frame
    # thresholds as float32: a value one ulp under the float32 threshold stays out, the float32 threshold itself is in (0.6 is no float32)
    on2, off2, mpe2, vel2 = _scene(8, 2)
    on2[3, 0] = np.float32(0.6); on2[3, 1] = np.nextafter(np.float32(0.6), np.float32(0))
    assert _same(dev, on2, off2, mpe2, vel2) == 6


def _raw_decode(dev, on, off, mpe, vel, cap, guard=64, **kw):
    """hftt_notes_decode through the C ABI with caller-owned outputs of cap + guard records, the guard pre-filled with a sentinel"""
    from hftt_hip import _capi, ops
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (on, off, mpe, vel)]
    F, N = on.shape
    L = _capi.lib()
    ws = torch.empty(L.hftt_notes_ws_bytes(F, N), dtype=torch.int8, device=dev)
    pitch = torch.full((cap + guard,), -77, dtype=torch.int32, device=dev)
    velocity = torch.full((cap + guard,), -78, dtype=torch.int32, device=dev)
    onset = torch.full((cap + guard,), -79.0, dtype=torch.float64, device=dev)
    offset = torch.full((cap + guard,), -80.0, dtype=torch.float64, device=dev)
    total = torch.full((1,), -1, dtype=torch.int32, device=dev)
    d = _capi.NotesDesc()
    d.F, d.N, d.note_min, d.cap, d.hop_sec = F, N, 21, cap, HOP
    d.onset, d.offset, d.mpe, d.velocity = (x.data_ptr() for x in t)
    d.thred_onset, d.thred_offset, d.thred_mpe = 0.6, 0.55, 0.5
    d.mode_velocity, d.mode_offset = ops.MODE_VELOCITY[kw.get('mode_velocity', 'ignore_zero')], ops.MODE_OFFSET[kw.get('mode_offset', 'shorter')]
    d.out_pitch, d.out_velocity, d.out_onset, d.out_offset, d.n_notes = pitch.data_ptr(), velocity.data_ptr(), onset.data_ptr(), offset.data_ptr(), total.data_ptr()
    d.ws, d.ws_bytes = ws.data_ptr(), ws.numel()
    _capi.check(L.hftt_notes_decode(C.byref(d), torch.cuda.current_stream(dev).cuda_stream), 'notes_decode')
    torch.cuda.synchronize(dev)
    return int(total.item()), pitch.cpu().numpy(), velocity.cpu().numpy(), onset.cpu().numpy(), offset.cpu().numpy()


def test_capacity(dev):
    from hftt_hip import HfttError, ops
    g = util.golden('amt')
    on, off, mpe, vel = (g[f'm2n.0.{k}'] for k in ('onset', 'offset', 'mpe', 'velocity'))
    n_ref = len(g['m2n.0.ignore_zero.shorter'])
    full = _raw_decode(dev, on, off, mpe, vel, n_ref)
    assert full[0] == n_ref
    for cap in (0, 1, n_ref // 2, n_ref - 1):
        total, *arrs = _raw_decode(dev, on, off, mpe, vel, cap)
        assert total == n_ref                                               # the true count, not the capped one
        for a, b, sentinel in zip(arrs, full[1:], (-77, -78, -79.0, -80.0)):
            np.testing.assert_array_equal(a[:cap], b[:cap])                 # the first cap records of the uncapped run
            assert (a[cap:] == sentinel).all()                              # nothing behind cap
    for a, sentinel in zip(full[1:], (-77, -78, -79.0, -80.0)):
        assert (a[n_ref:] == sentinel).all() and (a[:n_ref] != sentinel).all()
    t = [torch.from_numpy(a).to(dev) for a in (on, off, mpe, vel)]
    kw = dict(thred_onset=0.6, thred_offset=0.55, thred_mpe=0.5)
    with pytest.raises(HfttError, match='capacity'):
        ops.notes_decode(*t, HOP, capacity=n_ref - 1, **kw)
    assert len(ops.notes_decode(*t, HOP, capacity=n_ref, **kw)[0]) == n_ref
    # without capacity= the wrapper runs once more with the exact count: a file with more notes than the default room
    F, N = 4096, 2
    on2 = np.full((F, N), 0.7, np.float32); z = np.full((F, N), 0.1, np.float32); v2 = np.full((F, N), 5, np.int8)
    assert ops.notes_default_capacity(F, N) < N * F
    t2 = [torch.from_numpy(a).to(dev) for a in (on2, z, z + 0.8, v2)]
    pitch = ops.notes_decode(*t2, HOP, **kw)[0]
    assert len(pitch) == N * F
    # F == 0: no notes, no launch
    e = [torch.zeros(0, 88, device=dev), torch.zeros(0, 88, device=dev), torch.zeros(0, 88, device=dev), torch.zeros(0, 88, dtype=torch.int8, device=dev)]
    assert all(len(x) == 0 for x in ops.notes_decode(*e, HOP))


@pytest.mark.parametrize('shape', [(3, 8, 8, 4), (2, 128, 88, 128), (2, 8, 5, 7), (1, 4, 3, 100)], ids=lambda s: 'x'.join(map(str, s)))
def test_stitch(dev, shape):
    """hftt_stitch against the host assembly of AMT.transcript (whole clips) and transcript_stride (rows n_offset .. n_offset + T/2), bit for
    bit, int8 velocity roll included; exact ties planted in the logits; rows that no clip covers keep what they held."""
    from hftt_hip import ops
    b, T, N, V = shape
    r = np.random.RandomState(b * 1000 + V)
    o3 = [r.rand(b, T, N).astype(np.float32) for _ in range(3)]
    vel = r.randn(b, T, N, V).astype(np.float32)
    flat = vel.reshape(-1, V)
    top = flat.max(1) + 1.0
    flat[0::5, 0] = top[0::5]; flat[0::5, V - 1] = top[0::5]                         # a tie between index 0 and the last index
    flat[1::5, V // 2] = top[1::5]; flat[1::5, V - 1] = top[1::5]                    # a tie between two lanes' shares
    if V >= 4:
        flat[2::5, 1] = top[2::5]; flat[2::5, 2] = top[2::5]                         # a tie inside one 16-byte load
    flat[3::5, :] = 0.25                                                             # all equal: index 0
    want_arg = vel.argmax(3)
    assert (want_arg[np.unravel_index(np.arange(0, b * T * N, 5), (b, T, N))] == 0).all()
    assert (torch.from_numpy(vel).argmax(3).numpy() == want_arg).all()               # torch.argmax (the host path's) agrees with numpy's
    dev_o = [torch.from_numpy(a).to(dev) for a in o3] + [torch.from_numpy(vel).to(dev)]
    half = T // 2
    forms = [(T, 0)] + [(half, n_off) for n_off in (0, T // 4, T // 2)]
    for length, src0 in forms:
        covered = b * length
        F = covered + 5                                                              # five rows that no clip covers
        starts = [c * length for c in range(b)]
        if length == T:
            starts = starts[::-1]                                                    # any order of disjoint rows
        rolls = [torch.full((F, N), 7.0, device=dev) for _ in range(3)] + [torch.full((F, N), -5, dtype=torch.int8, device=dev)]
        ops.stitch(*dev_o, rolls, starts, src0=src0, length=length)
        for k in range(4):
            src = o3[k] if k < 3 else want_arg
            want = np.full((F, N), 7.0, np.float32) if k < 3 else np.full((F, N), -5, np.int8)
            for c, i in enumerate(starts):
                want[i:i + length] = src[c][src0:src0 + length]                      # model/amt.py transcript / transcript_stride
            got = rolls[k].cpu().numpy()
            assert got.dtype == want.dtype
            np.testing.assert_array_equal(got, want, err_msg='roll %d, len %d, src0 %d' % (k, length, src0))


@pytest.fixture(scope='module')
def trained(dev):
    from corpus import synth_audio as SA
    from model.amt import AMT
    amt = AMT(SA.default_config(), os.path.join(util.ROOT, 'tests', 'golden', 'config5_tiny_trained.pkl'), batch_size=2)
    notes = SA.pluck_notes(1234, 5.0)
    wave = SA.pluck_wave(notes, 5.0)
    feat_dev = amt.wave2feature(wave.unsqueeze(0), SA.SR, on_device=True)
    assert feat_dev.is_cuda
    feat = amt.wave2feature(wave.unsqueeze(0), SA.SR)
    assert not feat.is_cuda and torch.equal(feat_dev.cpu(), feat)                    # the keyword only skips the copy
    return amt, feat.numpy(), feat_dev


def test_end_to_end_equals_the_host_path(dev, trained):
    amt, feat, feat_dev = trained
    T = amt.config['input']['num_frame']
    assert -(-feat.shape[0] // T) % amt.batch_size != 0                              # a short last batch
    before = amt.transcript(feat)
    host_b = amt.mpe2note(*before[4:8])
    host_a = amt.mpe2note(*before[0:4])
    assert len(host_b) > 0 and len(host_a) > 0                                       # trained weights: there is something to compare
    assert amt.transcript_notes(feat) == host_b
    assert amt.transcript_notes(feat, output='A') == host_a
    assert amt.transcript_notes(feat_dev) == host_b                                  # a_feature as the device tensor
    kw = dict(thred_onset=0.4, thred_offset=0.3, thred_mpe=0.45, mode_velocity='org', mode_offset='longer')
    assert amt.transcript_notes(feat_dev, **kw) == amt.mpe2note(*before[4:8], **kw)
    n_off = T // 4
    stride = amt.transcript_stride(feat, n_off)
    host_s = amt.mpe2note(*stride[4:8])
    assert len(host_s) > 0
    assert amt.transcript_notes(feat, n_offset=n_off) == host_s
    assert amt.transcript_notes(feat_dev, n_offset=n_off, output='A') == amt.mpe2note(*stride[0:4])
    # the new path disturbs nothing: the host path gives what it gave before
    after = amt.transcript(feat)
    for a, b in zip(before, after):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert amt.mpe2note(*after[4:8]) == host_b
