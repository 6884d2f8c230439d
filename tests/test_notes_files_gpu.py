"""A file list in one pass (csrc/notes.hip: hftt_clip_windows, hftt_notes_decode_seg; AMT.transcript_notes_files) against what it restates:
numpy window slicing with per-window padding, AMT.mpe2note on every file's rows alone, and the per-file AMT.transcript_notes.  Everything is
compared with == (doubles included) or torch.equal."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import util

pytestmark = pytest.mark.gpu

HOP = 256 / 16000
MODES = [(mv, mo) for mv in ('ignore_zero', 'org') for mo in ('shorter', 'longer', 'offset')]
THR = dict(thred_onset=0.6, thred_offset=0.55, thred_mpe=0.5)
SENTINEL = -8192.0


def _chunk():
    from hftt_hip import _capi
    return _capi.NOTES_CHUNK


# ----------------------------------------------------------------------------------------------------------------------------------------
# hftt_clip_windows
# ----------------------------------------------------------------------------------------------------------------------------------------
def _raw_clip(dev, feat, row0, win_file, win_start, width, fill, guard=3):
    """hftt_clip_windows through the C ABI with `out` inside an arena, `guard` sentinel rows of `width` on either side; returns (out, arena)"""
    from hftt_hip import _capi
    R, n_bins = feat.shape
    B = len(win_file)
    n = B * n_bins * width
    arena = torch.full((2 * guard * width + n,), SENTINEL, dtype=torch.float32, device=dev)
    f = torch.from_numpy(np.ascontiguousarray(feat)).to(dev) if R else torch.zeros(1, n_bins, device=dev)
    t = [torch.tensor(list(x), dtype=torch.int32, device=dev) for x in (row0, win_file, win_start)]
    d = _capi.ClipWindowsDesc()
    d.feature, d.file_row0, d.win_file, d.win_start = f.data_ptr(), t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr()
    d.B, d.width, d.n_bins, d.n_files, d.R, d.fill = B, width, n_bins, len(row0) - 1, R, fill
    d.out = arena.data_ptr() + 4 * guard * width
    _capi.check(_capi.lib().hftt_clip_windows(C.byref(d), torch.cuda.current_stream(dev).cuda_stream), 'clip_windows')
    torch.cuda.synchronize(dev)
    a = arena.cpu()
    return a[guard * width:guard * width + n].reshape(B, n_bins, width), a


def _want_windows(feat, row0, win_file, win_start, width, fill):
    """out[b, k, t] = feature[row0[f] + s + t, k] inside the file, fill outside; a file index outside 0 .. n_files: all fill"""
    n_bins = feat.shape[1]
    out = np.full((len(win_file), n_bins, width), fill, np.float32)
    for b, (f, s) in enumerate(zip(win_file, win_start)):
        if not 0 <= f < len(row0) - 1:
            continue
        n = row0[f + 1] - row0[f]
        for t in range(width):
            if 0 <= s + t < n:
                out[b, :, t] = feat[row0[f] + s + t]
    return out


def _check_clip(dev, feat, row0, win_file, win_start, width, fill, guard=3):
    got, arena = _raw_clip(dev, feat, row0, win_file, win_start, width, fill, guard)
    want = torch.from_numpy(_want_windows(feat, row0, win_file, win_start, width, fill))
    assert not torch.isnan(got).any(), 'a frame of another file shows'
    assert torch.equal(got, want)
    side = torch.full((guard * width,), SENTINEL)
    assert torch.equal(arena[:guard * width], side) and torch.equal(arena[-guard * width:], side)      # bit-exact sentinels on both sides


@pytest.mark.parametrize('width', [1, 3, 63, 192])
@pytest.mark.parametrize('n_bins', [1, 5, 64, 65, 256])
def test_clip_windows(dev, n_bins, width):
    fill = np.float32(-18.420681)
    lens = [0, 1, 2, width - 1, width, width + 1, 2 * width + 3]
    row0 = [0] + list(np.cumsum(lens))
    n_files = len(lens)
    r = np.random.RandomState(1000 * n_bins + width)
    feat = r.randn(row0[-1], n_bins).astype(np.float32)
    for f, n in enumerate(lens):
        starts = [-width, -width + 1, -1, 0, n - 1, n]
        if n + 2 <= width:
            starts.append(-(width - n) // 2)                 # a window longer than its file: fill on both sides
        mine = feat.copy()
        mine[:row0[f]] = np.nan                                # every other file's rows are NaN: one leaked frame shows
        mine[row0[f + 1]:] = np.nan
        _check_clip(dev, mine, row0, [f] * len(starts), starts, width, fill)
    # file indices outside 0 .. n_files: all fill, whatever the features hold
    _check_clip(dev, np.full_like(feat, np.nan), row0, [-1, n_files, -1, n_files], [0, 0, -width + 1, 5], width, fill)
    # B = 1, and B = 67 over all files at once (more than one tile row of windows; finite features, checked against the construction)
    wf = [6]
    ws = [3]
    mine = feat.copy()
    mine[:row0[6]] = np.nan
    _check_clip(dev, mine, row0, wf, ws, width, fill)
    wf = [(3 * i) % n_files for i in range(67)]
    ws = [(-width + 7 * i) % (3 * width + 4) - width for i in range(67)]
    _check_clip(dev, feat, row0, wf, ws, width, fill)
    # the wrapper: the same windows as a device tensor
    from hftt_hip import ops
    out = ops.clip_windows(torch.from_numpy(feat).to(dev), row0, wf, ws, width, float(fill))
    assert out.shape == (67, n_bins, width) and torch.equal(out.cpu(), torch.from_numpy(_want_windows(feat, row0, wf, ws, width, fill)))


# ----------------------------------------------------------------------------------------------------------------------------------------
# hftt_notes_decode_seg
# ----------------------------------------------------------------------------------------------------------------------------------------
def _amt(N, note_min=21):
    from model.amt import AMT
    return AMT({'feature': {'sr': 16000, 'hop_sample': 256}, 'midi': {'note_min': note_min, 'num_note': N}}, None)


def _sorted_notes(pitch, velocity, onset, offset):
    assert pitch.dtype == np.int32 and velocity.dtype == np.int32 and onset.dtype == np.float64 and offset.dtype == np.float64
    assert (np.diff(pitch) >= 0).all()                       # in front of the sort: pitch-major
    order = np.lexsort((pitch, onset))
    return [{'pitch': int(pitch[i]), 'onset': float(onset[i]), 'offset': float(offset[i]), 'velocity': int(velocity[i])} for i in order]


def _to_dev(dev, arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrs]


def _seg_notes(dev, tracks, rows, **kw):
    """ops.notes_decode_seg -> one sorted list per segment, and seg_notes"""
    from hftt_hip import ops
    pitch, velocity, onset, offset, seg = (x.cpu().numpy() for x in ops.notes_decode_seg(*_to_dev(dev, tracks), rows, HOP, **kw))
    assert seg.dtype == np.int32 and len(seg) == len(rows) and seg[0] == 0 and seg[-1] == len(pitch)
    return [_sorted_notes(*(a[seg[s]:seg[s + 1]] for a in (pitch, velocity, onset, offset))) for s in range(len(rows) - 1)], seg


def _same_seg(dev, tracks, rows, modes=MODES, witness=True):
    """every segment == AMT.mpe2note on its rows alone (and == ops.notes_decode on them), exactly; returns the number of notes compared"""
    from hftt_hip import ops
    amt = _amt(tracks[0].shape[1])
    total = 0
    for mv, mo in modes:
        kw = dict(THR, mode_velocity=mv, mode_offset=mo)
        got, seg = _seg_notes(dev, tracks, rows, **kw)
        counts = []
        for s in range(len(rows) - 1):
            sl = [a[rows[s]:rows[s + 1]] for a in tracks]
            host = amt.mpe2note(a_onset=sl[0], a_offset=sl[1], a_mpe=sl[2], a_velocity=sl[3], **kw)
            assert len(got[s]) == len(host), (mv, mo, s, len(got[s]), len(host))
            for a, b in zip(got[s], host):
                assert a == b, (mv, mo, s, a, b)             # pitch, velocity ints; onset, offset doubles compared with ==
            if witness:
                one = _sorted_notes(*(x.cpu().numpy() for x in ops.notes_decode(*_to_dev(dev, sl), HOP, **kw)))
                assert one == got[s], (mv, mo, s)
            counts.append(len(host))
        assert list(seg) == [0] + list(np.cumsum(counts)), (mv, mo)        # the running sum of the per-slice counts
        total += sum(counts)
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


def test_random_tracks_in_segments_of_every_length(dev):
    ch = _chunk()
    lens = [0, 1, 2, 3, 7, 64, ch - 1, ch, ch + 1, 2 * ch + 1, 0, 1]
    rows = [0] + [int(x) for x in np.cumsum(lens)]
    total = 0
    for N in (1, 8, 88):
        for seed in range(3):
            tracks = _tracks(1000 * seed + 7 * rows[-1] + N, rows[-1], N)
            total += _same_seg(dev, tracks, rows, modes=MODES if seed == 0 else [MODES[(seed + N) % 6]], witness=seed == 0)
    assert total > 1000


def _scene(F, N=4):
    on = np.full((F, N), 0.1, np.float32)
    off = np.full((F, N), 0.1, np.float32)
    mpe = np.full((F, N), 0.9, np.float32)
    vel = np.full((F, N), 64, np.int8)
    return [on, off, mpe, vel]


def _border_scenes():
    """segments of chunk + 3 and 5 frames; name -> (tracks, notes in segment 0, notes in segment 1)"""
    ch = _chunk()
    r1 = ch + 3
    F = r1 + 5
    a = _scene(F)
    a[0][:] = 0.7                                            # a constant onset track: every frame of every pitch is an onset, in both segments
    b = _scene(F)
    b[0][r1 - 1, 2] = 0.9                                    # an onset peak at the last frame of segment 0 ...
    b[1][r1, 2] = 0.9; b[2][r1, 2] = 0.1                     # ... segment 1 opens with an offset peak and an mpe below the threshold
    c = _scene(F)
    c[0][r1 - 2:r1, 1] = 0.8                                 # a plateau that ends segment 0 ...
    c[0][r1:r1 + 2, 1] = 0.9                                 # ... and a higher one that opens segment 1
    return r1, F, {'a': (a, 4 * r1, 20), 'b': (b, 1, 0), 'c': (c, 2, 2)}


@pytest.mark.parametrize('name', ['a', 'b', 'c'])
def test_nothing_is_looked_up_across_a_border(dev, name):
    r1, F, scenes = _border_scenes()
    tracks, n0, n1 = scenes[name]
    amt = _amt(4)
    # on the host first: the slices hold the expected counts, and the concatenation decoded as ONE file differs already inside segment 0
    # (a: the last frame's offset is the next frame's onset instead of (F_s - 1) * hop; b: offset 4.144 at the peak behind the border
    # instead of 4.128; c: the 0.8 run is no peak in front of 0.9) -- a decoder that ignores the borders cannot pass
    host0 = amt.mpe2note(*(t[:r1] for t in tracks), **THR)
    host1 = amt.mpe2note(*(t[r1:] for t in tracks), **THR)
    assert (len(host0), len(host1)) == (n0, n1)
    whole = amt.mpe2note(*tracks, **THR)
    assert [n for n in whole if n['onset'] < (r1 - 0.5) * HOP] != host0
    if name == 'b':
        assert host0[0]['offset'] == (r1 - 1) * HOP and whole[0]['offset'] == r1 * HOP              # 4.128 and 4.144 at chunk = 256
    assert _same_seg(dev, tracks, [0, r1, F]) == 6 * (n0 + n1)
    # empty segments in front, between and behind change nothing
    got, seg = _seg_notes(dev, tracks, [0, 0, r1, r1, F, F], **THR)
    assert got == [[], host0, [], host1, []] and list(seg) == [0, 0, n0, n0, n0 + n1, n0 + n1]
    # the three frames around the border as three segments of one frame each
    three = [np.ascontiguousarray(t[r1 - 2:r1 + 1]) for t in tracks]
    _same_seg(dev, three, [0, 1, 2, 3])


def test_no_segment_and_no_row(dev):
    from hftt_hip import ops
    e = [torch.zeros(0, 88, device=dev)] * 3 + [torch.zeros(0, 88, dtype=torch.int8, device=dev)]
    for rows in ([0], [0, 0], [0, 0, 0, 0]):
        *arrs, seg = ops.notes_decode_seg(*e, rows, HOP, host=True)
        assert all(len(x) == 0 for x in arrs) and seg.tolist() == [0] * len(rows)


def _raw_seg(dev, tracks, rows, cap, guard=64):
    """hftt_notes_decode_seg through the C ABI with caller-owned outputs of cap + guard records, the guard pre-filled with a sentinel"""
    from hftt_hip import _capi
    t = _to_dev(dev, tracks)
    F, N = tracks[0].shape
    n_seg = len(rows) - 1
    L = _capi.lib()
    ws = torch.empty(L.hftt_notes_seg_ws_bytes(F, N, n_seg), dtype=torch.int8, device=dev)
    pitch = torch.full((cap + guard,), -77, dtype=torch.int32, device=dev)
    velocity = torch.full((cap + guard,), -78, dtype=torch.int32, device=dev)
    onset = torch.full((cap + guard,), -79.0, dtype=torch.float64, device=dev)
    offset = torch.full((cap + guard,), -80.0, dtype=torch.float64, device=dev)
    total = torch.full((1,), -1, dtype=torch.int32, device=dev)
    seg = torch.full((n_seg + 1 + guard,), -81, dtype=torch.int32, device=dev)
    rows_dev = torch.tensor(rows, dtype=torch.int32, device=dev)
    s = _capi.NotesSegDesc()
    d = s.notes
    d.F, d.N, d.note_min, d.cap, d.hop_sec = F, N, 21, cap, HOP
    d.onset, d.offset, d.mpe, d.velocity = (x.data_ptr() for x in t)
    d.thred_onset, d.thred_offset, d.thred_mpe = 0.6, 0.55, 0.5
    d.out_pitch, d.out_velocity, d.out_onset, d.out_offset, d.n_notes = pitch.data_ptr(), velocity.data_ptr(), onset.data_ptr(), offset.data_ptr(), total.data_ptr()
    d.ws, d.ws_bytes = ws.data_ptr(), ws.numel()
    host_rows = (C.c_int32 * (n_seg + 1))(*rows)
    s.n_seg, s.seg_row0_host, s.seg_row0, s.seg_notes = n_seg, host_rows, rows_dev.data_ptr(), seg.data_ptr()
    _capi.check(L.hftt_notes_decode_seg(C.byref(s), torch.cuda.current_stream(dev).cuda_stream), 'notes_decode_seg')
    torch.cuda.synchronize(dev)
    return int(total.item()), seg.cpu().numpy(), [x.cpu().numpy() for x in (pitch, velocity, onset, offset)]


def test_capacity(dev):
    from hftt_hip import HfttError, ops
    ch = _chunk()
    rows = [0, 7, ch + 8, ch + 8, 2 * ch + 30]
    tracks = _tracks(5, rows[-1], 8)
    amt = _amt(8)
    counts = [len(amt.mpe2note(*(t[rows[s]:rows[s + 1]] for t in tracks), **THR)) for s in range(4)]
    n_ref = sum(counts)
    assert n_ref > 40 and counts[1] > 0 and counts[3] > 0
    want_seg = [0] + list(np.cumsum(counts))
    full = _raw_seg(dev, tracks, rows, n_ref)
    assert full[0] == n_ref and list(full[1][:5]) == want_seg and (full[1][5:] == -81).all()
    for a, sentinel in zip(full[2], (-77, -78, -79.0, -80.0)):
        assert (a[n_ref:] == sentinel).all() and (a[:n_ref] != sentinel).all()
    for cap in (0, 1, counts[0] + 1, n_ref // 2, n_ref - 1):
        total, seg, arrs = _raw_seg(dev, tracks, rows, cap)
        assert total == n_ref and list(seg[:5]) == want_seg and (seg[5:] == -81).all()      # what exists, not what fits
        for a, b, sentinel in zip(arrs, full[2], (-77, -78, -79.0, -80.0)):
            np.testing.assert_array_equal(a[:cap], b[:cap])                                 # the first cap records of the uncapped run
            assert (a[cap:] == sentinel).all()                                              # nothing behind cap
    t = _to_dev(dev, tracks)
    with pytest.raises(HfttError, match='capacity'):
        ops.notes_decode_seg(*t, rows, HOP, capacity=n_ref - 1, **THR)
    assert len(ops.notes_decode_seg(*t, rows, HOP, capacity=n_ref, **THR)[0]) == n_ref
    # without capacity= the wrapper runs once more with the exact count: more notes than the default room
    F, N = 4096, 2
    on2 = np.full((F, N), 0.7, np.float32); z = np.full((F, N), 0.1, np.float32); v2 = np.full((F, N), 5, np.int8)
    assert ops.notes_default_capacity(F, N) < N * F
    out = ops.notes_decode_seg(*_to_dev(dev, (on2, z, z + 0.8, v2)), [0, 1000, F], HOP, host=True, **THR)
    assert len(out[0]) == N * F and out[4].tolist() == [0, N * 1000, N * F] and not out[0].is_cuda


# ----------------------------------------------------------------------------------------------------------------------------------------
# AMT.transcript_notes_files
# ----------------------------------------------------------------------------------------------------------------------------------------
ARGS = [dict(), dict(n_offset='T//4'), dict(thred_onset=0.4, thred_offset=0.3, thred_mpe=0.45, mode_velocity='org', mode_offset='longer')]


def _args(kw, T):
    return {k: (T // 4 if v == 'T//4' else v) for k, v in kw.items()}


@pytest.fixture(scope='module')
def files(dev):
    """two transcribers over the same weights (batch_size 3 and 1) and six files: 5.0 s, 2.1 s, 0.3 s, the first T and T + 1 frames of the
    first, and an empty one; half numpy arrays, half device tensors -- 3 + 2 + 1 + 1 + 2 + 0 = 9 clips"""
    from corpus import synth_audio as SA
    from model.amt import AMT
    path = os.path.join(util.ROOT, 'tests', 'golden', 'config5_tiny_trained.pkl')
    amt3, amt1 = AMT(SA.default_config(), path, batch_size=3), AMT(SA.default_config(), path, batch_size=1)
    T = amt3.config['input']['num_frame']
    feats = []
    for seed, dur, span in ((1234, 5.0, 5.0), (77, 2.1, 4.1), (5, 0.3, 2.3)):             # pluck_notes leaves its last 2 s without onsets
        wave = SA.pluck_wave([n for n in SA.pluck_notes(seed, span) if n['onset'] < dur], dur)
        feats.append(amt3.wave2feature(wave.unsqueeze(0), SA.SR).numpy())
    assert feats[0].shape == (313, 256)
    feats += [feats[0][:T].copy(), feats[0][:T + 1].copy(), np.zeros((0, 256), np.float32)]
    assert sum(-(-f.shape[0] // T) for f in feats) == 9
    mixed = [f if i % 2 == 0 else torch.from_numpy(f).to(dev) for i, f in enumerate(feats)]
    return amt3, amt1, feats, mixed, {}


def _host_packed(amt, feats, n_offset, bs):
    """the packed batches restated with numpy: per-file padding (amt.py:71-79 / :126-137), clips of all files in order, bs clips per model
    call across file borders, host stitching with .argmax(3) (amt.py:104-113 / :155-176); returns the 8 rolls of every file"""
    cin, cf, cm = amt.config['input'], amt.config['feature'], amt.config['midi']
    T, N = cin['num_frame'], cm['num_note']
    width = cin['margin_b'] + T + cin['margin_f']
    clips, rolls = [], []
    for f, a in enumerate(feats):
        n = a.shape[0]
        if n_offset is None:
            step, src0, front = T, 0, cin['margin_b']
            len_s = int(np.ceil(n / T) * T) - n
            back = len_s + cin['margin_f']
        else:
            step, src0, front = int(T / 2), n_offset, cin['margin_b'] + n_offset
            tmp_len = n + cin['margin_b'] + cin['margin_f'] + step
            len_s = int(np.ceil(tmp_len / step) * step) - tmp_len
            back = len_s + cin['margin_f'] + (step - n_offset)
        a_input = np.concatenate([np.full((front, cf['n_bins']), cin['min_value'], np.float32), a, np.full((back, cf['n_bins']), cin['min_value'], np.float32)])
        clips += [(f, i, a_input[i:i + width].T) for i in range(0, n, step)]
        rolls.append([np.zeros((n + len_s if n else 0, N), np.int8 if k % 4 == 3 else np.float32) for k in range(8)])
    for b0 in range(0, len(clips), bs):
        batch = clips[b0:b0 + bs]
        spec = torch.from_numpy(np.stack([c[2] for c in batch])).to(amt.device)
        with torch.no_grad():
            o = amt.model(spec)
        sel = [x.cpu().numpy() for x in (o[0], o[1], o[2], o[3].argmax(3), o[5], o[6], o[7], o[8].argmax(3))]
        for c, (f, i, _) in enumerate(batch):
            for k in range(8):
                rolls[f][k][i:i + step] = sel[k][c][src0:src0 + step]
    return rolls


def _reference(files, kw):
    """(notes_A, notes_B) per file from the restated packed batches at batch_size 3; the rolls are computed once per n_offset"""
    amt3, _, feats, _, cache = files
    n_offset = kw.get('n_offset')
    if n_offset not in cache:
        cache[n_offset] = _host_packed(amt3, feats, n_offset, 3)
    dec = {k: v for k, v in kw.items() if k != 'n_offset'}
    return [(amt3.mpe2note(*r[0:4], **dec), amt3.mpe2note(*r[4:8], **dec)) for r in cache[n_offset]]


@pytest.mark.parametrize('case', range(len(ARGS)))
def test_packed_batches_equal_the_host_path_at_equal_batches(dev, files, case):
    amt3, _, feats, mixed, _ = files
    kw = _args(ARGS[case], amt3.config['input']['num_frame'])
    ref = _reference(files, kw)
    assert sum(1 for a, b in ref if a) > 1 and sum(1 for a, b in ref if b) > 1          # more than one file has notes
    assert ref[5] == ([], [])
    assert amt3.transcript_notes_files(mixed, output='A', **kw) == [a for a, b in ref]
    assert amt3.transcript_notes_files(mixed, output='B', **kw) == [b for a, b in ref]
    assert amt3.transcript_notes_files(mixed, **kw) == [b for a, b in ref]
    assert amt3.transcript_notes_files(mixed, output='AB', **kw) == ref
    assert amt3.transcript_notes_files(feats, output='AB', **kw) == ref                 # all numpy: one block, no concatenation on the device


@pytest.mark.parametrize('case', range(len(ARGS)))
def test_one_clip_per_call_equals_the_per_file_method(dev, files, case):
    _, amt1, feats, mixed, _ = files
    kw = _args(ARGS[case], amt1.config['input']['num_frame'])
    loop = {o: [amt1.transcript_notes(f, output=o, **kw) for f in mixed] for o in 'AB'}
    assert sum(1 for x in loop['B'] if x) > 1
    for o in 'AB':
        assert amt1.transcript_notes_files(mixed, output=o, **kw) == loop[o]
    assert amt1.transcript_notes_files(mixed, output='AB', **kw) == list(zip(loop['A'], loop['B']))


def test_the_forward_is_independent_of_batch_composition_so_packing_equals_the_per_file_loop(dev, files):
    """The packed call puts clips of different files into one model call and fills the batches the per-file call leaves short.  That changes
    nothing only if the eval forward gives a clip the same outputs in any batch: held here bit for bit for the eight outputs, and with it
    the packed result at batch_size 3 equals the per-file loop at batch_size 3 (whose batches are 3, 2, 1, 1, 2 clips)."""
    from hftt_hip import ops
    amt3, _, feats, mixed, _ = files
    cin = amt3.config['input']
    T = cin['num_frame']
    lens = [f.shape[0] for f in feats]
    row0 = [0] + [int(x) for x in np.cumsum(lens)]
    feature = torch.from_numpy(np.concatenate(feats)).to(dev)
    wf = [f for f, n in enumerate(lens) for _ in range(0, n, T)]
    ws = [i - cin['margin_b'] for n in lens for i in range(0, n, T)]
    spec = ops.clip_windows(feature, row0, wf, ws, cin['margin_b'] + T + cin['margin_f'], cin['min_value'])
    assert spec.shape[0] == 9
    with torch.no_grad():
        o = amt3.model(spec)
        for c in range(9):
            one = amt3.model(spec[c:c + 1])
            for k in (0, 1, 2, 3, 5, 6, 7, 8):
                assert torch.equal(o[k][c], one[k][0]), (c, k, float((o[k][c] - one[k][0]).abs().max()))
    for case in range(len(ARGS)):
        kw = _args(ARGS[case], T)
        for out in 'AB':
            assert amt3.transcript_notes_files(mixed, output=out, **kw) == [amt3.transcript_notes(f, output=out, **kw) for f in mixed], (case, out)


def test_edge_lists_and_the_old_paths_are_undisturbed(dev, files):
    amt3, _, feats, mixed, _ = files
    before = amt3.transcript(feats[0])
    host_b = amt3.mpe2note(*before[4:8])
    single = amt3.transcript_notes(feats[0])
    assert single == host_b and len(host_b) > 0
    assert amt3.transcript_notes_files([]) == []
    assert amt3.transcript_notes_files([feats[5]]) == [[]]
    assert amt3.transcript_notes_files([feats[5], mixed[5]], output='AB') == [([], []), ([], [])]
    assert amt3.transcript_notes_files([feats[0]]) == [host_b]                          # one file: the batches are the per-file call's
    assert amt3.transcript_notes_files([mixed[1]]) == [amt3.transcript_notes(mixed[1])]
    amt3.transcript_notes_files(mixed, output='AB')
    # the new path disturbs nothing: the host path and the per-file call give what they gave before
    after = amt3.transcript(feats[0])
    for a, b in zip(before, after):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert amt3.mpe2note(*after[4:8]) == host_b and amt3.transcript_notes(feats[0]) == single
