"""Modal synthesis on the device: hftt_clip_synth, ops.clip_synth / VoiceBank, corpus.synth_audio.render_file and training.dataset.SynthClipStore.
What the bound allows, and which criterion catches which defect, is shown on the CPU by tests/test_synth_emul_bound.py on the same inputs.

Tiling: the kernel's tiles are 2,048 samples; width 16 at hop 256 shows (4 + 16 - 1) * 256 + 1,024 = 5,888 samples = two full tiles and one of 1,792
(lead 3: three full tiles and 512).  Inputs (tests/synth_emul.py): N = 5 tables at H = 1, 3, 32 and lead 0 / 3, one N = 88 table; files with 0
notes, 1 note, 300 records sounding inside one tile (a filter pass holds 256), a note across a tile border, an onset 10 s in front of the
window, a note cut by the file's end, windows before and behind a file, a bad file index, voices out of range.

  values   every written sample within the bound of synth_emul.py of the fp64 value of the header's formula; a sample where nothing sounds
           is 0; the row is untouched outside [0, e_b - o_b) and the arena around the rows intact; the three tables are the formulas'
  equal    overlapping windows, lead 0 against 3, and two voices with identical rows: bit for bit; the cancelling pair (table order)
  log-mel  hftt_clip_logmel over the scratch == over render_file's whole files as a float32 WaveTable, fill columns included; with
           lead = ceil(L / hop), clip_room over the scratch + clip_logmel == clip_logmel(room=) over the whole files
  store    SynthClipStore at the real clip width 192: labels == NoteClipStore's, spec == the composition fed the store's draws, the
           same seed gives the same batches, an augment that warps or mixes raises

Largest error / bound seen on an MI355X: 0.381 at H = 1 (one term per record: nothing averages out), 0.186 at H = 3 (lead 0 and 3 alike), 0.059 at
H = 32, 0.109 on the N = 88 table -- against 0.381, 0.130, 0.059, 0.099 of the fp32 numpy chain with correctly rounded S and E in the CPU test;
profiles/clip_synth_mi355x.txt, DESIGN.md section 10."""
import ctypes as C

import numpy as np
import pytest
import torch

import synth_emul as S

pytestmark = pytest.mark.gpu
GUARD = 7
FILL = -18.420681


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@pytest.fixture(scope='module')
def lm(dev):
    from hftt_hip import ops
    return ops.LogMel(dev, n_mels=8)


def _upload(table, bank, dev):
    from hftt_hip import ops
    return ops.LabelsTable(table, dev), ops.VoiceBank(device=dev, **bank)


def _synth(tab, vb, nsamp, windows, lead=0, width=S.WIDTH):
    """hftt_clip_synth through the C ABI with `out` inside a NaN arena -> (the pseudo-files' samples per window, the emulator's tables, which the
    kernel's must equal)"""
    from hftt_hip import _capi
    dev = tab.device
    n = len(windows)
    span = S.span_of(width, lead)
    arena = torch.full((n * span + 2 * GUARD,), float('nan'), device=dev)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    wf, ws, vi = i32([f for f, _, _ in windows]), i32([s for _, s, _ in windows]), i32([v for _, _, v in windows])
    fn = torch.tensor(list(nsamp), dtype=torch.int64, device=dev)
    samp0 = torch.full((2 * n + 1,), -7, dtype=torch.int64, device=dev)
    ofile, ostart = i32([-7] * n), i32([-7] * n)
    d = _capi.ClipSynthDesc()
    d.notes, d.row_ptr, d.file_nsamp = tab.notes.data_ptr() if tab.n_notes else None, tab.row_ptr.data_ptr(), fn.data_ptr()
    d.win_file, d.win_start, d.voice_index = wf.data_ptr(), ws.data_ptr(), vi.data_ptr()
    d.n_files, d.n_notes, d.B, d.width, d.N = tab.n_files, tab.n_notes, n, width, tab.N
    d.n_fft, d.hop, d.lead, d.sr, d.V, d.H = S.NFFT, S.HOP, lead, S.SR, vb.V, vb.H
    d.inc, d.amp, d.dec, d.vel_gain, d.rel = (t.data_ptr() for t in (vb.inc, vb.amp, vb.dec, vb.vel_gain, vb.rel))
    d.attack, d.release, d.span = vb.attack.data_ptr(), vb.release.data_ptr(), span
    d.out, d.out_samp0, d.out_win_file, d.out_win_start = arena[GUARD:].data_ptr(), samp0.data_ptr(), ofile.data_ptr(), ostart.data_ptr()
    _capi.check(_capi.lib().hftt_clip_synth(C.byref(d), torch.cuda.current_stream(dev).cuda_stream), 'clip_synth')
    torch.cuda.synchronize(dev)
    a = arena.cpu().numpy()
    assert np.isnan(a[:GUARD]).all() and np.isnan(a[GUARD + n * span:]).all(), 'the arena around the scratch was written'
    rows = a[GUARD:GUARD + n * span].reshape(n, span)
    n_prime = [nsamp[f] if 0 <= f < len(nsamp) and 0 <= v < vb.V else -1 for f, _, v in windows]
    t = S.pseudo_tables(n_prime, [s for _, s, _ in windows], width=width, lead=lead)
    assert np.array_equal(samp0.cpu().numpy(), t['samp0']) and np.array_equal(ofile.cpu().numpy(), t['win_file']) and np.array_equal(ostart.cpu().numpy(), t['win_start'])
    out = []
    for b in range(n):
        m = int(t['e'][b] - t['o'][b])
        assert not np.isnan(rows[b, :m]).any(), 'a sample of pseudo-file %d was not written' % (2 * b)
        assert np.isnan(rows[b, m:]).all(), 'the remainder of row %d was written' % b
        out.append(rows[b, :m].copy())
    return out, t


@pytest.mark.parametrize('name', sorted(S.cases()))
def test_values_against_fp64(dev, name):
    table, bank, t_ref, rows = S.reference(name)
    _, _, _, nsamp, windows, lead = S.cases()[name]
    tab, vb = _upload(table, bank, dev)
    got, t = _synth(tab, vb, nsamp, windows, lead)
    assert all(np.array_equal(t[k], t_ref[k]) for k in t)
    worst, seen, silent_seen = 0.0, 0, 0
    for b in range(len(windows)):
        if rows[b] is None:
            assert len(got[b]) == 0
            continue
        ref, bound, terms = rows[b]
        silent = terms == 0
        assert (_bits(got[b][silent]) == 0).all(), (name, b, 'a sample where nothing sounds is not +0')
        err = np.abs(got[b].astype(np.float64) - ref)
        if (~silent).any():
            ratio = float((err[~silent] / bound[~silent]).max())
            worst = max(worst, ratio)
        seen += int((~silent).sum())
        silent_seen += int(silent.sum())
    print('%s: largest error / bound %.3g over %d sounding samples (%d silent)' % (name, worst, seen, silent_seen))
    assert worst <= 1.0, (name, worst)
    assert seen > 5000 and silent_seen > 0


def test_overlapping_windows_a_lead_and_identical_voices_give_the_same_samples(dev):
    table, bank, _, _ = S.reference('N5-H3-lead0')
    bank = {k: v.copy() for k, v in bank.items()}
    for k in bank:
        bank[k][2] = bank[k][0]                                                  # voice 2: the rows of voice 0
    tab, vb = _upload(table, bank, dev)
    nsamp = S.FILE_NSAMP5
    # file 3 from frames 644 and 647 (three frames later: another tile origin for every sample), file 2's crowd from 4 and 9, under voices 0, 0, 2
    wins = ((3, 644, 0), (3, 647, 0), (3, 644, 2), (2, 4, 0), (2, 9, 0), (2, 9, 2))
    got, t = _synth(tab, vb, nsamp, wins)
    led, tl = _synth(tab, vb, nsamp, wins, lead=3)
    common = 0
    for a, b in ((0, 1), (3, 4)):
        lo, hi = max(t['o'][a], t['o'][b]), min(t['e'][a], t['e'][b])
        assert hi - lo > 2 * S.TILE
        assert np.array_equal(_bits(got[a][lo - t['o'][a]:hi - t['o'][a]]), _bits(got[b][lo - t['o'][b]:hi - t['o'][b]])), (a, b)
        common += int(hi - lo)
    for a, b in ((0, 2), (4, 5)):
        assert np.array_equal(_bits(got[a]), _bits(got[b])) and bool(got[a].any()), (a, b)
    for b in range(len(wins)):                                                   # lead 3 starts 768 samples earlier (or at the file's start) and ends alike
        assert tl['e'][b] == t['e'][b] and tl['o'][b] == max(0, t['o'][b] - 3 * S.HOP)
        assert np.array_equal(_bits(led[b][t['o'][b] - tl['o'][b]:]), _bits(got[b])), b
    assert common > 8000


def test_table_order_the_cancelling_pair_leaves_the_quiet_note_to_the_bit(dev):
    from hftt_hip.ops import labels_table_host
    bank, notes, nsamp = S.cancel_case()
    tab, vb = _upload(labels_table_host(notes, S.config(3)), bank, dev)
    got, t = _synth(tab, vb, nsamp, ((0, 0, 0), (1, 0, 0)), width=24)
    assert t['e'].tolist() == [6000, 6000] and np.array_equal(_bits(got[0]), _bits(got[1])) and bool(got[1].any())


VOICE_OF_FILE = (2, 1, 2, 0, 0)


@pytest.fixture(scope='module')
def whole(dev):
    """(note table, bank, the whole synthetic files of the N = 5 corpus under VOICE_OF_FILE as a float32 WaveTable): rendered once by
    render_file, shared by the two tests below"""
    from corpus import synth_audio as SA
    from hftt_hip import ops
    table, bank, _, _ = S.reference('N5-H3-lead0')
    tab, vb = _upload(table, bank, dev)
    files = [SA.render_file(tab, vb, f, VOICE_OF_FILE[f], n, hop=S.HOP) for f, n in enumerate(S.FILE_NSAMP5)]
    assert [int(x.numel()) for x in files] == list(S.FILE_NSAMP5) and all(bool(torch.isfinite(x).all()) for x in files)
    return tab, vb, ops.WaveTable([x.cpu() for x in files], dev, 'float32')


def _windows():
    files, starts = [f for f, _, _ in S.WINDOWS5], [s for _, s, _ in S.WINDOWS5]
    voices = [VOICE_OF_FILE[f] if 0 <= f < 5 else 0 for f in files]
    return files, starts, voices


def test_clip_logmel_over_the_scratch_is_clip_logmel_over_the_whole_files(dev, whole, lm):
    from hftt_hip import ops
    tab, vb, waves = whole
    files, starts, voices = _windows()
    want = ops.clip_logmel(waves, lm, files, starts, S.WIDTH, FILL)
    nsamp = torch.tensor(S.FILE_NSAMP5, dtype=torch.int64, device=dev)
    out, samp0, ofile, ostart = ops.clip_synth(tab, nsamp, vb, voices, files, starts, S.WIDTH, S.HOP, S.SR)
    got = ops.clip_logmel(ops.WetTable(out, samp0), lm, ofile, ostart, S.WIDTH, FILL)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    fill = (want == FILL).all(dim=1).sum(dim=1).tolist()
    assert fill[0] == 3 and fill[5] == S.WIDTH and fill[6] == S.WIDTH and fill[8] == S.WIDTH and fill[9] == S.WIDTH and 0 < fill[4] < S.WIDTH
    assert out.shape == (len(files), S.span_of()) and bool((want != FILL).any())


def test_a_room_over_the_scratch_is_the_room_over_the_whole_files(dev, whole, lm):
    from hftt_hip import ops
    tab, vb, waves = whole
    files, starts, voices = _windows()
    L = 700
    r = np.random.RandomState(9)
    ir = (r.standard_normal((2, L)) * np.exp(-np.arange(L) / 150.0)).astype(np.float32)
    room = ops.RoomBank(ir, dev, taps=[L, 300])
    index = torch.tensor([b % 3 - 1 for b in range(len(files))], dtype=torch.int32, device=dev)           # dry, response 0, response 1
    want = ops.clip_logmel(waves, lm, files, starts, S.WIDTH, FILL, room=(room, index))
    lead = -(-L // S.HOP)
    nsamp = torch.tensor(S.FILE_NSAMP5, dtype=torch.int64, device=dev)
    out, samp0, ofile, ostart = ops.clip_synth(tab, nsamp, vb, voices, files, starts, S.WIDTH, S.HOP, S.SR, lead=lead)
    wet, wsamp0, wfile, wstart = ops.clip_room(ops.WetTable(out, samp0), ofile, ostart, S.WIDTH, room, index, S.HOP)
    got = ops.clip_logmel(ops.WetTable(wet, wsamp0), lm, wfile, wstart, S.WIDTH, FILL)
    assert lead == 3 and torch.equal(got.view(torch.int32), want.view(torch.int32)) and bool((want != FILL).any())


def test_store_end_to_end_at_the_real_clip_width(dev):
    from corpus import synth_audio as SA
    from corpus.make_dataset import assemble_note_store, assemble_synth_store
    from hftt_hip import HfttError, ops
    from training.dataset import NoteClipStore, SynthClipStore, WaveAugment
    config = SA.default_config()
    config['input']['max_value'] = 0.0
    cin = config['input']
    width = cin['margin_b'] + cin['num_frame'] + cin['margin_f']
    assert width == 192
    notes = [SA.pluck_notes(7, dur=5.0), [], SA.pluck_notes(8, dur=4.0)]
    bank = SA.synth_voice_bank(4, config, seed=1, partials=16)
    vb = ops.VoiceBank(device=dev, **bank)
    store = assemble_synth_store(notes, config, release_samples=int(bank['release'].max()))
    nf = np.bincount(store['clip_file'], minlength=3)
    note_store = NoteClipStore(assemble_note_store([np.zeros((n, config['feature']['mel_bins']), np.float32) for n in nf], notes, config), config, dev)
    synth = SynthClipStore(store, config, dev, vb, seed=3)
    assert len(synth) == len(note_store) == int(nf.sum()) and synth.resident_bytes() == vb.nbytes() + synth.table.nbytes() + 8 * 3 + 8 * len(synth)
    ids = [0, 5, int(nf[0]) - 1, int(nf[0]), int(nf[0]) + int(nf[1]) + 40, len(synth) - 1]
    got, labels = synth.batch(ids), note_store.batch(ids)
    for k in range(1, 5):
        assert np.array_equal(got[k].cpu().numpy(), labels[k].cpu().numpy()), k
    assert bool(got[1].any())
    # spec: the composition fed the store's own draws
    twin = SynthClipStore(store, config, dev, vb, seed=3)
    voice = twin.draw_voice(len(ids))
    file, frame = synth.clip_file[torch.tensor(ids, device=dev)], synth.clip_frame[torch.tensor(ids, device=dev)]
    out, samp0, ofile, ostart = ops.clip_synth(synth.table, synth.file_nsamp, vb, voice, file, frame - cin['margin_b'], width, 256, 16000.0)
    want = ops.clip_logmel(ops.WetTable(out, samp0), synth.logmel, ofile, ostart, width, synth.fill)
    assert torch.equal(got[0], want) and got[0].shape == (len(ids), 256, 192) and bool(torch.isfinite(got[0]).all())
    assert len(set(voice.tolist())) > 1 and bool((got[0] != synth.fill).any())
    # the same seed gives the same batches, another seed other voices
    a, b, c = SynthClipStore(store, config, dev, vb, seed=3), SynthClipStore(store, config, dev, vb, seed=3), SynthClipStore(store, config, dev, vb, seed=4)
    for _ in range(2):
        x, y, z = a.batch(ids), b.batch(ids), c.batch(ids)
        assert all(torch.equal(p, q) for p, q in zip(x, y)) and all(torch.equal(p, q) for p, q in zip(x[1:], z[1:]))
    assert not torch.equal(x[0], z[0])
    # gain, noise and a room: the labels stay, the batch is reproducible
    ir, taps = SA.synth_room_bank(3, 16000, taps=1024, rt60=(0.05, 0.2), seed=2)
    kw = dict(gain_db=(-3.0, 3.0), noise_dbfs=(-70.0, -60.0), room_p=0.7, room_bank=ops.RoomBank(ir, dev, taps=taps), seed=5)
    r1, r2 = (SynthClipStore(store, config, dev, vb, seed=3, augment=WaveAugment(**kw)) for _ in range(2))
    assert r1.lead == 4
    x, y = r1.batch(ids), r2.batch(ids)
    assert all(torch.equal(p, q) for p, q in zip(x, y)) and all(torch.equal(p, q) for p, q in zip(x[1:], got[1:])) and not torch.equal(x[0], got[0])
    assert bool(torch.isfinite(x[0]).all())
    for bad in (dict(pitch_semitones=(-2, 2)), dict(detune_cents=10.0), dict(shift=True), dict(mix_p=0.5)):
        with pytest.raises(HfttError, match='warps or mixes'):
            SynthClipStore(store, config, dev, vb, augment=WaveAugment(**bad))
