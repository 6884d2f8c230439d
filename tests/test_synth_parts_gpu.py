"""The played clip synth on the device: hftt_clip_synth_parts, ops.clip_synth's play / tune / part, training.dataset.SynthPlay in SynthClipStore.
What the bound allows, and which criterion catches which defect, is shown on the CPU by tests/test_synth_parts_emul_bound.py on the same inputs
(tests/synth_parts_emul.py: hop 256, width 16, N = 5 at H = 1 and 3 and N = 88 at H = 3, six windows at the most).  Every launch writes into a NaN
arena: what the contract leaves unwritten stays NaN, and the guard in front of and behind the rows stays intact.

  identity   all groups NULL, and identity VALUES (shift 0, t_delay 0, t_scale 1, tune 2^31, part_file -1): all four outputs equal
             hftt_clip_synth's bit for bit -- the guard on the two copies of the walk (clip_synth.hip is pinned by tests/test_synth_capi.py)
  prepared   each option alone equals the OLD kernel on inputs prepared on the host: pitches moved in the table, times mapped in numpy fp64
             with two roundings, increments scaled by the integer formula, the partner's file rendered alone and cut to n'_A
  order      the cancelling duet: primary first, in table order
  combined   everything on, with a partner: every sample inside render64_parts' bound, silence +0
  equal      overlapping windows with equal draws: bit for bit
  store      labels == the numpy walker fed the store's own draws; spec == clip_logmel over ops.clip_synth for those draws, with and without
             a room; play=None: the batches of the composition as it was

Largest error / bound seen on an MI355X: see profiles/clip_synth_parts_mi355x.txt and DESIGN.md section 10."""
import ctypes as C

import numpy as np
import pytest
import torch

import mix_emul as M
import synth_emul as S
import synth_parts_emul as P

pytestmark = pytest.mark.gpu
GUARD = 7


def _upload(table, bank, dev):
    from hftt_hip import ops
    return ops.LabelsTable(table, dev), ops.VoiceBank(device=dev, **bank)


class _Run:
    """one launch into a NaN arena: rows int32 bits [B, span] (torch), the three tables (torch)"""

    def __init__(self, tab, vb, files, starts, voices, lead=0, width=S.WIDTH, file_nsamp=None, nsamp=None, play=None, part=None, part_nsamp=None, part_play=None):
        """file_nsamp given: hftt_clip_synth.  Otherwise hftt_clip_synth_parts with nsamp [B]; play / part_play: (shift, t_delay, t_scale, tune),
        each a list or None; part: (file, start, voice, gain) lists"""
        from hftt_hip import _capi
        dev = tab.device
        n = len(files)
        span = S.span_of(width, lead)
        arena = torch.full((n * span + 2 * GUARD,), float('nan'), device=dev)
        keep = []

        def t(v, dtype):
            if v is None:
                return None
            if dtype == 'u32':                                                  # (uint32 tunes travel as the int32 with the same bits)
                v, dtype = np.asarray(v, np.int64).astype(np.uint32).view(np.int32), torch.int32
            x = torch.as_tensor(np.asarray(v), device=dev).to(dtype).contiguous()
            keep.append(x)
            return x.data_ptr()
        samp0 = torch.full((2 * n + 1,), -7, dtype=torch.int64, device=dev)
        ofile, ostart = (torch.full((n,), -7, dtype=torch.int32, device=dev) for _ in range(2))
        d = _capi.ClipSynthDesc()
        d.notes, d.row_ptr, d.file_nsamp = tab.notes.data_ptr() if tab.n_notes else None, tab.row_ptr.data_ptr(), t(file_nsamp, torch.int64)
        d.win_file, d.win_start, d.voice_index = t(files, torch.int32), t(starts, torch.int32), t(voices, torch.int32)
        d.n_files, d.n_notes, d.B, d.width, d.N = tab.n_files, tab.n_notes, n, width, tab.N
        d.n_fft, d.hop, d.lead, d.sr, d.V, d.H = S.NFFT, S.HOP, lead, S.SR, vb.V, vb.H
        d.inc, d.amp, d.dec, d.vel_gain, d.rel = (x.data_ptr() for x in (vb.inc, vb.amp, vb.dec, vb.vel_gain, vb.rel))
        d.attack, d.release, d.span = vb.attack.data_ptr(), vb.release.data_ptr(), span
        d.out, d.out_samp0, d.out_win_file, d.out_win_start = arena[GUARD:].data_ptr(), samp0.data_ptr(), ofile.data_ptr(), ostart.data_ptr()
        stream = torch.cuda.current_stream(dev).cuda_stream
        if file_nsamp is not None:
            assert nsamp is None and play is None and part is None
            _capi.check(_capi.lib().hftt_clip_synth(C.byref(d), stream), 'clip_synth')
        else:
            m = _capi.ClipSynthPartsDesc()
            m.base, m.nsamp = d, t(nsamp, torch.int64)
            for args, pl in ((m.play, play), (m.part_play, part_play)):
                if pl is not None:
                    args.shift, args.t_delay, args.t_scale, args.tune_q31 = t(pl[0], torch.int32), t(pl[1], torch.float64), t(pl[2], torch.float64), t(pl[3], 'u32')
            if part is not None:
                m.part_file, m.part_start, m.part_voice, m.part_gain = t(part[0], torch.int32), t(part[1], torch.int32), t(part[2], torch.int32), t(part[3], torch.float32)
                m.part_nsamp = t(part_nsamp, torch.int64)
            _capi.check(_capi.lib().hftt_clip_synth_parts(C.byref(m), stream), 'clip_synth_parts')
        torch.cuda.synchronize(dev)
        assert bool(torch.isnan(arena[:GUARD]).all()) and bool(torch.isnan(arena[GUARD + n * span:]).all()), 'the arena around the scratch was written'
        self.rows = arena[GUARD:GUARD + n * span].view(n, span)
        self.bits = self.rows.view(torch.int32)
        self.tables = (samp0, ofile, ostart)

    def same(self, other):
        return torch.equal(self.bits, other.bits) and all(torch.equal(a, b) for a, b in zip(self.tables, other.tables))

    def check(self, n_prime, starts, lead=0, width=S.WIDTH):
        """the tables are the formulas', every sample of a pseudo-file is written and nothing behind it -> the pseudo-files (numpy), the tables"""
        t = S.pseudo_tables(n_prime, starts, width=width, lead=lead)
        samp0, ofile, ostart = (x.cpu().numpy() for x in self.tables)
        assert np.array_equal(samp0, t['samp0']) and np.array_equal(ofile, t['win_file']) and np.array_equal(ostart, t['win_start'])
        rows, out = self.rows.cpu().numpy(), []
        for b in range(len(starts)):
            m = int(t['e'][b] - t['o'][b])
            assert not np.isnan(rows[b, :m]).any(), 'a sample of pseudo-file %d was not written' % (2 * b)
            assert np.isnan(rows[b, m:]).all(), 'the remainder of row %d was written' % b
            out.append(rows[b, :m].copy())
        return out, t


def _columns(parts, key):
    return [p[key] for p in parts]


def _play_cols(parts):
    return tuple([p['play'][k] for p in parts] for k in ('shift', 't_delay', 't_scale', 'tune'))


def _run_windows(tab, vb, wins, **kw):
    """the windows of synth_parts_emul (pairs of parts) through the C ABI with every group given"""
    A = [a for a, _ in wins]
    B = [b if b is not None else {'file': -1, 'start': 0, 'voice': 0, 'gain': 1.0, 'nsamp': 0, 'play': P.IDENTITY} for _, b in wins]
    return _Run(tab, vb, _columns(A, 'file'), _columns(A, 'start'), _columns(A, 'voice'), nsamp=_columns(A, 'nsamp'), play=_play_cols(A),
                part=(_columns(B, 'file'), _columns(B, 'start'), _columns(B, 'voice'), _columns(B, 'gain')), part_nsamp=_columns(B, 'nsamp'), part_play=_play_cols(B), **kw)


# ------------------------------------------------------------------------------------------------ identity: the two copies of the walk
@pytest.mark.parametrize('name', ['N5-H3-lead3', 'N5-H1-lead0', 'N88-H3-lead0'])
def test_an_identity_performance_is_hftt_clip_synth_bit_for_bit(dev, name):
    """synth_emul's own cases (the crowd of 300, the far window, invalid files and voices, a lead): all four outputs"""
    table, bank, _, _ = S.reference(name)
    _, _, _, file_nsamp, windows, lead = S.cases()[name]
    tab, vb = _upload(table, bank, dev)
    files, starts, voices = ([w[k] for w in windows] for k in range(3))
    old = _Run(tab, vb, files, starts, voices, lead=lead, file_nsamp=file_nsamp)
    n = len(windows)
    nsamp = [file_nsamp[f] if 0 <= f < len(file_nsamp) else 0 for f in files]
    null = _Run(tab, vb, files, starts, voices, lead=lead, nsamp=nsamp)
    assert null.same(old) and bool((~torch.isnan(old.rows)).any())
    ident = ([0] * n, [0.0] * n, [1.0] * n, [P.UNISON] * n)
    values = _Run(tab, vb, files, starts, voices, lead=lead, nsamp=nsamp, play=ident, part=([-1] * n, [5] * n, [0] * n, [0.5] * n), part_nsamp=[9000] * n, part_play=ident)
    assert values.same(old)
    # a partner voice outside the bank, and a partner that lies wholly outside its own file: no partner either
    away = _Run(tab, vb, files, starts, voices, lead=lead, nsamp=nsamp, part=([0] * n, [5] * n, [vb.V] * n, [0.5] * n), part_nsamp=[9000] * n)
    gone = _Run(tab, vb, files, starts, voices, lead=lead, nsamp=nsamp, part=([1 % tab.n_files] * n, starts, [0] * n, [0.5] * n), part_nsamp=[-3] * n)
    assert away.same(old) and gone.same(old)


# ------------------------------------------------------------------------------------------------ each option against the old kernel on prepared inputs
@pytest.fixture(scope='module')
def five(dev):
    from hftt_hip.ops import labels_table_host
    notes, N, bank, nsamp, _ = P.cases()['N5-H3']
    table = labels_table_host(notes, S.config(N))
    tab, vb = _upload(table, bank, dev)
    return notes, table, bank, nsamp, tab, vb


WINS = ((0, 4, 2), (1, 0, 1), (2, 644, 0), (3, 2, 0), (0, 9, 1), (2, 690, 1))        # (file, first frame, voice) of the prepared equalities


def test_a_transposition_is_the_old_kernel_on_a_table_with_the_pitches_moved(dev, five):
    from hftt_hip.ops import labels_table_host
    notes, table, bank, nsamp, tab, vb = five
    files, starts, voices = ([w[k] for w in WINS] for k in range(3))
    shifts = [2, -2, 1, -1, -2, 4]
    n = len(WINS)
    got = _Run(tab, vb, files, starts, voices, nsamp=[nsamp[f] for f in files], play=(shifts, [0.0] * n, [1.0] * n, None))
    for k in sorted(set(shifts)):
        moved = [[dict(x, pitch=x['pitch'] + k) for x in f if 21 <= x['pitch'] + k < 26] for f in notes]
        assert any(len(a) < len(b) for a, b in zip(moved, notes))                               # notes left the range
        mtab, _ = _upload(labels_table_host(moved, S.config(5)), bank, dev)
        want = _Run(mtab, vb, files, starts, voices, file_nsamp=nsamp)
        rows = [b for b in range(n) if shifts[b] == k]
        assert torch.equal(got.bits[rows], want.bits[rows]) and all(torch.equal(x, y) for x, y in zip(got.tables, want.tables)), k
    assert bool((got.rows[0] != 0).any())


def test_a_time_map_is_the_old_kernel_on_a_table_with_the_times_mapped_in_fp64(dev, five):
    from hftt_hip.ops import labels_table_host
    notes, table, bank, nsamp, tab, vb = five
    files, starts, voices = ([w[k] for w in WINS] for k in range(3))
    n = len(WINS)
    pl = P.play_of(int(1.1 * 2 ** 24) | 1, int(100.3 * 2 ** 24))
    mapped_n = [P.nsamp_play(table, f, nsamp[f], pl) for f in range(len(nsamp))]
    got = _Run(tab, vb, files, starts, voices, nsamp=[mapped_n[f] for f in files], play=([0] * n, [pl['t_delay']] * n, [pl['t_scale']] * n, None))
    mapped = [[dict(x, onset=float(P.time_map(x['onset'], pl)), offset=float(P.time_map(x['offset'], pl))) for x in f] for f in notes]
    mtab, _ = _upload(labels_table_host(mapped, S.config(5)), bank, dev)
    assert np.array_equal(mtab.row_ptr.cpu().numpy(), tab.row_ptr.cpu().numpy())                 # the same records in the same order
    want = _Run(mtab, vb, files, starts, voices, file_nsamp=mapped_n)
    assert got.same(want) and bool((got.rows[0] != 0).any())
    plain = _Run(tab, vb, files, starts, voices, file_nsamp=nsamp)
    assert not torch.equal(got.bits[0], plain.bits[0])


def test_a_tune_is_the_old_kernel_on_a_bank_with_the_increments_scaled(dev, five):
    from hftt_hip import ops
    notes, table, bank, nsamp, tab, vb = five
    files, starts, voices = ([w[k] for w in WINS] for k in range(3))
    n = len(WINS)
    tunes = [int(ops.tune_q31(c)) for c in (30.0, -45.0, 50.0, 0.0, 30.0, 50.0)]
    got = _Run(tab, vb, files, starts, voices, nsamp=[nsamp[f] for f in files], play=(None, None, None, tunes))
    for tune in sorted(set(tunes)):
        scaled = dict(bank, inc=((bank['inc'].astype(np.uint64) * np.uint64(tune)) >> np.uint64(31)).astype(np.uint32))
        want = _Run(tab, ops.VoiceBank(device=dev, **scaled), files, starts, voices, file_nsamp=nsamp)
        rows = [b for b in range(n) if tunes[b] == tune]
        assert torch.equal(got.bits[rows], want.bits[rows]) and all(torch.equal(x, y) for x, y in zip(got.tables, want.tables)), tune
    assert tunes[2] > 1 << 31 > tunes[1] and tunes[3] == 1 << 31


def test_a_partner_at_gain_one_under_a_silent_primary_is_the_old_kernel_on_the_partners_file(dev, five):
    notes, table, bank, nsamp, tab, vb = five
    # primary: the file without notes (3,000 samples) from frame 0; partner: file 3 under voice 1, its frame 5 at column 0 -> partner samples
    # 1,280 .. 4,280; and file 0's crowd, its frame 9 at column 0
    got = _Run(tab, vb, [4, 4], [0, 0], [0, 2], nsamp=[3000, 3000], part=([3, 0], [5, 9], [1, 2], [1.0, 1.0]), part_nsamp=[nsamp[3], nsamp[0]])
    old = _Run(tab, vb, [3, 0], [5, 9], [1, 2], file_nsamp=nsamp)
    for b, ps in enumerate((5, 9)):
        o = (ps - 4) * S.HOP                                                                     # the old window's pseudo-file starts here
        want = old.bits[b, ps * S.HOP - o:ps * S.HOP - o + 3000]
        assert torch.equal(got.bits[b, :3000], want) and bool((want != 0).any()), b
        assert bool(torch.isnan(got.rows[b, 3000:]).all())                                       # cut to n'_A
    assert got.tables[1].tolist() == [0, 2] and got.tables[0].tolist()[:4] == [0, 3000, S.span_of(), S.span_of() + 3000]


def test_the_sum_runs_primary_first_in_table_order_the_cancelling_duet(dev):
    from hftt_hip.ops import labels_table_host
    bank, notes, nsamp = P.cancel_duet()
    tab, vb = _upload(labels_table_host(notes, S.config(3)), bank, dev)
    duet = _Run(tab, vb, [0], [0], [0], width=24, nsamp=[nsamp[0]], part=([1], [0], [1], [1.0]), part_nsamp=[nsamp[1]])
    alone = _Run(tab, vb, [2], [0], [1], width=24, file_nsamp=nsamp)
    assert torch.equal(duet.bits, alone.bits) and bool((alone.rows[0, :6000] != 0).any()) and bool(torch.isnan(alone.rows[0, 6000:]).all())


# ------------------------------------------------------------------------------------------------ everything on
@pytest.mark.parametrize('name', sorted(P.cases()))
def test_the_combined_case_against_fp64(dev, name):
    table, bank, wins, t_ref, rows = P.reference(name)
    tab, vb = _upload(table, bank, dev)
    run = _run_windows(tab, vb, wins)
    V = bank['amp'].shape[0]
    n_prime = [A['nsamp'] if 0 <= A['file'] < tab.n_files and 0 <= A['voice'] < V else -1 for A, _ in wins]
    got, t = run.check(n_prime, [A['start'] for A, _ in wins])
    assert all(np.array_equal(t[k], t_ref[k]) for k in t)
    worst, seen, silent_seen = 0.0, 0, 0
    for b in range(len(wins)):
        ref, bound, terms = rows[b]
        silent = terms == 0
        assert (got[b][silent].view(np.int32) == 0).all(), (name, b, 'a sample where nothing sounds is not +0')
        err = np.abs(got[b].astype(np.float64) - ref)
        if (~silent).any():
            worst = max(worst, float((err[~silent] / bound[~silent]).max()))
        seen += int((~silent).sum())
        silent_seen += int(silent.sum())
    print('%s: largest error / bound %.3g over %d sounding samples (%d silent)' % (name, worst, seen, silent_seen))
    assert worst <= 1.0, (name, worst)
    assert seen > 5000 and (silent_seen > 0 or name.startswith('N88'))


def test_overlapping_windows_with_equal_draws_give_the_same_samples(dev):
    table, bank, wins, _, _ = P.reference('N5-H3')
    tab, vb = _upload(table, bank, dev)
    pairs = []
    for A, B in (wins[0], wins[2]):                                                             # the two crowds; the far window with its cut partner
        pairs += [(A, B), (dict(A, start=A['start'] + 3), dict(B, start=B['start'] + 3))]        # three frames later: another tile origin, the same offset
    run = _run_windows(tab, vb, pairs)
    lead = _run_windows(tab, vb, pairs, lead=3)
    got, t = run.check([A['nsamp'] for A, _ in pairs], [A['start'] for A, _ in pairs])
    led, tl = lead.check([A['nsamp'] for A, _ in pairs], [A['start'] for A, _ in pairs], lead=3)
    common = 0
    for a, b in ((0, 1), (2, 3)):
        lo, hi = max(t['o'][a], t['o'][b]), min(t['e'][a], t['e'][b])
        assert hi - lo > 2 * S.TILE
        x, y = got[a][lo - t['o'][a]:hi - t['o'][a]], got[b][lo - t['o'][b]:hi - t['o'][b]]
        assert np.array_equal(x.view(np.int32), y.view(np.int32)) and bool(x.any()), (a, b)
        common += int(hi - lo)
    for b in range(len(pairs)):                                                                  # a lead moves the tile origin and nothing else
        assert np.array_equal(led[b][t['o'][b] - tl['o'][b]:].view(np.int32), got[b].view(np.int32)), b
    assert common > 8000


# ------------------------------------------------------------------------------------------------ the store
def _store_inputs(dev):
    from corpus.make_dataset import assemble_synth_store
    from hftt_hip import ops
    config = S.config(5)
    r = np.random.default_rng(7)
    notes = [M.draw_notes(r, 30, [21, 22, 23, 24, 25], span=1024, longest=300), M.draw_notes(r, 20, [22, 23, 24], span=800, longest=200), [],
             M.draw_notes(r, 12, [23], span=600, longest=100)]
    bank = S.random_bank(3, 5, 3, seed=77)
    bank['inc'] = bank['inc'] // np.uint32(2)                                                    # an octave of headroom: any tune stays below Nyquist
    vb = ops.VoiceBank(device=dev, **bank)
    store = assemble_synth_store(notes, config, release_samples=int(bank['release'].max()))
    return config, notes, vb, store


def _draws(st, ids):
    """what SynthClipStore.batch draws for `ids`, from a twin with the same seeds: the order is the store's contract (voice; the augment's gain
    and noise; play; duet; the partner's play; the room)"""
    from training.dataset import warped_frame
    ids = torch.as_tensor(ids, device=st.device)
    B, hop = ids.numel(), st.logmel.hop
    file, frame = st.clip_file[ids], st.clip_frame[ids]
    d = {'file': file, 'voice': st.draw_voice(B)}
    d['gain'], d['noise'], d['seed'] = st.augment.draw(B) if st.augment is not None else (None, None, 0)
    d['warp'], d['tune'] = st.play.draw_play(st.gen, B, hop, *st._semitones(file))
    d['frame'] = warped_frame(frame, d['warp'], hop)
    on, partner, d['pvoice'], d['pgain'] = st.play.draw_duet(st.gen, B, len(st), st.bank.V)
    pfile, pframe = st.clip_file[partner], st.clip_frame[partner]
    d['pwarp'], d['ptune'] = st.play.draw_play(st.gen, B, hop, *st._semitones(pfile))
    d['pframe'] = warped_frame(pframe, d['pwarp'], hop)
    d['pfile'] = torch.where(on, pfile, torch.full_like(pfile, -1))
    d['room'] = st.augment.draw_room(B) if st.augment is not None and st.augment.rooms else None
    return d


@pytest.mark.parametrize('room', [False, True], ids=['dry', 'room'])
def test_the_store_under_a_play_labels_from_the_walker_and_spec_from_the_composition(dev, room):
    from corpus import synth_audio as SA
    from hftt_hip import ops
    from training.dataset import SynthClipStore, SynthPlay, WaveAugment
    config, notes, vb, store = _store_inputs(dev)
    play = SynthPlay(transpose=(-3, 3), tune_cents=40.0, tempo=(0.7, 1.4), shift=True, p_play=0.8, duet_p=0.6, duet_gain_db=(-6.0, 0.0))
    aug = lambda: None
    if room:
        ir, taps = SA.synth_room_bank(3, 16000, taps=512, rt60=(0.02, 0.05), seed=2)
        bank = ops.RoomBank(ir, dev, taps=taps)
        aug = lambda: WaveAugment(room_p=0.7, room_bank=bank, seed=5)
    st, twin = (SynthClipStore(store, config, dev, vb, seed=11, augment=aug(), play=play) for _ in range(2))
    ids = list(range(0, len(st), max(1, len(st) // 6)))[:6]
    for _ in range(2):                                                                          # two batches: the draw counts per batch are fixed
        got, d = st.batch(ids), _draws(twin, ids)
    cin, hop = config['input'], 256
    T, mb, width = cin['num_frame'], cin['margin_b'], cin['margin_b'] + cin['num_frame'] + cin['margin_f']
    nsamp = ops.synth_nsamp(st.table, st.file_nsamp, d['file'], d['warp'])
    # labels: the numpy walker fed the draws
    c = {k: v.cpu().numpy() for k, v in d.items() if torch.is_tensor(v)}
    sr = float(config['feature']['sr'])
    src = lambda f, start, w, b: {'notes': notes[f], 'start': int(start), 'shift': int(w.shift[b]), 't_delay': float(w.t_delay(sr)[b]), 't_scale': float(w.t_scale()[b])}
    a_frames = ops.synth_frames(nsamp, hop).cpu().numpy()
    duets = 0
    for b in range(len(ids)):
        A = src(int(c['file'][b]), c['frame'][b], d['warp'], b)
        Bp = src(int(c['pfile'][b]), c['pframe'][b], d['pwarp'], b) if c['pfile'][b] >= 0 else None
        duets += Bp is not None
        want = M.mix_labels(config, A, Bp, T, int(a_frames[b]))
        for k in range(4):
            assert np.array_equal(got[1 + k][b].cpu().numpy().astype(want[k].dtype), want[k]), (b, k)
    assert 0 < duets and bool(got[1].any()) and len(set(c['tune'].tolist())) > 1 and int(d['warp'].shift.abs().sum()) > 0
    # spec: clip_logmel over what ops.clip_synth gives for those draws
    part = ops.SynthPart(d['pfile'], d['pframe'] - mb, d['pvoice'], d['pgain'], d['pwarp'], d['ptune'])
    wave, samp0, wfile, wstart = ops.clip_synth(st.table, st.file_nsamp, vb, d['voice'], d['file'], d['frame'] - mb, width, hop, sr, lead=st.lead,
                                                play=d['warp'], tune=d['tune'], part=part, nsamp=nsamp)
    if room:
        assert st.lead == 2
        wave, samp0, wfile, wstart = ops.clip_room(ops.WetTable(wave, samp0), wfile, wstart, width, st.augment.room_bank, d['room'], hop)
    want = ops.clip_logmel(ops.WetTable(wave, samp0), st.logmel, wfile, wstart, width, st.fill, gain=d['gain'], noise_std=d['noise'], seed=d['seed'])
    assert torch.equal(got[0], want) and bool(torch.isfinite(got[0]).all()) and bool((got[0] != st.fill).any())


def test_the_store_without_a_play_gives_the_batches_it_always_gave(dev):
    from hftt_hip import ops
    from training.dataset import SynthClipStore, SynthPlay
    config, notes, vb, store = _store_inputs(dev)
    st, twin, played = SynthClipStore(store, config, dev, vb, seed=11, play=None), SynthClipStore(store, config, dev, vb, seed=11), SynthClipStore(store, config, dev, vb, seed=11, play=SynthPlay(p_play=0.0))
    ids = list(range(0, len(st), max(1, len(st) // 6)))[:6]
    cin = config['input']
    width, mb = cin['margin_b'] + cin['num_frame'] + cin['margin_f'], cin['margin_b']
    for _ in range(2):
        got = st.batch(ids)
        voice = twin.draw_voice(len(ids))
        t = torch.tensor(ids, device=dev)
        file, frame = st.clip_file[t], st.clip_frame[t]
        out, samp0, ofile, ostart = ops.clip_synth(st.table, st.file_nsamp, vb, voice, file, frame - mb, width, 256, 16000.0)
        want = (ops.clip_logmel(ops.WetTable(out, samp0), st.logmel, ofile, ostart, width, st.fill),) + ops.labels_render(st.table, file, frame, cin['num_frame'], form='train')
        assert all(torch.equal(x, y) for x, y in zip(got, want))
    # a play that never plays (p_play = 0: identity values through the new launches) draws the same first voices and gives the same first batch
    a, b = SynthClipStore(store, config, dev, vb, seed=11).batch(ids), played.batch(ids)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and bool(a[1].any())
