"""hftt_clip_synth_parts restated on the host from include/hftt_hip.h (a helper, not a test; nothing here was read off the kernel).  It extends
synth_emul.py: the records of a file under a PLAY (records_play), the fp64 value of the header's formula for a window of two parts with the
per-sample bound (render64_parts), the fp32 rounding chain with the defects a kernel could have (render32_parts, for
test_synth_parts_emul_bound.py), and the inputs the GPU test runs -- so that the CPU test holds the emulation to the bound on exactly those.

A part is a dict: file, voice, start (the part's frame that window column 0 shows), nsamp (n', the part's length under its map), play (play_of:
shift, t_delay, t_scale, tune) and, for a partner, gain.  A window is (A, B), B None without a partner.

The bound is synth_emul's formula, term by term, with K_C = 5 on partner terms: their coefficient carries one further rounding, the product
with part_gain.  EPS_S, EPS_E and gamma are synth_emul's and room_emul's as they stand; nothing is re-measured.  The tuning product and the time
map are exact integer / correctly rounded fp64 operations that the reference performs too: they add nothing to the bound."""
from fractions import Fraction

import numpy as np

import synth_emul as S
from room_emul import gamma
from synth_emul import F32, HOP, NFFT, SR, WIDTH, note

K_C_PARTNER = S.K_C + 1
UNISON = 1 << 31


# ------------------------------------------------------------------------------------------------ a play and the records under it
def play_of(step_q24=1 << 24, delay_q24=0, shift=0, cents=0.0, sr=SR):
    """tempo * 2^24, delay in samples * 2^24, semitones, cents -> what the kernel takes, derived as ops.Warp derives it: t_scale = 2^24 / step,
    t_delay = delay / 2^24 / sr (fp64), tune = round(2^(cents / 1200) 2^31)"""
    return {'shift': int(shift), 't_delay': np.float64(delay_q24) / np.float64(1 << 24) / np.float64(sr), 't_scale': np.float64(1 << 24) / np.float64(step_q24),
            'tune': int(np.round(np.exp2(np.float64(cents) / 1200.0) * 2.0 ** 31)), 'step_q24': int(step_q24), 'delay_q24': int(delay_q24)}


IDENTITY = play_of()


def time_map(t, pl, fma=False):
    """t' = fmul(fadd(t, t_delay), t_scale): fp64, two roundings (numpy rounds each).  fma: ONE rounding of the exact value (a defect)"""
    t = np.asarray(t, np.float64)
    if fma:
        td, ts = Fraction(float(pl['t_delay'])), Fraction(float(pl['t_scale']))
        return np.array([float((Fraction(float(x)) + td) * ts) for x in t.ravel()], np.float64).reshape(t.shape)
    return (t + np.float64(pl['t_delay'])) * np.float64(pl['t_scale'])


def records_play(table, f, pl, defect=None):
    """the records of file f under play pl that can sound, in TABLE order: (n_on, D int64; bank row; velocity; t'_on, t'_off fp64).  A record whose
    row p + shift lies outside 0 .. N - 1 is dropped.  defect: 'map_fma', 'map_onset_only', 'row_minus' (row p - shift), 'row_clamp' (clamped)"""
    N = table['N']
    rp = table['row_ptr'][f * N:(f + 1) * N + 1].astype(np.int64)
    rows = table['notes'][rp[0]:rp[-1]]
    sr = np.float64(table['sr'])
    t_on = time_map(rows['onset_sec'], pl, fma=defect == 'map_fma')
    t_off = rows['offset_sec'].astype(np.float64) if defect == 'map_onset_only' else time_map(rows['offset_sec'], pl, fma=defect == 'map_fma')
    n_on = (t_on * sr + 0.5).astype(np.int64)
    n_off = (t_off * sr + 0.5).astype(np.int64)
    row = np.repeat(np.arange(N), np.diff(rp)) + (-pl['shift'] if defect == 'row_minus' else pl['shift'])
    if defect == 'row_clamp':
        row = np.clip(row, 0, N - 1)
    ok = (row >= 0) & (row < N)
    vel = np.clip(rows['velocity'], 0, 127).astype(np.int64)
    return n_on[ok], np.maximum(n_off - n_on, 1)[ok], row[ok], vel[ok], t_on[ok], t_off[ok]


def nsamp_play(table, f, nsamp, pl):
    """the length of file f under its map: nsamp + ceil(t'(file_end_sec) sr) - ceil(file_end_sec sr) (ops.synth_nsamp)"""
    end, sr = np.float64(table['file_end_sec'][f]), np.float64(table['sr'])
    return int(nsamp + np.ceil(time_map(end, pl) * sr) - np.ceil(end * sr))


def tuned(inc, tune):
    """inc' = (uint32)(((uint64)inc * tune) >> 31)"""
    return np.uint32(((int(inc) * int(tune)) >> 31) & 0xFFFFFFFF)


def _parts(table, bank, A, B, i, defect=None):
    """the walk of one window at primary positions i (int64 array), part by part in the order of the sum: yields (records, voice, the part's
    positions, its extent n', gain or None, tune, the voice whose release counts, K_C).  The planted defects that concern WHICH part is walked
    HOW are applied here."""
    V, n_files = bank['amp'].shape[0], len(table['row_ptr']) // table['N']
    out = [(records_play(table, A['file'], A['play'], defect), A['voice'], i, A['nsamp'], None, A['play']['tune'], A['voice'], S.K_C)]
    if B is not None and 0 <= B['file'] < n_files and 0 <= B['voice'] < V:
        delta = (B['start'] - A['start']) * HOP
        pl = dict(B['play'], shift=A['play']['shift']) if defect == 'primary_shift' else B['play']
        v = A['voice'] if defect == 'primary_voice' else B['voice']
        out.append((records_play(table, B['file'], pl, defect), v, i - delta if defect == 'offset_sign' else i + delta,
                    A['nsamp'] if defect == 'cut_at_nA' else B['nsamp'], F32(B['gain']), pl['tune'], A['voice'] if defect == 'primary_release' else v, K_C_PARTNER))
        if defect == 'partner_first':
            out.reverse()
    return out


# ------------------------------------------------------------------------------------------------ fp64 and the bound
def render64_parts(table, bank, A, B, i0, i1):
    """primary samples [i0, i1) of window (A, B) -> (fp64 value of the header's formula, the bound, the number of sounding terms), each [i1 - i0]"""
    n = max(0, i1 - i0)
    ref, mag, slope, terms = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n, np.int64)
    if n == 0:
        return ref, ref.copy(), terms
    H = bank['amp'].shape[2]
    for recs, v, pos, n_part, gain, tune, v_rel, k_c in _parts(table, bank, A, B, np.arange(i0, i1, dtype=np.int64)):
        att, relse, rel = max(int(bank['attack'][v]), 1), max(int(bank['release'][v_rel]), 0), np.float64(bank['rel'][v])
        inside = (pos >= 0) & (pos < max(int(n_part), 0))
        for on, D, p, vel, _, _ in zip(*recs):
            tau = pos - on
            live = inside & (tau >= 0) & (tau < D + relse)
            if not live.any():
                continue
            t = tau[live]
            ra = np.minimum(t + 1, att).astype(np.float64) / att
            vg = np.float64(bank['vel_gain'][v, vel]) * (1.0 if gain is None else np.float64(gain))
            for h in range(H):
                arg = np.minimum(np.float64(bank['dec'][v, p, h]) * t + rel * np.maximum(0, t - D), 126.0)
                c = np.float64(bank['amp'][v, p, h]) * vg * ra * np.exp2(-arg)
                ref[live] += c * np.sin(2.0 * np.pi * S.phase_turns(tuned(bank['inc'][v, p, h], tune), t).astype(np.float64))
                mag[live] += np.abs(c)
                slope[live] += np.abs(c) * (S.EPS_S + np.log(2.0) * arg * 2.0 ** -23 + S.EPS_E + k_c * 2.0 ** -24)
            terms[live] += H
    return ref, slope + gamma(terms) * mag + terms * 2.0 ** -126, terms


# ------------------------------------------------------------------------------------------------ the fp32 chain, and what a kernel could get wrong
def render32_parts(table, bank, A, B, i0, i1, defect=None):
    """the header's rounding chain in fp32 numpy with correctly rounded S and E -> fp32 [i1 - i0].  defect: None, or one of
         'partner_first'    the partner's records summed in front of the primary's
         'offset_sign'      iB = i - (part_start - win_start) hop
         'cut_at_nA'        the partner cut at the primary's length n'_A instead of its own n'_B
         'primary_voice'    the partner played with the primary's voice
         'primary_release'  the partner's records end after the PRIMARY voice's release
         'primary_shift'    the partner transposed by the primary's shift
         'map_fma'          the time map with one rounding
         'map_onset_only'   the time map applied to onsets, offsets as written
         'tune_30'          inc * tune >> 30
         'tune_on_phase'    the tune applied to the wrapped phase inc * tau instead of to inc
         'row_minus'        bank row p - shift
         'row_clamp'        a row outside the bank clamped into it instead of dropped"""
    n = max(0, i1 - i0)
    acc = np.zeros(n, F32)
    if n == 0:
        return acc
    H = bank['amp'].shape[2]
    for recs, v, pos, n_part, gain, tune, v_rel, _ in _parts(table, bank, A, B, np.arange(i0, i1, dtype=np.int64), defect):
        att, relse, rel = max(int(bank['attack'][v]), 1), max(int(bank['release'][v_rel]), 0), F32(bank['rel'][v])
        inside = (pos >= 0) & (pos < max(int(n_part), 0))
        for on, D, p, vel, _, _ in zip(*recs):
            tau = pos - on
            live = inside & (tau >= 0) & (tau < D + relse)
            if not live.any():
                continue
            t = tau[live]
            tf, rf = t.astype(F32), np.maximum(0, t - D).astype(F32)
            ra = np.minimum(t + 1, att).astype(F32) / F32(att)
            vg = bank['vel_gain'][v, vel]
            a = acc[live]
            for h in range(H):
                inc = bank['inc'][v, p, h]
                if defect == 'tune_on_phase':
                    w = (np.uint64(inc) * (t.astype(np.uint64) & np.uint64(0xFFFFFFFF))) & np.uint64(0xFFFFFFFF)
                    w = np.array([(int(x) * int(tune)) >> 31 for x in w], np.uint64) & np.uint64(0xFFFFFFFF)
                    u = w.astype(np.uint32).view(np.int32).astype(F32) * F32(2.0 ** -32)
                else:
                    u = S.phase_turns(np.uint32(((int(inc) * int(tune)) >> 30) & 0xFFFFFFFF) if defect == 'tune_30' else tuned(inc, tune), t)
                s = np.sin(2.0 * np.pi * u.astype(np.float64)).astype(F32)
                x = np.minimum(bank['dec'][v, p, h] * tf + rel * rf, F32(126.0))
                e = np.exp2(-x.astype(np.float64)).astype(F32)
                g0 = bank['amp'][v, p, h] * vg
                if gain is not None:
                    g0 = F32(g0 * gain)
                a = S._fma32((g0 * ra) * e, s, a)
            acc[live] = a
    return acc


# ------------------------------------------------------------------------------------------------ the inputs of tests/test_synth_parts_gpu.py
# Files of the N = 5 corpus (sr 16,000, tiles of 2,048 samples; every file but the empty one is longer than two tiles):
#   0  synth_emul's crowd: 300 records over all five pitches that sound at once in samples 3,300 .. 5,100 (more than one filter pass holds)
#   1  a second crowd of 200 records over all five pitches around samples 2,600 .. 3,400: with file 0 in one window, 500 records in a tile
#   2  synth_emul's far file (a note across a tile border, an onset 10 s in front of the window at frame 644, an overlap, a note cut by the end)
#   3  two overlapping notes of one pitch and a third that ends at sample 8,000 of a file of 7,000: cut by n'
#   4  no notes
FILE_NSAMP5 = (12000, 9000, 180000, 7000, 3000)
SEC = S.SEC


def notes5():
    r = np.random.RandomState(55)
    crowd2 = [note(21 + k % 5, (1500 + int(r.randint(0, 1100))) * SEC, (3400 + int(r.randint(0, 1500))) * SEC, int(r.randint(1, 128))) for k in range(200)]
    base = S.notes5()
    return [base[2], crowd2, base[3], base[4] + [note(24, 0.3, 0.5, 100)], []]


def _part(table, nsamp, file, start, voice, play=IDENTITY, gain=None):
    known = 0 <= file < len(nsamp)
    p = {'file': file, 'start': start, 'voice': voice, 'play': play, 'nsamp': nsamp_play(table, file, nsamp[file], play) if known else 0}
    if gain is not None:
        p['gain'] = gain
    return p


def windows5(table, nsamp=FILE_NSAMP5):
    """the six windows of the combined case.  Tempo 1.1 and 0.8, delays off the sample grid, +30 / -45 / +50 cents, shifts +2 and -2 on files with
    all five pitches (notes leave the bank at BOTH ends), partner offsets +2, -7 and +10 frames"""
    P = lambda *a, **k: _part(table, nsamp, *a, **k)
    fast = play_of(int(1.1 * 2 ** 24) | 1, int(100.3 * 2 ** 24), 2, 30.0)
    slow = play_of(int(0.8 * 2 ** 24) | 1, int(17.7 * 2 ** 24), -2, -45.0)
    sharp = play_of(cents=50.0)
    return [
        (P(0, 4, 2, fast), P(1, 6, 0, slow, gain=0.7)),             # both crowds, every option on both parts; the partner two frames ahead
        (P(1, 0, 1, slow), P(0, -7, 2, sharp, gain=0.5)),           # a window at the file's start; the partner seven frames behind
        (P(2, 644, 0), P(3, 14, 1, play_of(shift=1), gain=1.25)),   # the far window as written; the partner (7,000 samples) ends inside it: n'_B cuts
        (P(4, 0, 1), P(3, 0, 0, gain=1.0)),                         # a primary without notes: the partner alone, over the primary's 3,000 samples
        (P(2, 690, 1, sharp), P(7, 0, 0, gain=1.0)),                # the file's end under a tune; a partner file outside the table: no partner
        (P(3, 2, 0, play_of(shift=-1, delay_q24=int(255.9 * 2 ** 24))), P(0, 2, 9, gain=1.0)),      # a partner voice outside the bank: no partner
    ]


def notes88():
    r = np.random.RandomState(89)
    out = []
    for f in range(2):
        notes = []
        for _ in range(40):
            on = float(r.uniform(0.0, 0.9))
            notes.append(note(21 + int(r.randint(0, 88)), on, on + float(r.uniform(0.02, 0.5)), int(r.randint(1, 128))))
        out.append(notes)
    return out


FILE_NSAMP88 = (20000, 18000)


def windows88(table, nsamp=FILE_NSAMP88):
    P = lambda *a, **k: _part(table, nsamp, *a, **k)
    up, down = play_of(int(0.9 * 2 ** 24) | 1, int(3.25 * 2 ** 24), 7, 12.5), play_of(int(1.3 * 2 ** 24) | 1, 0, -11, -50.0)
    return [(P(0, 0, 0, up), P(1, 3, 1, down, gain=0.9)), (P(1, 30, 1, down), P(0, 21, 0, up, gain=0.35))]


def cases():
    """name -> (note lists, N, bank, file_nsamp, windows(table)): H = 1 and 3 on the N = 5 corpus and the N = 88 table.  Every file used is
    longer than two tiles."""
    out = {}
    for H in (1, 3):
        out['N5-H%d' % H] = (notes5(), 5, S.random_bank(3, 5, H, seed=200 + H), FILE_NSAMP5, windows5)
    out['N88-H3'] = (notes88(), 88, S.random_bank(2, 88, 3, seed=288), FILE_NSAMP88, windows88)
    return out


_REFERENCE = {}


def reference(name):
    """(host note table, bank, windows, tables, [(fp64 reference, bound, terms) per window]) of a case; computed at the first call, then shared"""
    if name not in _REFERENCE:
        from hftt_hip.ops import labels_table_host
        notes, N, bank, nsamp, make = cases()[name]
        table = labels_table_host(notes, S.config(N))
        wins = make(table)
        V = bank['amp'].shape[0]
        n_prime = [A['nsamp'] if 0 <= A['file'] < len(nsamp) and 0 <= A['voice'] < V else -1 for A, _ in wins]
        t = S.pseudo_tables(n_prime, [A['start'] for A, _ in wins])
        rows = [render64_parts(table, bank, A, B, int(t['o'][b]), int(t['e'][b])) if t['win_file'][b] >= 0 else None for b, (A, B) in enumerate(wins)]
        _REFERENCE[name] = (table, bank, wins, t, rows)
    return _REFERENCE[name]


# ------------------------------------------------------------------------------------------------ the cancelling duet (summation order)
# synth_emul's cancelling pair, split over two parts: voice 0 has pitch rows (big, -big, quiet), voice 1 the same with every amplitude negated.
# File 0 holds one record of pitch 0; file 1 a record of pitch 0 with the same times and a later one of pitch 2; file 2 that later one alone.
# Window (file 0 under voice 0) + (file 1 under voice 1, gain 1): primary first, the sum is +big, then -big = +0 exactly, then the quiet record
# from +0 -- bit for bit the render of file 2 under voice 1.  Partner first, the quiet record (which starts first in time, but second in the
# table) stands on -big and loses its low bits.
def cancel_duet():
    bank, _, _ = S.cancel_case()
    two = {k: np.concatenate([v, v]) for k, v in bank.items()}
    two['amp'][1] = -two['amp'][1]
    big, quiet = note(21, 0.05, 0.2, 64), note(23, 0.01, 0.3, 64)
    return two, [[big], [big, quiet], [quiet]], (6000, 6000, 6000)
