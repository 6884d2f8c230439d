"""hftt_clip_synth restated on the host from include/hftt_hip.h (a helper, not a test; nothing here was read off the kernel): the fp64 value of the
header's formula on the fp32 / uint32 table entries, an fp32 emulation of its rounding chain (with the defects a kernel could have, for
test_synth_emul_bound.py), the per-sample bound, the pseudo-file tables, and the inputs the GPU test runs -- so that the CPU test holds the
emulation to the bound on exactly those.

The bound of one sample, every sounding term t = (record, partial) with c64 / arg the exact coefficient / exponent on the table entries:
    sum_t |c64_t| (EPS_S + ln 2 |arg_t| 2^-23 + EPS_E + K_C 2^-24)  +  gamma(n) sum_t |c64_t|  +  n 2^-126
  EPS_S              |S(u) - sin(2 pi u)| of v_sin_f32, absolute, over EVERY u the contract can form (|S| <= 1 multiplies c)
  ln 2 |arg| 2^-23   the exponent dec tf + rel rf carries two product roundings and one sum rounding, each <= 2^-24 of a part of arg
                     (tf, rf exact below 2^24 samples); d/dy 2^y = ln 2 2^y
  EPS_E              |E(y) / 2^y - 1| of v_exp_f32 on [-126, 0]
  K_C = 4            the roundings of c: amp * vel_gain, the division of the ramp, and two products
  gamma(n)           the worst case of the n fmas of the chain, in any order (room_emul.gamma); n 2^-126 covers every underflow

EPS_S and EPS_E were measured ONCE on an MI355X by tools/synth_fn_error.hip (profiles/clip_synth_mi355x.txt):
  S  exhaustive over the 150,994,960 arguments (float)(int32)x * 2^-32 (both signs of every float an int32 converts to): largest error
     1.254137e-07 = 2^-22.927 (at u = 0.257801473) -> rounded up to a power of two, no further margin: EPS_S = 2^-22
  E  a grid of 2^25 + 2 arguments over [-126, 0]: largest relative error 8.270945e-08 = 2^-23.527 (at y = -8.93766975) -> times 2 (the grid
     is not exhaustive) = 2^-22.527, rounded up likewise: EPS_E = 2^-22"""
import numpy as np

from room_emul import gamma, lead as room_lead

HOP, NFFT, WIDTH, SR = 256, 2048, 16, 16000.0
TILE, CHUNK = 2048, 256                     # the kernel's tiling as the header states it: tiles of 2,048 samples, filter passes of 256 records
EPS_S = 2.0 ** -22                          # measured 2^-22.927 (profiles/clip_synth_mi355x.txt)
EPS_E = 2.0 ** -22                          # measured 2^-23.527, times 2
K_C = 4
F32 = np.float32


# ------------------------------------------------------------------------------------------------ tables
def note(pitch, onset, offset, velocity=64):
    return {'pitch': pitch, 'onset': onset, 'offset': offset, 'velocity': velocity}


def config(N, note_min=21, sr=SR, hop=HOP):
    return {'feature': {'sr': int(sr), 'hop_sample': hop, 'mel_bins': 8, 'n_bins': 8, 'fft_bins': NFFT, 'window_length': NFFT, 'log_offset': 1e-8},
            'input': {'margin_b': 2, 'margin_f': 2, 'num_frame': WIDTH - 4, 'min_value': -18.420681, 'max_value': 0.0},
            'midi': {'note_min': note_min, 'num_note': N, 'num_velocity': 128}}


def random_bank(V, N, H, seed, sr=SR):
    """a bank that exercises the formula, not an instrument: frequencies anywhere below Nyquist, amplitudes of both signs with some partials off,
    decays from none to 60 dB in 50 ms, releases, attacks from 1 sample up"""
    r = np.random.RandomState(seed)
    inc = np.round(r.uniform(20.0, 0.5 * sr, (V, N, H)) / sr * 2.0 ** 32).astype(np.uint64).astype(np.uint32)
    amp = (r.uniform(-1.0, 1.0, (V, N, H)) * (r.uniform(0, 1, (V, N, H)) > 0.15)).astype(F32)
    dec = (np.exp(r.uniform(np.log(1e-6), np.log(0.025), (V, N, H))) * (r.uniform(0, 1, (V, N, H)) > 0.1)).astype(F32)
    vel_gain = r.uniform(0.05, 1.0, (V, 128)).astype(F32)
    rel = np.exp(r.uniform(np.log(1e-4), np.log(0.05), V)).astype(F32)
    attack = r.randint(1, 200, V).astype(np.int32)
    attack[0] = 1
    release = r.randint(0, 3000, V).astype(np.int32)
    return {'inc': inc, 'amp': amp, 'dec': dec, 'vel_gain': vel_gain, 'rel': rel, 'attack': attack, 'release': release}


def records(table, f):
    """the records of file f of a host note table (ops.labels_table_host) in TABLE order: (n_on, D int64; pitch index, velocity)"""
    N = table['N']
    rp = table['row_ptr'][f * N:(f + 1) * N + 1].astype(np.int64)
    rows = table['notes'][rp[0]:rp[-1]]
    sr = np.float64(table['sr'])
    n_on = (rows['onset_sec'] * sr + 0.5).astype(np.int64)                      # numpy rounds the product and the sum separately
    n_off = (rows['offset_sec'] * sr + 0.5).astype(np.int64)
    pitch = np.repeat(np.arange(N), np.diff(rp))
    return n_on, np.maximum(n_off - n_on, 1), pitch, np.clip(rows['velocity'], 0, 127).astype(np.int64)


def phase_turns(inc, tau):
    """u = (float)(int32)(inc * (uint32)tau) * 2^-32 as fp32 (exact wrapped product, one rounding in the conversion, an exact scaling)"""
    prod = (np.uint64(inc) * (tau.astype(np.uint64) & np.uint64(0xFFFFFFFF))) & np.uint64(0xFFFFFFFF)
    return prod.astype(np.uint32).view(np.int32).astype(F32) * F32(2.0 ** -32)


# ------------------------------------------------------------------------------------------------ fp64 and the bound
def render64(table, bank, f, v, i0, i1):
    """samples [i0, i1) of file f under voice v -> (fp64 value of the header's formula, the bound, the number of sounding terms), each [i1 - i0]"""
    n = max(0, i1 - i0)
    ref, mag, slope, terms = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n, np.int64)
    if n == 0:
        return ref, ref.copy(), terms
    i = np.arange(i0, i1, dtype=np.int64)
    att, relse, rel = max(int(bank['attack'][v]), 1), max(int(bank['release'][v]), 0), np.float64(bank['rel'][v])
    H = bank['amp'].shape[2]
    for on, D, p, vel in zip(*records(table, f)):
        tau = i - on
        live = (tau >= 0) & (tau < D + relse)
        if not live.any():
            continue
        t = tau[live]
        ra = np.minimum(t + 1, att).astype(np.float64) / att
        vg = np.float64(bank['vel_gain'][v, vel])
        for h in range(H):
            arg = np.minimum(np.float64(bank['dec'][v, p, h]) * t + rel * np.maximum(0, t - D), 126.0)
            c = np.float64(bank['amp'][v, p, h]) * vg * ra * np.exp2(-arg)
            ref[live] += c * np.sin(2.0 * np.pi * phase_turns(bank['inc'][v, p, h], t).astype(np.float64))
            mag[live] += np.abs(c)
            slope[live] += np.abs(c) * (EPS_S + np.log(2.0) * arg * 2.0 ** -23 + EPS_E + K_C * 2.0 ** -24)
        terms[live] += H
    return ref, slope + gamma(terms) * mag + terms * 2.0 ** -126, terms


# ------------------------------------------------------------------------------------------------ the fp32 chain, and what a kernel could get wrong
def _fma32(a, b, c):
    """fma(a, b, c) in fp32: the product of two fp32 is exact in fp64 (one further rounding in the fp64 sum is below the fp32 result's by 2^-29)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def render32(table, bank, f, v, i0, i1, defect=None, origin=None):
    """the header's rounding chain in fp32 numpy with correctly rounded S and E -> fp32 [i1 - i0].  defect: None, or one of
         'phase_fp32'     the phase as an fp32 product inc * tau instead of the wrapped integer product
         'onset_late'     every onset one sample late
         'no_release'     a record ends at its offset
         'rel_from_onset' the release decay runs from the onset
         'vel_by_pitch'   the velocity curve read at the pitch index
         'leak'           the record that follows the file's last one in the table (a neighbouring file's) sounds too
         'drop_overflow'  of the records that sound inside a tile of TILE samples only the first CHUNK are kept
         'time_order'     the records summed in onset order
         'tile_origin'    the oscillator as an fp32 rotation recurrence anchored at `origin` (the first sample of the caller's tile)"""
    n = max(0, i1 - i0)
    acc = np.zeros(n, F32)
    if n == 0:
        return acc
    i = np.arange(i0, i1, dtype=np.int64)
    att, relse, rel = max(int(bank['attack'][v]), 1), max(int(bank['release'][v]), 0), F32(bank['rel'][v])
    H = bank['amp'].shape[2]
    recs = list(zip(*records(table, f)))
    if defect == 'leak':
        N = table['N']
        nxt = int(table['row_ptr'][(f + 1) * N])
        if nxt < len(table['notes']):
            r = table['notes'][nxt]
            on = np.int64(r['onset_sec'] * np.float64(table['sr']) + 0.5)
            recs.append((on, max(np.int64(r['offset_sec'] * np.float64(table['sr']) + 0.5) - on, 1), N - 1, int(np.clip(r['velocity'], 0, 127))))
    if defect == 'time_order':
        recs.sort(key=lambda r: r[0])
    if defect == 'onset_late':
        recs = [(on + 1, D, p, vel) for on, D, p, vel in recs]
    if defect == 'no_release':
        relse = 0
    kept = {}                                               # tile -> records kept so far ('drop_overflow')
    for on, D, p, vel in recs:
        tau = i - on
        live = (tau >= 0) & (tau < D + relse)
        if defect == 'drop_overflow':
            for tile in np.unique(i[live] // TILE):
                kept[tile] = kept.get(tile, 0) + 1
                if kept[tile] > CHUNK:
                    live &= i // TILE != tile
        if not live.any():
            continue
        t = tau[live]
        tf = t.astype(F32)
        rf = (t if defect == 'rel_from_onset' else np.maximum(0, t - D)).astype(F32)
        ra = np.minimum(t + 1, att).astype(F32) / F32(att)
        vg = bank['vel_gain'][v, p if defect == 'vel_by_pitch' else vel]
        a = acc[live]
        for h in range(H):
            inc = bank['inc'][v, p, h]
            if defect == 'phase_fp32':
                x = F32(np.float64(inc) * 2.0 ** -32) * tf
                u = (x - np.floor(x)).astype(F32)
            elif defect == 'tile_origin':
                u = _rotation(inc, t, (i0 if origin is None else origin) - on)
            else:
                u = phase_turns(inc, t)
            s = np.sin(2.0 * np.pi * u.astype(np.float64)).astype(F32)
            x = np.minimum(bank['dec'][v, p, h] * tf + rel * rf, F32(126.0))    # fp32 * fp32 + fp32 * fp32: numpy rounds each
            e = np.exp2(-x.astype(np.float64)).astype(F32)
            c = ((bank['amp'][v, p, h] * vg) * ra) * e
            a = _fma32(c, s, a)
        acc[live] = a
    return acc


def _rotation(inc, tau, tau_anchor):
    """the phase a per-thread rotation would carry: exact at the anchor, then angle += (float)inc 2^-32 per sample in fp32 -- in turns, so that the
    caller's sin sees the drift"""
    step = F32(np.float64(inc) * 2.0 ** -32)
    u0 = phase_turns(inc, np.array([max(tau_anchor, 0)], np.int64))[0]
    x = u0 + step * (tau - max(tau_anchor, 0)).astype(F32)
    return (x - np.round(x)).astype(F32)


# ------------------------------------------------------------------------------------------------ the tables the kernel writes
def span_of(width=WIDTH, lead=0, hop=HOP, n_fft=NFFT):
    return (room_lead(hop, n_fft) + lead + width - 1) * hop + n_fft // 2


def pseudo_tables(n_prime, win_start, width=WIDTH, lead=0, hop=HOP, n_fft=NFFT, span=None):
    """n_prime[b]: samples of window b's file, negative for a window without a valid file or voice -> dict(o, e [B]; samp0 int64 [2 B + 1],
    win_file, win_start int32 [B]) by the header's formulas"""
    span = span_of(width, lead, hop, n_fft) if span is None else span
    B, front = len(n_prime), room_lead(hop, n_fft) + lead
    o, e = np.zeros(B, np.int64), np.zeros(B, np.int64)
    samp0, wf, ws = np.zeros(2 * B + 1, np.int64), np.zeros(B, np.int32), np.zeros(B, np.int32)
    for b in range(B):
        s, n = int(win_start[b]), max(int(n_prime[b]), 0)
        o[b] = max(0, s - front) * hop
        e[b] = min(n, (s + width - 1) * hop + n_fft // 2)
        valid = int(n_prime[b]) >= 0 and o[b] <= n
        length = max(0, e[b] - o[b]) if valid else 0
        e[b] = o[b] + length
        samp0[2 * b], samp0[2 * b + 1] = b * span, b * span + length
        wf[b], ws[b] = (2 * b if valid else -1), s - o[b] // hop
    samp0[2 * B] = B * span
    return {'o': o, 'e': e, 'samp0': samp0, 'win_file': wf, 'win_start': ws}


# ------------------------------------------------------------------------------------------------ the inputs of tests/test_synth_gpu.py
# width 16 at hop 256: a row shows (4 + 16 - 1) * 256 + 1024 = 5,888 samples = two full tiles of 2,048 and one of 1,792 (lead 3: + 768 = three
# full tiles and 512).  Files of the N = 5 corpus (sr 16,000):
#   0  no notes                                         1  one note
#   2  300 records that all sound at once (more than a filter pass of 256 holds), spread over the pitches, in a tile of the window at frame 8
#   3  a note that straddles the border of tiles 0 and 1 of the window at frame 8; one whose onset lies 10 s in front of that window
#      (tau ~ 160,000: the phase has wrapped thousands of times); two of one pitch that overlap (list order); one cut by the file's end
FILE_NSAMP5 = (3000, 9000, 12000, 180000, 7000)
SEC = 1.0 / SR


def notes5():
    r = np.random.RandomState(5)
    crowd = [note(21 + int(r.randint(0, 5)), (2100 + int(r.randint(0, 900))) * SEC, (3300 + int(r.randint(0, 2000))) * SEC, int(r.randint(1, 128))) for _ in range(300)]
    w = 640 * HOP                                           # the window at frame 640 + 4 of file 3 starts at sample 163,840
    far = [note(23, (w - 160000) * SEC, (w + 3000) * SEC, 90), note(22, (w + TILE - 700) * SEC, (w + TILE + 900) * SEC, 50),
           note(25, (w + 100) * SEC, (w + 2500.4) * SEC, 127), note(25, (w + 1500) * SEC, (w + 1500) * SEC, 1), note(21, 178000 * SEC, 179990 * SEC, 77)]
    return [[], [note(24, 0.05, 0.3, 100)], crowd, far, [note(22, 0.0, 0.2, 64), note(22, 0.1, 0.35, 3)]]


# (file, first frame, voice): the file's start from frame -3; one note; the crowd; file 3's far window (border, 10 s, overlap) and its end
# (cut by n'); windows before a file and behind it; the empty file; a bad file index; a voice out of range
WINDOWS5 = ((4, -3, 0), (1, 0, 1), (2, 4, 2), (3, 644, 0), (3, 690, 1), (1, -40, 0), (1, 60, 0), (0, 0, 2), (7, 0, 0), (-1, 0, 0), (1, 0, 3), (1, 0, -1))


def notes88():
    r = np.random.RandomState(88)
    out = []
    for _ in range(40):
        on = float(r.uniform(0.0, 0.9))
        out.append(note(21 + int(r.randint(0, 88)), on, on + float(r.uniform(0.02, 0.5)), int(r.randint(1, 128))))
    return [out]


FILE_NSAMP88 = (20000,)
WINDOWS88 = ((0, 0, 0), (0, 30, 1))


# The cancelling pair (summation order): one voice without decay, ramp or velocity curve, H = 1; pitches 0 and 1 have the same increment and
# amplitudes +1024 and -1024, so that with E(0) = 1 their coefficients are powers of two, c S is exact, and two notes with the same times cancel
# to the bit WHEN THEY ARE ADJACENT in the sum; pitch 2 is quiet.  Table order is pitch order: (0, 1, 2) = big, -big, quiet -> the sample is the
# quiet note's alone, bit for bit.  In time order the quiet note, which starts first, stands in front and loses its low bits to the big one.
def cancel_case():
    bank = {'inc': np.array([[[300000000], [300000000], [123456789]]], np.uint32), 'amp': np.array([[[1024.0], [-1024.0], [1e-3]]], F32),
            'dec': np.zeros((1, 3, 1), F32), 'vel_gain': np.ones((1, 128), F32), 'rel': np.zeros(1, F32), 'attack': np.ones(1, np.int32),
            'release': np.zeros(1, np.int32)}
    pair = [note(21, 0.05, 0.2, 64), note(22, 0.05, 0.2, 64)]
    quiet = [note(23, 0.01, 0.3, 64)]
    return bank, [pair + quiet, quiet], (6000, 6000)


# ------------------------------------------------------------------------------------------------ the cases, and their reference (computed once)
def cases():
    """name -> (note lists, N, bank, file_nsamp, windows, lead): H = 1, 3, 32 on the N = 5 corpus, lead 3 at H = 3, and the N = 88 table"""
    out = {}
    for H, lead in ((1, 0), (3, 0), (3, 3), (32, 0)):
        out['N5-H%d-lead%d' % (H, lead)] = (notes5(), 5, random_bank(3, 5, H, seed=100 + H), FILE_NSAMP5, WINDOWS5, lead)
    out['N88-H3-lead0'] = (notes88(), 88, random_bank(2, 88, 3, seed=188), FILE_NSAMP88, WINDOWS88, 0)
    return out


_REFERENCE = {}


def reference(name):
    """(host note table, bank, tables, [(fp64 reference, bound, terms) per window]) of a case; computed at the first call and then shared"""
    if name not in _REFERENCE:
        from hftt_hip.ops import labels_table_host
        notes, N, bank, nsamp, windows, lead = cases()[name]
        table = labels_table_host(notes, config(N))
        V = bank['amp'].shape[0]
        n_prime = [nsamp[f] if 0 <= f < len(nsamp) and 0 <= v < V else -1 for f, _, v in windows]
        t = pseudo_tables(n_prime, [s for _, s, _ in windows], lead=lead)
        rows = [render64(table, bank, f, v, int(t['o'][b]), int(t['e'][b])) if t['win_file'][b] >= 0 else None for b, (f, _, v) in enumerate(windows)]
        _REFERENCE[name] = (table, bank, t, rows)
    return _REFERENCE[name]
