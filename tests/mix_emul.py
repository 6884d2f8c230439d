"""numpy restatement of the label rule of clip mixing (include/hftt_hip.h, hftt_labels_render_mix): one cell = frame t of the window and one
pitch, which walks the primary's notes of that pitch in list order and then the partner's, carrying o, off, mpe, vel.  The walk below is the
per-cell rule evaluated for all frames of a pitch at once (each frame's state is its own: no frame reads another's).

A source is a dict: notes (the file's list, dicts with pitch / onset / offset / velocity), start (the file frame that window frame 0 shows) and
optionally shift, t_delay, t_scale (the map of hftt_labels_render_warp; t_scale None = no map).

    mix_labels(config, A, B, length, a_frames)      the contract: B's notes walked behind A's with the carried state
    max_combined(config, A, B, length, a_frames)    the shortcut the contract rules out: two separate renders, combined by maximum
"""
import numpy as np


def grid(config):
    cf = config['feature']
    hop_ms = 1000 * cf['hop_sample'] / cf['sr']
    return hop_ms, cf['sr'] / cf['hop_sample'], int(50.0 / hop_ms + 0.5)


def _frame_of(sec, fps):
    return int(sec * fps + 0.5)


def prepare(config, src, duration_tolerance=False):
    """the source's notes per OUTPUT pitch index, in list order, with what the walk reads of each; and the source's frame count"""
    cm = config['midi']
    N, note_min = cm['num_note'], cm['note_min']
    hop_ms, fps, tol = grid(config)
    notes = src['notes']
    warp = src.get('t_scale') is not None
    shift = int(src.get('shift', 0)) if warp else 0
    td, ts = (np.float64(src['t_delay']), np.float64(src['t_scale'])) if warp else (None, None)
    starts = {}
    for n in notes:                                     # flags bit 0: a property of the note inside its own, unwarped file
        starts.setdefault(n['pitch'], set()).add(n['onset'])
    per_pitch = [[] for _ in range(N)]
    for n in notes:
        on, off = np.float64(n['onset']) + 0.0, np.float64(n['offset']) + 0.0
        if warp:
            on, off = (on + td) * ts, (off + td) * ts
        on_f, off_f = _frame_of(on, fps), _frame_of(off, fps)
        on_ms, off_ms = on * 1000.0, off * 1000.0
        sharp = -1
        if n['offset'] not in starts[n['pitch']]:
            sharp = tol
            if duration_tolerance:
                sharp = max(tol, int((off_ms - on_ms) * 0.2 / hop_ms + 0.5))
        j = n['pitch'] - note_min + shift               # output pitch j walks source pitch j - shift
        if 0 <= j < N:
            per_pitch[j].append((on_f, off_f, on_ms, off_ms, sharp, int(n['velocity'])))
    end = max([0.0] + [n['offset'] for n in notes])
    if not notes:
        nframe = 1
    elif warp:
        nframe = _frame_of((np.float64(end) + td) * ts, fps) + 1
    else:
        nframe = _frame_of(end, fps) + 1
    return per_pitch, nframe


def _walk(config, per_pitch, f, count, state):
    """walk one source: f int64 [length] the source's file frames, count bool [length] where its notes count; state = (o, off, mpe, vel) [length, N]"""
    hop_ms, fps, tol = grid(config)
    o, off, mpe, vel = state
    on_den = tol * hop_ms
    ff = f.astype(np.float64)
    for j, notes in enumerate(per_pitch):
        for on_f, off_f, on_ms, off_ms, sharp, v in notes:
            d_on, d_off = f - on_f, f - off_f
            m = count & (d_on >= -tol) & (d_on <= tol)
            tri = np.maximum(0.0, 1.0 - np.abs(ff * hop_ms - on_ms) / on_den).astype(np.float32)
            o[m, j] = np.maximum(o[m, j], tri[m])
            hit = m & (o[:, j] >= np.float32(0.5)) & ((d_on >= 0) | (vel[:, j] == 0))          # the VALUE vel == 0, after the max
            vel[hit, j] = v
            mpe[count & (d_on >= 0) & (d_off <= 0), j] = True
            if sharp >= 0:
                m = count & (d_off >= -sharp) & (d_off <= sharp)
                tri = np.maximum(0.0, 1.0 - np.abs(ff * hop_ms - off_ms) / (sharp * hop_ms)).astype(np.float32)
                off[m, j] = np.maximum(off[m, j], tri[m])


def _empty(config, length):
    N = config['midi']['num_note']
    return (np.zeros((length, N), np.float32), np.zeros((length, N), np.float32), np.zeros((length, N), bool), np.zeros((length, N), np.int64))


def _counts(config, A, B, length, a_frames, dt):
    t = np.arange(length, dtype=np.int64)
    pa, nfa = prepare(config, A, dt)
    fa = A['start'] + t
    ca = (fa >= 0) & (fa < nfa)
    if B is None:
        return (pa, fa, ca), None
    pb, nfb = prepare(config, B, dt)
    fb = B['start'] + t
    cb = (fb >= 0) & (fb < nfb) & (fa >= 0) & (fa < a_frames)
    return (pa, fa, ca), (pb, fb, cb)


def _typed(state):
    o, off, mpe, vel = state
    return o, off, mpe, vel.astype(np.int8)


def mix_labels(config, A, B, length, a_frames=0, duration_tolerance=False):
    """(onset, offset fp32, mpe bool, velocity int8) [length, N] of the window: A's notes where 0 <= f < nframe_A, then B's (None: no partner)
    where 0 <= fB < nframe_B and 0 <= f < a_frames, with the same carried state"""
    sa, sb = _counts(config, A, B, length, a_frames, duration_tolerance)
    state = _empty(config, length)
    _walk(config, *sa, state)
    if sb is not None:
        _walk(config, *sb, state)
    return _typed(state)


def max_combined(config, A, B, length, a_frames=0, duration_tolerance=False):
    """two separate walks from zero state, combined by maximum: NOT the contract (the velocity track reads the combined onset track)"""
    sa, sb = _counts(config, A, B, length, a_frames, duration_tolerance)
    one, two = _empty(config, length), _empty(config, length)
    _walk(config, *sa, one)
    _walk(config, *sb, two)
    return _typed(tuple(np.maximum(x, y) for x, y in zip(one, two)))


def draw_notes(rng, n, pitches, span=2048, longest=512):
    """n notes on a 1 / 1024 s grid over `pitches`"""
    return [{'pitch': int(rng.choice(pitches)), 'onset': k / 1024.0, 'offset': (k + d) / 1024.0, 'velocity': int(v)}
            for k, d, v in zip(rng.integers(0, span, n), rng.integers(1, longest + 1, n), rng.integers(1, 128, n))]


def cross_touch(a, b):
    """an offset of one list equals an onset of the same pitch in the other: the combined list's "no offset target" flags would differ"""
    on_a, on_b = {(n['pitch'], n['onset']) for n in a}, {(n['pitch'], n['onset']) for n in b}
    return any((n['pitch'], n['offset']) in on_b for n in a) or any((n['pitch'], n['offset']) in on_a for n in b)
