"""The numpy model of the streaming note decoder (tests/notes_stream_emul.py) against AMT.mpe2note with ==, for every split of a file's
rows into steps; causality; promptness; and every planted defect of the model must fail these same criteria.  No GPU."""
import numpy as np
import pytest

import util   # noqa: F401  (puts the package on sys.path)
import notes_stream_emul as E

HOP, THR = E.HOP, E.THR
MODES = ('ignore_zero', 'org')


def _host(on, off, mpe, vel, mv):
    from model.amt import AMT
    amt = AMT({'feature': {'sr': 16000, 'hop_sample': 256}, 'midi': {'note_min': 21, 'num_note': on.shape[1]}}, None, device='cpu')
    return amt.mpe2note(a_onset=on, a_offset=off, a_mpe=mpe, a_velocity=vel, thred_onset=THR[0], thred_offset=THR[1], thred_mpe=THR[2],
                        mode_velocity=mv, mode_offset='shorter')


def _emul(N, H, mv, defect=None):
    return E.StreamEmul(N, H, HOP, *THR, mode_velocity=mv, defect=defect)


def _check(on, off, mpe, vel, H, mv, sizes, defect=None):
    """'' when the streamed notes are the offline ones, else what differs; also the share returned before the closing step"""
    host = _host(on, off, mpe, vel, mv)
    em = _emul(on.shape[1], H, mv, defect)
    notes, log = E.run_split(em, on, off, mpe, vel, sizes)
    if em.overflow:
        return 'overflow', 0, len(host)
    got = E.as_dicts(notes)
    early = log[-2][1] if len(log) > 1 else 0
    if got != host:
        bad = [x for x in got if x not in host][:2] + [x for x in host if x not in got][:2]
        return 'differs: %d / %d notes, e.g. %r' % (len(got), len(host), bad), early, len(host)
    return '', early, len(host)


def _cases():
    """(name, tracks, ring rows): the random recipe at every size, the hand-built scenes"""
    out = []
    for F in (1, 2, 3, 7, 64, 257, 513):
        for N in (1, 8):
            out.append(('tracks-%d-%d' % (F, N), E.tracks(7 * F + N, F, N), 64))
    out.append(('hand', E.hand_scene(), 128))
    out.append(('constant', E.constant_scene(131), 192))
    return out


CASES = _cases()


@pytest.mark.parametrize('name,tr,H', CASES, ids=[c[0] for c in CASES])
def test_every_split_gives_the_offline_notes(name, tr, H):
    F = len(tr[0])
    total = 0
    for mv in MODES:
        for kind, sizes in E.splits(F, H, F).items():
            if kind == 'rows' and F > 300 and mv == 'org':
                continue                                                    # the slowest split once per size
            msg, early, n = _check(*tr, H, mv, sizes)
            assert msg == '', (name, mv, kind, msg)
            total += n
        msg, early, n = _check(*tr, max(F, 4), mv, [F])                         # everything at once, in the closing step
        assert msg == '', (name, mv, 'once', msg)
    if F >= 64 and tr[0].shape[1] >= 8:
        assert total > 0


def test_hand_built_scene_holds_what_it_is_built_for():
    on, off, mpe, vel = E.hand_scene()
    host = _host(on, off, mpe, vel, 'org')
    pitches = {x['pitch'] for x in host}
    assert 21 + 6 in pitches and len([x for x in host if x['pitch'] == 22]) == 48 + 3
    n5 = [x for x in host if x['pitch'] == 26]
    assert len(n5) >= 9
    # the trim guard's case: the note at frame 10 ends at the onset of frame 15, which lies BEFORE the offset peak's refined time at frame 14
    a = [x for x in n5 if x['onset'] == 10 * HOP][0]
    b = [x for x in n5 if abs(x['onset'] - 15 * HOP) < HOP][0]
    assert a['offset'] == b['onset'] < 14.5 * HOP


def test_causality_a_shared_prefix_gives_the_same_notes():
    F, N, H, cut = 257, 8, 160, 150
    a = E.tracks(11, F, N)
    b = tuple(x.copy() for x in a)
    r = np.random.RandomState(5)
    for x, y in zip(b[:3], E.tracks(12, F, N)[:3]):
        x[cut:] = y[cut:]
    b[3][cut:] = r.randint(0, 128, size=(F - cut, N))
    for sizes in ([1] * F, [50, 50, 50, 107], [cut, F - cut]):
        ea, eb = _emul(N, H, 'ignore_zero'), _emul(N, H, 'ignore_zero')
        na, la = E.run_split(ea, *a, sizes)
        nb, lb = E.run_split(eb, *b, sizes)
        k = max(i for i, (rows, _) in enumerate(la) if rows <= cut)
        assert la[k][1] == lb[k][1] and na[:la[k][1]] == nb[:lb[k][1]]
        assert la[k][1] > 0 and na != nb


def _events(on, off, mpe, mv):
    """per note of a plateau-free file: (pitch, onset time) -> the frame of its deciding event (next onset peak, first offset peak, first frame
    below thred_mpe), None when the file ends first"""
    from model.amt import _pick_peaks
    out = {}
    for j in range(on.shape[1]):
        loc, times = _pick_peaks(on[:, j], THR[0], HOP)
        ploc, _ = _pick_peaks(off[:, j], THR[1], HOP)
        bl = np.nonzero(mpe[:, j] < np.float32(THR[2]))[0]
        for q, f in enumerate(loc):
            ev = [int(loc[q + 1])] if q + 1 < len(loc) else []
            ev += [int(p) for p in ploc[ploc > f][:1]] + [int(m) for m in bl[bl > f][:1]]
            out[(21 + j, float(times[q]))] = min(ev) if ev else None
    return out


def _prompt(defect=None):
    """one row per step on plateau-free tracks: '' when every note is out by the step that delivers row g + 2"""
    F, N, H = 200, 8, 64
    on, off, mpe, vel = E.smooth_tracks(3, F, N)
    on[on < 0.9] *= 0.5                                                     # sparse onsets: notes that wait for an offset or a dip
    ev = _events(on, off, mpe, 'org')
    em = _emul(N, H, 'org', defect)
    notes, log = E.run_split(em, on, off, mpe, vel, [1] * F)
    late, seen = [], 0
    for rows, n in log:
        for p, v, a, b in notes[seen:n]:
            g = ev.get((p, a))
            if g is not None and g + 2 < F - 1 and rows - 1 > g + 2:
                late.append((p, a, g, rows - 1))
        seen = n
    assert len(ev) > 50
    return '%d late notes, e.g. %r' % (len(late), late[:2]) if late else ''


def test_promptness_without_plateaus():
    assert _prompt() == ''


def test_promptness_on_the_random_tracks():
    early = total = 0
    for seed in range(6):
        tr = E.tracks(100 + seed, 257, 8)
        for mv in MODES:
            msg, e, n = _check(*tr, 64, mv, [1] * 257)
            assert msg == ''
            early += e
            total += n
    assert total > 500 and early >= 0.9 * total, (early, total)


def _fails_somewhere(defect):
    """the criteria above, applied to the model with one defect: the first that fails"""
    for name, tr, H in CASES:
        F = len(tr[0])
        if F > 300:
            continue
        for mv in MODES:
            for kind, sizes in E.splits(F, H, F).items():
                try:
                    msg = _check(*tr, H, mv, sizes, defect)[0]
                except (AssertionError, IndexError, ValueError) as e:
                    msg = 'raised %r' % (e,)
                if msg:
                    return '%s %s %s: %s' % (name, mv, kind, msg)
    return ''


@pytest.mark.parametrize('defect', E.DEFECTS)
def test_planted_defects_fail_the_criteria(defect):
    assert _fails_somewhere(defect) != '', defect


def test_a_decoder_that_waits_for_close_fails_promptness():
    F, N = 257, 8
    tr = E.tracks(100, F, N)
    host = _host(*tr, 'org')
    em = _emul(N, 1024, 'org')
    em.deliver(*tr, close=True)                                             # everything in the closing step: exact, and never early
    notes, total = em.step()
    assert E.as_dicts(notes) == host
    early = 0                                                               # what test_promptness_on_the_random_tracks counts
    assert len(host) > 50 and not early >= 0.9 * len(host)
