"""A numpy model of the streaming note decoder (csrc/notes_stream.hip, hftt_notes_stream_step): one stream, a ring of H rows, a fixed-size
record per pitch, the same step interface.  The walk below is the kernel's, statement for statement, so that the kernel can be held to it
with == and the model itself to AMT.mpe2note (tests/test_notes_stream_emul_bound.py).

Per pitch the record holds the commit frame c (every onset peak in front of it has been returned, or is the one pending `head`), the values
on[c - 1], off[c - 1] and the value of the run in front of the run that holds c - 1 on both tracks, and the head's frame, time and velocity.
A step walks the rows c .. row_end once more, never older ones.

A frame is DECIDED when its peak status cannot change any more: its value is below the threshold, or not above the run in front of it, or its
run has ended.  Only the trailing run of a track can be undecided, and only while it could still become a peak.

DEFECTS: wrong variants of single rules, switched on by name, that the criteria of the bound test must reject."""
import numpy as np

NEG = np.float32(-np.inf)
FOUND, UNDEC, END, PASSED = 0, 1, 2, 3
NO, PEAK, OPEN = 0, 1, 2
DEFECTS = ('horizon_is_end', 'plateau_early', 'no_trim_guard', 'no_clip', 'velocity_at_run_start', 'state_lost_at_wrap', 'below_at_next_onset')


class _Cursor:
    """the run of one track that holds a frame, moved forward run by run; rows below W only"""

    def __init__(self, get, c, m1, pv, W, thr, closed, defect):
        self.get, self.W, self.thr, self.closed, self.defect = get, W, thr, closed, defect
        self.valid = c < W
        if self.valid:
            v = get(c)
            self.s, self.v = c, v
            self.pv = NEG if c == 0 else (m1 if v != m1 else pv)
            self._extend()

    def _extend(self):
        i = self.s + 1
        while i < self.W and self.get(i) == self.v:
            i += 1
        self.e = i - 1
        self.open = i == self.W
        self.nv = NEG if self.open else self.get(i)

    def next(self):
        self.s, self.pv, self.v = self.e + 1, self.v, self.nv
        self._extend()

    def status(self):
        if not (self.v >= self.thr and self.v > self.pv):
            return NO
        if self.open:
            if self.closed or (self.defect == 'horizon_is_end' and self.e == self.s) or (self.defect == 'plateau_early' and self.e > self.s):
                return PEAK
            return OPEN
        return PEAK if self.v > self.nv else NO

    def find(self, q, L):
        """the first peak frame >= q: (FOUND, frame) | (UNDEC, first frame >= q that is undecided) | (PASSED, -) no peak up to L, all
        decided | (END, -) no peak below W, all decided.  The cursor stays on the run of the answer."""
        while True:
            if not self.valid:
                return END, -1
            if q > self.e:
                if self.open:
                    return END, -1
                self.next()
                continue
            start = max(q, self.s)
            if start > L:
                return PASSED, -1
            st = self.status()
            if st == OPEN:
                return UNDEC, start
            if st == PEAK:
                return FOUND, start
            if self.open:
                return END, -1
            self.next()


class StreamEmul:
    def __init__(self, N, H, hop, thred_onset=0.5, thred_offset=0.5, thred_mpe=0.5, mode_velocity='ignore_zero', note_min=21, defect=None):
        assert defect is None or defect in DEFECTS
        self.N, self.H, self.hop, self.note_min, self.defect = N, H, float(hop), note_min, defect
        self.thr = (np.float32(thred_onset), np.float32(thred_offset), np.float32(thred_mpe))
        self.keep_zero = mode_velocity != 'ignore_zero'
        self.ring = [np.zeros((H, N), np.float32) for _ in range(3)] + [np.zeros((H, N), np.int8)]
        self.row_end, self.closed, self.overflow = 0, False, False
        z = lambda dt: np.zeros(N, dt)
        self.st = dict(c=z(np.int64), w=z(np.int64), head=z(np.int64), head_time=z(np.float64), head_vel=z(np.int32),
                       on_m1=z(np.float32), on_pv=z(np.float32), off_m1=z(np.float32), off_pv=z(np.float32), flags=z(np.int32))

    # ------------------------------------------------------------------ the producer's side
    def room(self):
        """rows that the ring takes without losing one that a walk still needs"""
        if self.closed or self.overflow:
            return 0
        return self.H - (self.row_end - int(self.st['c'].min()))

    def deliver(self, on, off, mpe, vel, close=False):
        n = len(on)
        assert n <= self.H and not self.closed
        for ring, a in zip(self.ring, (on, off, mpe, vel)):
            for i in range(n):
                ring[(self.row_end + i) % self.H] = a[i]
        self.row_end += n
        self.closed = bool(close)

    # ------------------------------------------------------------------ peak time (model/amt.py _pick_peaks), fp32 refinement
    def _ptime(self, get, i, W, closed):
        t = i * self.hop
        last = closed or self.defect == 'horizon_is_end'
        if i == 0 or (last and i == W - 1):
            return t
        l, c, r = get(i - 1), get(i), get(i + 1)
        h2 = np.float32(self.hop * 0.5)
        with np.errstate(all='ignore'):
            if l > r:
                return float(np.float32(t) - (h2 * (l - r)) / (c - r))
            if l < r:
                return float(np.float32(t) + (h2 * (r - l)) / (c - l))
        return t

    # ------------------------------------------------------------------ one pitch, one step: (notes, new record)
    def _walk(self, j):
        s, H, hop, d = self.st, self.H, self.hop, self.defect
        W, closed, c = self.row_end, self.closed, int(s['c'][j])
        ron, roff, rmp, rvel = self.ring
        m1 = (s['on_m1'][j], s['off_m1'][j])
        on = lambda i: m1[0] if i == c - 1 else ron[i % H, j]
        off = lambda i: m1[1] if i == c - 1 else roff[i % H, j]
        vel = lambda i: int(rvel[i % H, j])
        oc = _Cursor(on, c, m1[0], s['on_pv'][j], W, self.thr[0], closed, d)
        fc = _Cursor(off, c, m1[1], s['off_pv'][j], W, self.thr[1], closed, d)

        def below(a, b):
            for i in range(a, min(b, W)):
                if rmp[i % H, j] < self.thr[2]:
                    return i
            return -1

        notes = []
        head = int(s['head'][j]) - 1
        new_head, c_new = -1, W
        ft, fv = float(s['head_time'][j]), int(s['head_vel'][j])
        f, have = head, head >= 0
        if not have:
            kind, f = oc.find(c, W)
            have = kind == FOUND
            if kind == UNDEC:
                c_new = f
        while have:
            kept = True
            if f != head:
                fv = vel(oc.s if d == 'velocity_at_run_start' else f)
                kept = self.keep_zero or fv > 0
                if kept:
                    ft = self._ptime(on, f, W, closed)
            x = max(f + 1, c)
            kind, ln = oc.find(x, W)
            if not kept:                                         # a dropped onset: it only ended the note in front of it
                if kind == FOUND:
                    f = ln
                    continue
                c_new = ln if kind == UNDEC else W
                break
            val = None
            if kind == FOUND:                                    # case A: the next onset peak is known
                tn = self._ptime(on, ln, W, closed)
                m = below(x, ln + 1 if d == 'below_at_next_onset' else ln)
                k2, p = fc.find(x, W if d == 'no_clip' else ln)
                if k2 == UNDEC and p <= ln:
                    c_new = min(ln, p, m if m >= 0 else ln)
                else:
                    loff, toff = (p, self._ptime(off, p, W, closed)) if k2 == FOUND else (ln, tn)
                    val = toff if m < 0 or loff <= m else m * hop
                    if d == 'below_at_next_onset' and m == ln:
                        val = m * hop
                    if self.keep_zero or vel(ln) > 0:
                        val = min(val, tn)
                    elif ln + 1 <= oc.e and d != 'no_trim_guard' and (self.keep_zero or vel(ln + 1) > 0):
                        val = min(val, self._ptime(on, ln + 1, W, closed))
            elif closed:                                         # the file's last onset
                k2, p = fc.find(x, W)
                m = below(x, W)
                if k2 == FOUND:
                    val = self._ptime(off, p, W, closed) if m < 0 or p <= m else m * hop
                else:
                    val = m * hop if m >= 0 else (W - 1) * hop
            else:                                                # case B: no onset peak decided behind f
                d_on = ln if kind == UNDEC else W
                k2, p = fc.find(x, W)
                lim = W if k2 == END else p
                m = below(x, lim)
                ev = -1
                if m >= 0:
                    ev, v = m, m * hop
                elif k2 == FOUND:
                    ev, v = p, self._ptime(off, p, W, closed)
                if ev >= 0 and d_on > ev + (0 if d == 'no_trim_guard' else 1):
                    val = v
                else:
                    c_new = min(d_on, lim, m if m >= 0 else W)
            if val is None:                                      # not final: f waits as the head
                new_head = f
                break
            notes.append((j + self.note_min, fv, ft, val))
            if kind != FOUND:
                c_new = W if closed else d_on
                break
            f = ln
        rec = dict(c=c_new, w=W, head=new_head + 1, head_time=ft if new_head >= 0 else 0.0, head_vel=fv if new_head >= 0 else 0, flags=1 if closed else 0)
        for name, get in (('on', on), ('off', off)):
            cur, pv = s[name + '_m1'][j], s[name + '_pv'][j]
            for i in range(c, c_new):
                v = get(i)
                if i == 0:
                    cur, pv = v, NEG
                elif v != cur:
                    cur, pv = v, cur
            rec[name + '_m1'], rec[name + '_pv'] = cur, pv
        if d == 'state_lost_at_wrap' and c_new // H != c // H:
            rec['head'] = 0
        return notes, rec

    # ------------------------------------------------------------------ the step
    def count_overflow(self):
        s = self.st
        for j in range(self.N):
            if s['flags'][j] & 2 or (not s['flags'][j] & 1 and (self.row_end - int(s['c'][j]) > self.H or self.row_end - int(s['w'][j]) > self.H)):
                return True
        return False

    def step(self, cap=None):
        """-> (notes pitch-major with ascending onset frame, as (pitch, velocity, onset, offset), total); with total > cap nothing is
        returned and the records stay as they were"""
        s = self.st
        if self.count_overflow():
            self.overflow = True
            s['flags'] |= 2
            return [], 0
        out, recs = [], []
        for j in range(self.N):
            if s['flags'][j] & 1:
                recs.append(None)
                continue
            notes, rec = self._walk(j)
            out += notes
            recs.append(rec)
        if cap is not None and len(out) > cap:
            return [], len(out)
        for j, rec in enumerate(recs):
            if rec is not None:
                for k, v in rec.items():
                    s[k][j] = v
        return out, len(out)


def as_dicts(notes):
    """the records of all steps -> the sorted list of AMT.mpe2note"""
    got = [{'pitch': int(p), 'onset': float(a), 'offset': float(b), 'velocity': int(v)} for p, v, a, b in notes]
    return sorted(sorted(got, key=lambda x: x['pitch']), key=lambda x: x['onset'])


def run_split(emul, on, off, mpe, vel, sizes):
    """deliver the rows in steps of `sizes` (the last one closes; zeros are steps without rows; 'room': each step fills the ring's room) -> (all notes in the order returned,
    [(rows delivered, notes so far)] per step)"""
    notes, log, r = [], [], 0
    F = len(on)
    k = 0
    while True:
        n = min(emul.room(), F - r) if sizes == 'room' else sizes[k]
        last = r + n == F if sizes == 'room' else k == len(sizes) - 1
        emul.deliver(on[r:r + n], off[r:r + n], mpe[r:r + n], vel[r:r + n], close=last)
        r += n
        k += 1
        got, total = emul.step()
        assert total == len(got)
        notes += got
        log.append((r, len(notes)))
        if last:
            assert r == F
            return notes, log


# ---------------------------------------------------------------------- the tracks and splits that both test files use
HOP = 256 / 16000
THR = (0.6, 0.55, 0.5)


def tracks(seed, F, N):
    """the recipe of tests/test_notes_gpu.py::_tracks: smoothed noise quantised to 1/20 (plateaus, exact ties)"""
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


def smooth_tracks(seed, F, N):
    """unquantised noise: no two neighbouring frames are equal, so no plateau exists and every frame is decided one row later"""
    r = np.random.RandomState(seed)
    on, off, mpe = (r.rand(F, N).astype(np.float32) for _ in range(3))
    for a in (on, off, mpe):
        assert (a[1:] != a[:-1]).all()
    vel = r.randint(1, 128, size=(F, N)).astype(np.int8)
    return on, off, mpe, vel


def scene(F, N=8):
    on = np.full((F, N), 0.1, np.float32)
    off = np.full((F, N), 0.1, np.float32)
    mpe = np.full((F, N), 0.9, np.float32)
    vel = np.full((F, N), 64, np.int8)
    return on, off, mpe, vel


def constant_scene(F):
    """constant tracks at and just below the threshold (tests/test_notes_gpu.py): every frame an onset, with offsets, with mpe below"""
    on, off, mpe, vel = scene(F, 4)
    thr = np.float32(THR[0])
    on[:, 0] = thr
    on[:, 1] = np.nextafter(thr, np.float32(0))
    on[:, 2] = thr; off[:, 2] = np.float32(THR[1])
    on[:, 3] = thr; mpe[:, 3] = 0.2
    vel[5::7, 2] = 0
    return on, off, mpe, vel


def hand_scene(ch=48):
    """the hand-built tracks of tests/test_notes_gpu.py with `ch` in the place of the decode chunk: plateaus, ties, both signs of the
    refinement, clipping, the three offset rules, the trim with a dropped note in between, and peaks at both ends of the file"""
    F = 2 * ch + 120
    on, off, mpe, vel = scene(F)
    b = 110                                                                                  # the plateau block sits behind the single events
    on[b + ch - 3:b + ch + 4, 0] = 0.8
    on[b + 2 * ch - 2:b + 2 * ch, 0] = 0.8; on[b + 2 * ch - 3, 0] = 0.95
    off[b + ch - 1:b + ch + 1, 0] = 0.7
    on[b + ch - 2:b + 2 * ch + 1, 1] = 0.7
    off[F - 5:, 1] = 0.9
    on[F - 5:, 2] = 0.9
    on[0, 2] = 0.9; on[1, 2] = 0.3
    on[F - 1, 3] = 0.9; on[F - 2, 3] = 0.4
    off[0, 3] = 0.8; off[F - 1, 3] = 0.8
    on[10, 3] = 0.9; on[9, 3] = on[11, 3] = 0.4
    on[20, 3] = 0.9; on[19, 3] = 0.3; on[21, 3] = 0.5
    on[30, 3] = 0.9; on[29, 3] = 0.5; on[31, 3] = 0.3
    off[25, 3] = 0.9; off[24, 3] = 0.2; off[26, 3] = 0.3
    on[10, 4] = 0.9; on[20, 4] = 0.9; off[30, 4] = 0.9
    on[40, 4] = 0.9; mpe[41, 4] = 0.1
    on[50, 4] = 0.9; vel[50, 4] = 0
    on[52, 4] = 0.9; off[51, 4] = 0.9; mpe[60, 4] = 0.1
    on[70, 4] = 0.9; off[75, 4] = 0.9; mpe[73, 4] = 0.1
    on[80, 4] = 0.9; off[83, 4] = 0.9; mpe[86, 4] = 0.1
    on[90, 4] = 0.9; off[93, 4] = 0.9; mpe[93, 4] = 0.1
    on[b + ch - 1, 4] = 0.9; off[b + ch, 4] = 0.9; mpe[b + ch + 1, 4] = 0.1
    # pitch 5: the trim guard -- an offset peak at p pushed late by half a hop, a kept onset at p + 1 pulled early by as much: in fp32 the
    # onset comes out one ulp EARLIER; a dropped onset plateau frame with a
    # kept one behind it; an onset whose only offset peak lies beyond the next onset with a dip at the next onset itself
    under = np.nextafter(np.float32(0.9), np.float32(0))
    on[10, 5] = 0.9; off[14, 5] = 0.9; off[13, 5] = 0.2; off[15, 5] = under; on[15, 5] = 0.9; on[14, 5] = under; on[16, 5] = 0.2
    on[30, 5] = 0.9; on[34:36, 5] = 0.8; vel[34, 5] = 0; off[36, 5] = 0.9; on[33, 5] = 0.75
    on[50, 5] = 0.9; on[55, 5] = 0.9; on[56, 5] = 0.5; mpe[55, 5] = 0.1; off[58, 5] = 0.9
    on[70, 5] = 0.9; mpe[72, 5] = 0.1; on[73, 5] = 0.9; on[72, 5] = 0.85
    on[15, 6] = 0.9; vel[15, 6] = 0
    on[100, 7] = 0.9; on[104, 7] = 0.9; on[108, 7] = 0.9; vel[104, 7] = 0; off[b + 90, 7] = 0.9
    on[b + 2 * ch - 1, 7] = 0.9; on[b + 2 * ch, 7] = 0.3
    return on, off, mpe, vel


def splits(F, H, seed):
    """everything at once (a ring as long as the file is the caller's part), one row per step, random sizes with empty steps, steps of
    exactly the ring's room"""
    r = np.random.RandomState(seed)
    rnd = []
    while sum(rnd) < F:
        rnd.append(int(min(F - sum(rnd), r.choice([0, 0, 1, 2, 3, 5, 17, H // 4]))))
    return {'room': 'room', 'rows': [1] * F, 'random': rnd + [0]}
