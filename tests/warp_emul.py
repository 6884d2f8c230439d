"""numpy fp32 restatement, fp64 ideal and per-sample criterion of the warp (include/hftt_hip.h: hftt_wave_warp, hftt_clip_logmel_warp), and the
host oracle of hftt_labels_render_warp.  Nothing here touches a device; tests/clip_logmel_emul.py and tests/frontend_emul.py are imported, not
edited.

  proto_table / cut_of / warp_len       the table, the cutoff and n' as the contract states them
  wave_warp_emul     warped samples j of one file, operation for operation in numpy fp32 (every `*`, `+`, `-` below on np.float32 operands is one
                     IEEE rounding, as under `#pragma clang fp contract(off)`); defect=<name> plants one wrong variant
  wave_warp_ideal    the same filter evaluated analytically in fp64 -- no table -- on the fp32 source, and the bound (below)
  staged_emul / staged_ideal            the sample the clip log-mel stages: clip_logmel_emul.mix's gain and noise on the warped sample, keyed on j
  warp_notes / labels_oracle            a note list under t' = (t + t_delay) * t_scale and a pitch shift, through corpus.conv_note2label

The bound of one warped sample (identity windows: 0, the sample is copied).  Write p(u) = sinc(u) cos^2(pi u / 2Z) and u_i = d_i cut / 2^24.
Per tap the kernel's weight w_i differs from p(u_i) by at most EPS_W:
  * position: (float)d and the product with cut round once each, so the table position is off by at most u * 2^-23 <= Z * 2^-23; |p'| <= 1.7
    (|sinc'| <= 1.371, the window's slope <= pi / 2Z = 0.262 against |sinc| <= 1): 1.7 * 6 * 2^-23 = 1.22e-6
  * linear interpolation between entries 1 / L apart: (1 / L)^2 / 8 * max|p''|, |p''| <= pi^2 / 3 + 2 * 1.371 * 0.262 + (pi / 2Z)^2 / 2 * 2 <= 4.2:
    2.0e-6 at L = 512
  * the entries are rounded once (<= 2^-25, |T| <= 1) and the interpolation is a convex combination of them: 2^-25
  * fsub, fmul, fadd of the interpolation on magnitudes <= 1: 3 * 2^-24
A tap that one side's test |d| cut <= Z 2^24 admits and the other's does not has u within Z * 2^-22 of Z, where |p| < 1e-12: inside EPS_W as well.
The term fmul(fmul(w, cut), s) carries two more roundings and the sequential sum over K <= 27 terms at most (K - 1) * 2^-24 * sum |term|
(Higham, Accuracy and Stability, 4.4), so
    |got - ideal| <= sum_i cut |s_i| (EPS_W + |p(u_i)| (K + 1) 2^-24 * 1.01)
over the taps the ideal admits with u <= Z (1 + 2^-20).  The staged sample adds the two roundings of mix: gain * bound + 2^-24 (|gain * ideal| +
|gain * ideal + noise|) * 1.01."""
import numpy as np
import torch

import clip_logmel_emul as CE

Z, L = 6, 512                                   # HFTT_WARP_ZEROS, HFTT_WARP_TABLE_L
TABLE_LEN = Z * L + 2
ONE = 1 << 24
STEP_MIN, STEP_MAX = 1 << 23, 1 << 25
H_MAX = 14                                      # (int)(Z / cut) + 2 at the smallest cutoff, 0.99 / 2
K_MAX = 27
EPS_W = 1.7 * Z * 2.0 ** -23 + (1.0 / L) ** 2 / 8 * 4.2 + 2.0 ** -25 + 3 * 2.0 ** -24
DEFECTS = ('taps_not_scaled_by_cut', 'delay_wrong_sign', 'n_warped_off_by_one', 'neighbour_samples_at_border', 'noise_keyed_on_source_index',
           'identity_not_bypassed', 'rate_inverted')

F32 = np.float32


def proto(u):
    """p(u) in fp64 (0 beyond Z)"""
    u = np.abs(np.asarray(u, np.float64))
    return np.where(u < Z, np.sinc(u) * np.cos(np.pi * u / (2 * Z)) ** 2, 0.0)


def proto_table():
    t = proto(np.arange(TABLE_LEN, dtype=np.float64) / L)
    t[Z * L:] = 0.0
    return t.astype(F32)


def step_of(semitones):
    """round(2^(semitones / 12) * 2^24): the step of a pitch shift"""
    return int(round(2.0 ** (semitones / 12.0) * ONE))


def cut_of(step):
    return F32(0.99 * min(1.0, float(ONE) / float(step)))


def warp_len(n, step, delay):
    return 0 if n <= 0 else (((n - 1) << 24) + delay) // step + 1


def is_identity(step, delay):
    return step == ONE and delay % ONE == 0


def _taps(n, step, delay, cut, j, H):
    """(i [J, 2H + 2] int64, d = |pos - (i << 24)| int64, inside [0, n) bool) of the warped samples j"""
    pos = np.asarray(j, np.int64) * np.int64(step) - np.int64(delay)
    i = (pos >> 24)[:, None] + np.arange(-H, H + 2, dtype=np.int64)[None, :]
    d = np.abs(pos[:, None] - (i << 24))
    return i, d, (i >= 0) & (i < n)


def wave_warp_emul(x, step, delay, j, cut=None, defect=None, corpus=None, samp0=0):
    """fp32 [len(j)]: warped samples j of the file x (fp32 numpy; int16 sources are dequantised by the caller, exactly).  corpus / samp0: the
    concatenated files and x's place in them (read only by the neighbour defect)."""
    assert defect is None or defect in DEFECTS
    x = np.asarray(x, F32)
    n = len(x)
    j = np.asarray(j, np.int64)
    out = np.zeros(len(j), F32)
    if not (STEP_MIN <= step <= STEP_MAX and 0 <= delay <= 1 << 48):
        return out
    cut = cut_of(step) if cut is None else F32(cut)
    if defect == 'rate_inverted':
        step = (1 << 48) // step
    npr = warp_len(n, step, delay) - (1 if defect == 'n_warped_off_by_one' else 0)
    ok = (j >= 0) & (j < npr)
    if is_identity(step, delay) and defect != 'identity_not_bypassed':
        i = j - (delay >> 24)
        ok &= (i >= 0) & (i < n)
        out[ok] = x[i[ok]]
        return out
    if defect == 'taps_not_scaled_by_cut':
        cut = F32(0.99)
    T = proto_table()
    # (the kernel walks H = (int)(Z / cut) + 2 <= H_MAX positions either side: a range that only has to cover the taps the test admits)
    i, d, inside = _taps(n, step, -delay if defect == 'delay_wrong_sign' else delay, cut, j, H_MAX)
    if defect == 'neighbour_samples_at_border':
        src, at = np.asarray(corpus, F32), i + samp0
        inside = (at >= 0) & (at < len(src))
    else:
        src, at = x, i
    s = np.where(inside, src[np.clip(at, 0, max(len(src) - 1, 0))] if len(src) else F32(0), F32(0)).astype(F32)
    q = d.astype(F32) * cut                                        # (float)d, then one product
    take = inside & (q <= F32(Z * ONE)) & ok[:, None]
    xq = np.minimum(q, F32(Z * ONE)) * F32(L / ONE)                 # (clipped only where the tap is not taken: the index stays inside the table)
    e = xq.astype(np.int32)
    f = xq - e.astype(F32)
    w = T[e] + f * (T[e + 1] - T[e])
    term = (w * cut) * s
    acc = np.zeros(len(j), F32)
    for k in range(i.shape[1]):                                     # increasing i, sequentially
        acc = np.where(take[:, k], acc + term[:, k], acc)
    return acc.astype(F32)


def wave_warp_ideal(x, step, delay, j, cut=None):
    """(ideal, bound) fp64 [len(j)]: the filter evaluated analytically on the fp32 source, and the derived per-sample bound (module docstring)"""
    x = np.asarray(x, F32).astype(np.float64)
    n = len(x)
    j = np.asarray(j, np.int64)
    ideal, bound = np.zeros(len(j)), np.zeros(len(j))
    if not (STEP_MIN <= step <= STEP_MAX and 0 <= delay <= 1 << 48):
        return ideal, bound
    ok = (j >= 0) & (j < warp_len(n, step, delay))
    if is_identity(step, delay):
        i = j - (delay >> 24)
        ok &= (i >= 0) & (i < n)
        ideal[ok] = x[i[ok]]
        return ideal, bound
    cut = float(cut_of(step) if cut is None else F32(cut))
    i, d, inside = _taps(n, step, delay, cut, j, H_MAX)
    u = d.astype(np.float64) * cut / ONE
    s = np.where(inside, x[np.clip(i, 0, max(n - 1, 0))] if n else 0.0, 0.0)
    p = proto(u)
    ideal = np.where(ok, (p * cut * s).sum(1), 0.0)
    near = u <= Z * (1 + 2.0 ** -20)
    bound = np.where(ok, (cut * np.abs(s) * near * (EPS_W + np.abs(p) * (K_MAX + 1) * 2.0 ** -24 * 1.01)).sum(1), 0.0)
    return ideal, bound


def staged_emul(x, file, step, delay, j, gain=None, noise_std=None, seed=0, defect=None, **kw):
    """the sample hftt_clip_logmel_warp stages: mix (clip_logmel_emul) of the warped sample, the noise keyed on (seed, file, j)"""
    w = wave_warp_emul(x, step, delay, j, defect=defect, **kw)
    j = np.asarray(j, np.int64)
    idx = j
    if defect == 'noise_keyed_on_source_index':
        idx = (j * np.int64(step) - np.int64(delay)) >> 24
    ok = (j >= 0) & (j < warp_len(len(x), step, delay))
    mixed = CE.mix(torch.from_numpy(w), file, gain, noise_std, seed, idx=idx).numpy()
    return np.where(ok, mixed, F32(0)).astype(F32)


def staged_ideal(x, file, step, delay, j, gain=None, noise_std=None, seed=0):
    ideal, bound = wave_warp_ideal(x, step, delay, j)
    j = np.asarray(j, np.int64)
    ok = (j >= 0) & (j < warp_len(len(x), step, delay))
    g = 1.0 if gain is None else float(F32(gain))
    nz = np.zeros(len(j)) if noise_std is None else CE.noise_term(seed, file, j, noise_std).astype(np.float64)
    out = np.where(ok, ideal * g + nz, 0.0)
    b = np.where(ok, g * bound + 2.0 ** -24 * 1.01 * (np.abs(ideal * g) * (gain is not None) + np.abs(out) * (noise_std is not None)), 0.0)
    return out, b


def violations(got, ideal, bound):
    """indices where |got - ideal| > bound (a NaN violates)"""
    err = np.abs(np.asarray(got, np.float64) - ideal)
    return np.nonzero(~(err <= bound))[0]


# ------------------------------------------------------------------------------------------------
# labels: the note list under the time map and the pitch shift, through the reference's note2label
LABEL_CFG = {'feature': {'sr': 16000, 'hop_sample': 256}, 'midi': {'note_min': 21, 'num_note': 88}}


def _note(pitch, onset, offset, velocity=64):
    return {'pitch': pitch, 'onset': onset, 'offset': offset, 'velocity': velocity}


# decimal times at least 1 us apart, so that the "no offset target" flags of the warped and the unwarped list agree; pitch 60 holds a repeated
# note whose offset is the next onset (no offset target) and two overlapping onsets; pitch 107 leaves the range under +3 and is not the last to end
LABEL_NOTES = [_note(60, 0.100001, 0.400002, 70), _note(60, 0.400002, 0.650003, 50), _note(23, 0.020004, 0.300005, 90), _note(107, 0.210006, 0.330007, 33),
               _note(64, 0.500008, 0.900009, 101), _note(60, 0.640011, 0.700012, 20)]
# a second file: long enough for two chunks of 256 frames, notes at both ends of the range
LABEL_NOTES_LONG = [_note(21, 0.000013, 0.250014, 11), _note(108, 0.300015, 4.700016, 127), _note(66, 4.100017, 5.200018, 64), _note(66, 5.200018, 5.300019, 65)]


def t_scale_of(step):
    return float(ONE) / float(step)


def t_delay_of(delay, sr):
    return float(delay) / float(ONE) / float(sr)


def warp_notes(notes, shift, t_delay, t_scale, note_min, N):
    """the list with t' = (t + t_delay) * t_scale (two fp64 roundings) and pitch + shift; a note shifted out of note_min .. note_min + N is dropped"""
    out = []
    for n in notes:
        p = n['pitch'] + shift
        if note_min <= p < note_min + N:
            out.append({'pitch': p, 'velocity': n['velocity'],
                        'onset': float((np.float64(n['onset']) + np.float64(t_delay)) * np.float64(t_scale)),
                        'offset': float((np.float64(n['offset']) + np.float64(t_delay)) * np.float64(t_scale))})
    return out


def labels_oracle(config, notes, shift, t_delay, t_scale, start, length, duration_tolerance=False):
    """(onset, offset fp32, mpe bool, velocity int8) [length, N]: frames start .. start + length of note2label_arrays on the warped list, zeros
    outside its frames.  The caller keeps the file's last-ending note inside the pitch range, so the list's frame count is the contract's."""
    from corpus.conv_note2label import note2label_arrays
    cm = config['midi']
    a = note2label_arrays(config, warp_notes(notes, shift, t_delay, t_scale, cm['note_min'], cm['num_note']), duration_tolerance)
    nf = a['onset'].shape[0]
    fr = start + np.arange(length)
    v = (fr >= 0) & (fr < nf)
    out = []
    for k in ('onset', 'offset', 'mpe', 'velocity'):
        t = np.zeros((length, cm['num_note']), a[k].dtype)
        t[v] = a[k][fr[v]]
        out.append(t)
    return tuple(out)
