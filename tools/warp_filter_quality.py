#!/usr/bin/env python3
"""Passband droop and alias / image rejection of the warp's resampling filter (include/hftt_hip.h: Hann-windowed sinc, Z = 6 zero crossings,
rolloff 0.99, scaled to the cutoff), evaluated in fp64 on the CPU -- no table, no device: the figures are properties of the filter chosen, not
tolerances of any test.

  python tools/warp_filter_quality.py [--out profiles/warp_filter_quality.txt]

For the rates r = 2^(+-2/12) a tone of frequency f (in units of the source's Nyquist rate) is played back at rate r: the warped signal should
hold one tone at f r (units of its own Nyquist rate) when f r < 1, and nothing when f r >= 1 (the tone would alias).  A least-squares fit of
the sine and cosine at f r gives the gain of the wanted tone; what remains after it is subtracted is images, aliases and the filter's ripple."""
import argparse
import os

import numpy as np

Z, ROLLOFF = 6, 0.99


def warp_ideal(x, r, delay=0.0):
    """y[j] = sum_i x[i] cut p((j r - delay - i) cut), p(u) = sinc(u) cos^2(pi u / 2Z) on |u| < Z, cut = ROLLOFF min(1, 1 / r)"""
    cut = ROLLOFF * min(1.0, 1.0 / r)
    n2 = int(np.floor((len(x) - 1 + delay) / r)) + 1
    pos = np.arange(n2) * r - delay
    H = int(Z / cut) + 2
    i = np.floor(pos).astype(np.int64)[:, None] + np.arange(-H, H + 2)[None, :]
    u = (pos[:, None] - i) * cut
    p = np.where(np.abs(u) < Z, np.sinc(u) * np.cos(np.pi * u / (2 * Z)) ** 2, 0.0)
    ok = (i >= 0) & (i < len(x))
    return (p * cut * np.where(ok, x[np.clip(i, 0, len(x) - 1)], 0.0)).sum(1)


def tone_response(f, r, n=8192):
    """(gain of the tone at f r, rms of the rest) relative to the input tone's amplitude, away from the ends of the file"""
    x = np.sin(np.pi * f * np.arange(n) + 0.3)
    y = warp_ideal(x, r, delay=0.37)[64:-64]
    j = np.arange(64, 64 + len(y))
    fo = f * r
    if fo >= 1.0:
        return 0.0, float(np.sqrt(2.0 * np.mean(y ** 2)))
    A = np.stack([np.sin(np.pi * fo * j), np.cos(np.pi * fo * j)], 1)
    c, *_ = np.linalg.lstsq(A, y, rcond=None)
    rest = y - A @ c
    return float(np.hypot(*c)), float(np.sqrt(2.0 * np.mean(rest ** 2)))


def db(v):
    return 20.0 * np.log10(max(v, 1e-300))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='profiles/warp_filter_quality.txt')
    args = ap.parse_args()
    lines = ['warp resampling filter, fp64, Z = %d, rolloff %.2f: tone at f (source Nyquist = 1) played back at rate r' % (Z, ROLLOFF)]
    for semis in (2, -2):
        r = 2.0 ** (semis / 12.0)
        edge = min(1.0, 1.0 / r)                        # the highest source frequency that still fits under the warped Nyquist rate
        lines.append('r = 2^(%+d/12) = %.6f, cutoff %.4f of the source Nyquist rate' % (semis, r, ROLLOFF * edge))
        for frac in (0.1, 0.25, 0.5, 0.7, 0.8, 0.9, 0.95):
            g, rest = tone_response(frac * edge, r)
            lines.append('  f = %.2f of the band edge: gain %+.3f dB, everything else %.1f dB' % (frac, db(g), db(rest)))
        sweep = np.linspace(0.02, 0.8, 79) * edge
        res = [tone_response(f, r) for f in sweep]
        lines.append('  sweep 0.02 .. 0.80 of the band edge: worst droop %+.3f dB, worst residue %.1f dB' % (min(db(g) for g, _ in res), max(db(b) for _, b in res)))
        if r > 1.0:                                     # tones that must not survive: f r >= 1
            for f in (1.0 / r + 0.02, 1.0 / r + 0.05, 1.0 / r + 0.1, 0.999):
                if f < 1.0:
                    lines.append('  f = %.3f (would alias to %.3f): %.1f dB left' % (f, 2.0 - f * r, db(tone_response(f, r)[1])))
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(text)
    print(text, end='')


if __name__ == '__main__':
    main()
