"""fp32 restatement, fp64 reference and per-cell criterion of the clip log-mel, csrc/clip_logmel.hip: hftt_clip_logmel.

The contract (include/hftt_hip.h) says that column c of window b IS log-mel frame win_start[b] + c of file win_file[b]'s waveform alone, after
the int16 conversion, the per-window gain and the per-sample noise.  So the restatement is tests/frontend_emul.py's, file by file:

  mix             the sample in front of the window product: x (fp32, or int16 * 2^-15), fmul by the gain, fadd of the noise term; the counter
                  hash restated in numpy as tests/util.py::keep_mask restates it
  clip_logmel_emul   frontend_emul.logmel_emul of every (mixed) file, then the window / fill mapping; defect=<name> plants one wrong variant
  clip_logmel_expect / clip_logmel_check   frontend_emul.logmel_ref / logmel_bound of the (mixed) file's fp32 waveform, cell by cell -- NO new
                  tolerance: the bound is the one hftt_logmel carries -- and `==` on the bits of every fill cell

tests/test_clip_logmel_emul_bound.py shows on the CPU that the criterion passes the restatement on every scene below and fails every defect;
tests/test_clip_logmel_gpu.py holds the kernel to it on the same scenes.
"""
import functools

import numpy as np
import torch

import frontend_emul as FE

DEFECTS = ('neighbour_samples_at_border', 'frame_off_by_one', 'fill_on_the_wrong_side', 'last_frame_outside', 'win_file_ignored',
           'noise_keyed_clip_local', 'noise_keyed_frame_local', 'gain_after_noise', 'int16_scale_32767')

# the corpus: signals of frontend_emul.logmel_signal, concatenated in this order.  File 3 (constant 1.0: full scale) is directly followed by the
# silent file 4: one sample of bleed across that border lifts frame 0 of file 4 off logf(log_offset).
FILES = (('test_logmel_wave', 4219), ('impulse_last', 1), ('tone_0.3', 255), ('constant', 2047), ('zeros', 2304), ('noise_1e-4', 257),
         ('two_tone', 1023), ('nyquist', 256))
SILENT = 4
WIDTHS = (1, 21, 192)          # below, not a multiple of, and (the training width) twelve times the 16 frames a workgroup owns
FILL = -18.420681
# per width: scenes of B = 5 windows (file, first frame).  Frames per file: 17, 1, 1, 8, 10, 2, 4, 2.
SCENES = {
    # the last valid frame of the silent file; wholly before (negative); wholly behind (the first frame outside); the last valid frame of
    # file 0; the first window again (two overlapping windows of one file); window order is not file order
    1: [[(4, 9), (4, -1), (4, 10), (0, 16), (4, 9)],
        [(7, 0), (5, 1), (3, 0), (1, 0), (2, -1)]],
    # negative and straddling the last frame (file 4: frames -3 .. 17); straddling the last frame; overlapping the previous window; wholly
    # before; wholly behind
    21: [[(4, -3), (0, 5), (0, 0), (6, -21), (1, 1)],
         [(7, -2), (5, 0), (6, 1), (3, -20), (2, -7)]],
    192: [[(4, -5), (0, 3), (0, -100), (3, -192), (2, 1)],
          [(1, -64), (7, -190), (5, -32), (6, -1), (3, -96)]],
}
GAIN = (0.5, 1.75, 1.0, 0.25, 3.0)                     # per window
NOISE_STD = (1e-2, 1e-3, 0.0, 1e-4, 3e-2)              # (0.0: the term is an exact zero)
SEED = 0x1234_5678_9ABC_DEF1
NOISE_C = np.float32(1.0 / np.sqrt(np.float64(21845.0)))      # 1 / sqrt(21845), rounded once


def n_frames(n):
    return 1 + n // FE.HOP


@functools.lru_cache(maxsize=None)
def scene_waves():
    """the files as fp32 tensors (never written to)"""
    return tuple(FE.logmel_signal(s, n) for s, n in FILES)


def quantize_i16(w):
    """round(x * 32768) clipped to int16: what ops.WaveTable stores of a floating-point waveform"""
    return torch.round(w.double() * 32768.0).clamp(-32768, 32767).to(torch.int16)


def dequantize(q, scale=1.0 / 32768.0):
    return q.float() * np.float32(scale)                # (float)s * (1 / 32768): exact


def hash_u32(seed, site, idx):
    """numpy restatement of hftt_hash (csrc/hftt_common.h): a splitmix64 key over (seed, site), one 32-bit mixer per index"""
    M64, M32 = np.uint64, np.uint32
    with np.errstate(over='ignore'):
        k = M64(seed) + M64(0x9E3779B97F4A7C15) * M64(site + 1)
        k ^= k >> M64(30); k *= M64(0xBF58476D1CE4E5B9)
        k ^= k >> M64(27); k *= M64(0x94D049BB133111EB)
        k ^= k >> M64(31)
        idx = np.asarray(idx).astype(np.uint64)
        lo = (idx & M64(0xFFFFFFFF)).astype(np.uint32); hi = (idx >> M64(32)).astype(np.uint32)
        x = (lo + M32(int(k) & 0xFFFFFFFF)) ^ (hi ^ (hi << M32(16)))
        x ^= x >> M32(16); x *= M32(0x7FEB352D)
        x ^= x >> M32(15); x ^= M32(int(k) >> 32); x *= M32(0x846CA68B)
        x ^= x >> M32(16)
    return x


def noise_term(seed, file, idx, noise_std):
    """fmul((float)(b0 + b1 + b2 + b3 - 510), fmul(noise_std, C)) for the samples `idx` of file `file`, fp32 numpy"""
    h = hash_u32(seed, file, idx)
    s = ((h & 0xFF).astype(np.int64) + ((h >> 8) & 0xFF) + ((h >> 16) & 0xFF) + (h >> 24)) - 510
    return s.astype(np.float32) * (np.float32(noise_std) * NOISE_C)


def mix(x, file, gain=None, noise_std=None, seed=0, idx=None, gain_after_noise=False):
    """the samples that enter the window product: fp32 x -> fadd(fmul(x, gain), noise), each step one fp32 rounding and skipped when its
    operand is None.  idx: the index each sample is hashed with (default: its position inside the file)."""
    s = x.numpy().astype(np.float32)
    nz = None if noise_std is None else noise_term(seed, file, np.arange(len(s)) if idx is None else idx, noise_std)
    if gain is not None and not gain_after_noise:
        s = s * np.float32(gain)
    if nz is not None:
        s = s + nz
    if gain is not None and gain_after_noise:
        s = s * np.float32(gain)
    return torch.from_numpy(s.astype(np.float32))


def _per_window(v, b):
    return None if v is None else float(v[b])


def _file_wave(waves, f, wave_i16, scale=1.0 / 32768.0):
    return dequantize(waves[f], scale) if wave_i16 else waves[f]


def clip_logmel_emul(waves, t, windows, width, fill, wave_i16=False, gain=None, noise_std=None, seed=0, defect=None):
    """[B, n_mels, width] fp32: hftt_clip_logmel restated.  waves: the files (fp32, or int16 with wave_i16); windows: [(file, first frame)];
    gain / noise_std: per-window sequences or None."""
    assert defect is None or defect in DEFECTS
    hop, nfft = t['hop'], t['n_fft']
    pad = nfft // 2 // hop                              # frame t of a file = frame t + pad of the file with n_fft / 2 samples put in front
    out = torch.full((len(windows), t['n_mels'], width), fill, dtype=torch.float32)
    cache = {}

    def file_frames(f, g, s):
        """log-mel [frames, n_mels] of file f under this window's gain / noise"""
        key = (f, g, s)
        if key not in cache:
            x = _file_wave(waves, f, wave_i16, 1.0 / 32767.0 if defect == 'int16_scale_32767' else 1.0 / 32768.0)
            x = mix(x, f, g, s, seed, gain_after_noise=defect == 'gain_after_noise')
            if defect == 'neighbour_samples_at_border':        # the samples around the file come from the corpus, not from zeros
                allx = torch.cat([mix(_file_wave(waves, k, wave_i16), k, g, s, seed) for k in range(len(waves))])
                s0 = sum(len(w) for w in waves[:f])
                ext = torch.cat([torch.zeros(nfft // 2), allx, torch.zeros(nfft // 2)])[s0:s0 + len(x) + nfft]
                ext = ext.clone(); ext[nfft // 2:nfft // 2 + len(x)] = x
                cache[key] = FE.logmel_emul(ext, t)[pad:pad + n_frames(len(x))]
            else:
                cache[key] = FE.logmel_emul(x, t)
        return cache[key]

    for b, (f, start) in enumerate(windows):
        if defect == 'win_file_ignored':
            f = b % len(waves)
        g, s = _per_window(gain, b), _per_window(noise_std, b)
        n = len(waves[f])
        nf = n // hop if defect == 'last_frame_outside' else n_frames(n)
        cols = torch.arange(width)
        fr = start + cols + (1 if defect == 'frame_off_by_one' else 0)
        valid = (fr >= 0) & (fr < nf)
        if not bool(valid.any()):
            continue
        if defect in ('noise_keyed_clip_local', 'noise_keyed_frame_local') and s is not None:
            x = _file_wave(waves, f, wave_i16)
            i0 = start * hop - nfft // 2
            for c in cols[valid].tolist():               # the staged samples of the clip (of the frame), hashed with their position in it
                lo = i0 if defect == 'noise_keyed_clip_local' else i0 + c * hop
                span = (width - 1) * hop + nfft if defect == 'noise_keyed_clip_local' else nfft
                i = torch.arange(lo, lo + span)
                ok = (i >= 0) & (i < n)
                seg = torch.zeros(span)
                seg[ok] = mix(x[i[ok]], f, g, s, seed, idx=(i[ok] - lo).numpy())
                col = c if defect == 'noise_keyed_clip_local' else 0
                out[b, :, c] = FE.logmel_emul(seg, t)[pad + col]
            continue
        feat = file_frames(f, g, s)
        if defect == 'fill_on_the_wrong_side':           # the fill sits at the other end of the window
            valid = valid.flip(0)
            fr = fr.clamp(0, nf - 1)
        out[b][:, valid] = feat[fr[valid].clamp(0, feat.shape[0] - 1)].T
    return out


def clip_logmel_expect(waves, t, windows, width, wave_i16=False, gain=None, noise_std=None, seed=0):
    """dict(ref, up, down fp64 [B, n_mels, width]; valid bool [B, width]): frontend_emul.logmel_ref and logmel_bound of each window's file --
    the dequantised, gained and noised fp32 waveform, mixed by `mix` -- at the window's frames.  Cells outside `valid` are fill cells."""
    B, M = len(windows), t['n_mels']
    ref = torch.zeros(B, M, width, dtype=torch.float64)
    up, down = torch.zeros_like(ref), torch.zeros_like(ref)
    valid = torch.zeros(B, width, dtype=torch.bool)
    cache = {}
    for b, (f, start) in enumerate(windows):
        key = (f, _per_window(gain, b), _per_window(noise_std, b))
        if key not in cache:
            r = FE.logmel_ref(mix(_file_wave(waves, f, wave_i16), f, key[1], key[2], seed), t)
            cache[key] = (r['out'],) + FE.logmel_bound(r)
        o, u, d = cache[key]
        fr = start + torch.arange(width)
        v = (fr >= 0) & (fr < o.shape[0])
        valid[b] = v
        for dst, src in ((ref, o), (up, u), (down, d)):
            dst[b][:, v] = src[fr[v]].T
    return dict(ref=ref, up=up, down=down, valid=valid)


def clip_logmel_check(got, exp, fill):
    """violations: (kind, b, m, c, got, expected) of the worst cells -- a valid cell outside -down <= got - ref <= up (NaN violates), a fill cell
    whose bits are not the fill's; a wrong shape.  Empty = pass; no cell is excluded."""
    if tuple(got.shape) != tuple(exp['ref'].shape):
        return [('shape', -1, -1, -1, tuple(got.shape), tuple(exp['ref'].shape))]
    got = got.detach().cpu()
    valid = exp['valid'][:, None, :].expand_as(exp['ref'])
    err = got.double() - exp['ref']
    bad_valid = valid & ~torch.where(err >= 0, err <= exp['up'], -err <= exp['down'])
    fill_bits = torch.tensor(fill, dtype=torch.float32).view(torch.int32)
    bad_fill = ~valid & (got.contiguous().view(torch.int32) != fill_bits)
    out = []
    for kind, bad in (('valid', bad_valid), ('fill', bad_fill)):
        for b, m, c in bad.nonzero()[:4].tolist():
            out.append((kind, b, m, c, float(got[b, m, c]), float(exp['ref'][b, m, c]) if kind == 'valid' else fill))
        if int(bad.sum()) > 4:
            out.append((kind, 'and %d more' % (int(bad.sum()) - 4), -1, -1, 0.0, 0.0))
    return out


def clip_logmel_ratio(got, exp):
    """worst |error| / bound over the valid cells (reported, not asserted); 0.0 without valid cells"""
    valid = exp['valid'][:, None, :].expand_as(exp['ref'])
    if not bool(valid.any()):
        return 0.0
    err = got.detach().cpu().double() - exp['ref']
    return float((err.abs() / torch.where(err >= 0, exp['up'], exp['down']))[valid].max())
