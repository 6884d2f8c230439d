"""fp32 restatements, fp64 references and rounding-model criteria of the audio front end, csrc/logmel.hip (hftt_logmel and hftt_resample) and
the frame transform it shares with the clip log-mel, csrc/logmel_frame.h.

As in tests/elementwise_emul.py, three things per kernel, all in torch and device-agnostic:

  *_ref    the fp64 evaluation of the same operation on the same, already rounded, fp32 inputs and tables (ops.LogMel.tables, the fp32
           kernel table of ops.resample_kernel_table), plus the magnitudes the bound needs;
  *_emul   the kernel's arithmetic in fp32 in the kernel's order (packing, five radix-4 Stockham stages, the split pass, the sequential CSR
           sum, logf; four interleaved fma accumulators for the resampler); defect=<name> selects one deliberately wrong variant;
  *_check  |got - ref| <= bound element by element, no element excluded; returns the list of violations (empty = pass).

The bounds are first-order rounding models: U32 = 2^-24 per fp32 rounding times a count read off the source (the function or kernel is cited
by name beside each count) times the magnitude the rounding acts on.  The device contracts a * b + c into one fma where it can; that removes roundings, so the
counts (no contraction) hold for either code.  tests/test_frontend_emul_bound.py shows on the CPU what the criteria resolve;
tests/test_frontend_fp64_gpu.py holds the kernels to them.
"""
import math

import torch

from elementwise_emul import U32, F32_TINY, C_LOG, f32, violations      # noqa: F401  (U32, F32_TINY re-exported to the tests)

LOGMEL_DEFECTS = ('odd_sample_uses_even_window', 'last_sample_dropped', 'frame_start_off_by_one', 'split_twiddle_conjugated',
                  'second_half_turn_sign', 'mel_last_weight_dropped', 'offset_inside_the_sum', 'frames_floor_of_n_minus_1')
RESAMPLE_DEFECTS = ('phase_row_off_by_one', 'window_base_ignores_width', 'tail_taps_dropped', 'block_window_one_frame_short')

N_FFT, HOP, LOG_OFFSET = 2048, 256, 1e-8


def logmel_tables():
    """the tables of ops.LogMel as host tensors + hop, n_fft, n_mels and the fp32 log offset (how the descriptor's float field holds it)"""
    from hftt_hip import ops
    t = ops.LogMel.tables(16000, N_FFT, 256)
    t.update(hop=HOP, n_fft=N_FFT, n_mels=256, log_offset=f32(LOG_OFFSET))
    return t


def tables_to(t, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in t.items()}


def _fb_dense(t, dtype, drop_last=False):
    """the CSR filterbank as a dense [n_fft / 2 + 1, n_mels] matrix (for the fp64 reference and the bound: a sum's order does not matter there)"""
    dev = t['fb_w'].device
    W = torch.zeros(t['n_fft'] // 2 + 1, t['n_mels'], dtype=dtype, device=dev)
    st, ln, off = t['fb_start'].tolist(), t['fb_len'].tolist(), t['fb_off'].tolist()
    for m in range(t['n_mels']):
        n = ln[m] - (1 if drop_last else 0)
        if n > 0:
            W[st[m]:st[m] + n, m] = t['fb_w'][off[m]:off[m] + n].to(dtype)
    return W


def n_frames_of(n, hop=HOP):
    return 1 + n // hop


def _frames(wave, t, n_frames, start_shift=0):
    """[n_frames, n_fft] samples of the centred, zero-padded frames (logmel_kernel, frame start and packing: start = frame * hop - n_fft / 2) and their validity"""
    n = wave.numel()
    idx = (torch.arange(n_frames, device=wave.device)[:, None] * t['hop'] - t['n_fft'] // 2 + start_shift
           + torch.arange(t['n_fft'], device=wave.device)[None, :])
    ok = (idx >= 0) & (idx < n)
    return torch.where(ok, wave[idx.clamp(0, n - 1)], torch.zeros((), dtype=wave.dtype, device=wave.device)), ok, idx


# ================================================================================================ log-mel: fp64 reference
def logmel_ref(wave, t):
    """fp64: frame x fp32 window, torch.fft.rfft, |X|^2, the filterbank sum, log(. + offset), on the device of `wave`.  Also the magnitudes
    of the bound: l1 = sum |x w| and l2 = ||x w||_2 per frame, |X_k|, p_k, the mel sum and W (dense fp64)."""
    wave = wave.detach().reshape(-1)
    assert wave.dtype == torch.float32
    F = n_frames_of(wave.numel(), t['hop'])
    fr, _, _ = _frames(wave, t, F)
    xw = fr.double() * t['window'].double()[None, :]
    X = torch.fft.rfft(xw, dim=1)
    p = X.real ** 2 + X.imag ** 2
    W = _fb_dense(t, torch.float64)
    mel = p @ W
    return dict(out=torch.log(mel + t['log_offset']), l1=xw.abs().sum(1), l2=xw.pow(2).sum(1).sqrt(), absX=X.abs(), p=p, mel=mel, W=W,
                fb_len=t['fb_len'].double(), offset=t['log_offset'])


# ================================================================================================ log-mel: the kernel in fp32
def _cmul(ax, ay, wx, wy):                     # logmel_frame.h: frame_cmul, without contraction: two products and one sum per component
    return ax * wx - ay * wy, ax * wy + ay * wx


def logmel_emul(wave, t, defect=None):
    """logmel_kernel<2048> in fp32, vectorised over the frames (each frame is one workgroup; thread j of a stage is column j here)"""
    assert defect is None or defect in LOGMEL_DEFECTS
    wave = wave.detach().reshape(-1).float()
    dev = wave.device
    n, NFFT, hop = wave.numel(), t['n_fft'], t['hop']
    N, Q = NFFT // 2, NFFT // 8
    F = 1 + ((n - 1) // hop if defect == 'frames_floor_of_n_minus_1' else n // hop)
    fr, ok, idx = _frames(wave, t, F, start_shift=1 if defect == 'frame_start_off_by_one' else 0)
    win = t['window']
    # packing (logmel_kernel): z[n] = x[2n] w[2n] + i x[2n + 1] w[2n + 1], each slot with its own bounds test
    xe = fr[:, 0::2] * win[None, 0::2]
    w_odd = win[None, 0::2] if defect == 'odd_sample_uses_even_window' else win[None, 1::2]
    odd = fr[:, 1::2]
    if defect == 'last_sample_dropped':        # s0 + 1 < n - 1
        odd = torch.where(idx[:, 1::2] < n - 1, odd, torch.zeros((), device=dev))
    xo = odd * w_odd
    zero = torch.zeros((), device=dev)
    re, im = torch.where(ok[:, 0::2], xe, zero), torch.where(ok[:, 1::2], xo, zero)      # (an out-of-range slot is 0, not wave * window)
    tc, ts = t['twiddle'][:N], t['twiddle'][N:]

    def tw(m, split=False):                    # logmel_frame.h: frame_tw: e^(-2 pi i m / 2048); the second half turn is a sign
        mm = m & (N - 1)
        c, sn = tc[mm], ts[mm]
        second = (m & N) != 0
        if defect == 'second_half_turn_sign':
            second = torch.zeros_like(second)
        wx, wy = torch.where(second, -c, c), torch.where(second, sn, -sn)
        if split and defect == 'split_twiddle_conjugated':
            wy = -wy
        return wx[None, :], wy[None, :]

    j = torch.arange(Q, device=dev)
    Ns = 1
    while Ns < N:                              # logmel_frame.h: frame_stage, once per Ns (the stage loop of both kernels)
        k = j & (Ns - 1)
        step = NFFT // (4 * Ns)
        v = [(re[:, j + q * Q], im[:, j + q * Q]) for q in range(4)]
        if Ns > 1:
            for q in (1, 2, 3):
                v[q] = _cmul(v[q][0], v[q][1], *tw(q * k * step))
        a02 = (v[0][0] + v[2][0], v[0][1] + v[2][1]); s02 = (v[0][0] - v[2][0], v[0][1] - v[2][1])
        a13 = (v[1][0] + v[3][0], v[1][1] + v[3][1]); s13 = (v[1][0] - v[3][0], v[1][1] - v[3][1])
        j0 = ((j - k) << 2) + k
        nre, nim = torch.empty_like(re), torch.empty_like(im)
        nre[:, j0] = a02[0] + a13[0]; nim[:, j0] = a02[1] + a13[1]
        nre[:, j0 + Ns] = s02[0] + s13[1]; nim[:, j0 + Ns] = s02[1] - s13[0]
        nre[:, j0 + 2 * Ns] = a02[0] - a13[0]; nim[:, j0 + 2 * Ns] = a02[1] - a13[1]
        nre[:, j0 + 3 * Ns] = s02[0] - s13[1]; nim[:, j0 + 3 * Ns] = s02[1] + s13[0]
        re, im = nre, nim
        Ns *= 4
    # logmel_frame.h: frame_split, split pass and power, k = 0 .. N with Z[N] = Z[0]
    kk = torch.arange(N + 1, device=dev)
    zkx, zky = re[:, kk & (N - 1)], im[:, kk & (N - 1)]
    znx, zny = re[:, (N - kk) & (N - 1)], im[:, (N - kk) & (N - 1)]
    ex, ey = 0.5 * (zkx + znx), 0.5 * (zky - zny)
    ox, oy = 0.5 * (zky + zny), -0.5 * (zkx - znx)
    wox, woy = _cmul(ox, oy, *tw(kk, split=True))
    xr, xi = ex + wox, ey + woy
    pw = xr * xr + xi * xi
    # logmel_frame.h: frame_mel, the CSR sum in sequence
    st, ln, off = t['fb_start'].long(), t['fb_len'].long(), t['fb_off'].long()
    if defect == 'mel_last_weight_dropped':
        ln = ln - 1
    offset = torch.tensor(t['log_offset'], dtype=torch.float32, device=dev)
    acc = torch.zeros(F, t['n_mels'], device=dev)
    for jj in range(int(ln.max())):
        live = jj < ln
        term = t['fb_w'][(off + jj).clamp_max(t['fb_w'].numel() - 1)][None, :] * pw[:, (st + jj).clamp_max(N)]
        if defect == 'offset_inside_the_sum':
            term = term + offset
        acc = torch.where(live[None, :], acc + term, acc)
    return torch.log(acc if defect == 'offset_inside_the_sum' else acc + offset)


# ================================================================================================ log-mel: the criterion
# Delta X_k, in U32 of the frame's magnitude S (below), along the longest path from a sample to X_k:
#   window product (logmel_kernel, packing; clip_logmel_kernel packs with the same product)                                    1
#   frame_stage, Ns = 1 (no twiddle): a02 / s02 / a13 / s13, then the sum of two of them: two additions                         2
#   frame_stage, Ns = 4 .. 256: frame_cmul = product + sum 2, frame_tw's two table entries 2, two additions 2        = 6, x 4   24
#   frame_split: e or o 1 (the halving is exact), frame_cmul 2, frame_tw's two table entries 2, e + wo 1                        6
C_FFT = 1 + 2 + 4 * 6 + 6
# The magnitude S.  'l1': sum |x w| of the frame -- every rounding of every path with the same sign: a bound in the strict sense, and the
# criterion.  'l2': ||x w||_2 -- the count still linear along a path, the 2048 paths into one bin added as independent terms -- is the
# tighter, statistical form; tests/test_frontend_emul_bound.py records what share of the cells each leaves open.
LOGMEL_NORM = 'l1'
# p_k = xr * xr + xi * xi (frame_split, power): two products and a sum, 3 U32 of p_k at most
C_POW = 3


def logmel_bound(ref, norm=LOGMEL_NORM, c_fft=C_FFT, c_pow=C_POW, c_sum=None, c_log=C_LOG):
    """(upward, downward) bounds of got - ref, each [n_frames, n_mels]:
      Delta X_k  <= c_fft U32 S;   Delta p_k <= 2 |X_k| Delta X_k + Delta X_k^2 + c_pow U32 p_k  (+ F32_TINY: a product below the normal range)
      Delta mel  <= sum_j w_j Delta p_j + c_sum U32 sum_j w_j p_j, c_sum = len + 1      (frame_mel: the product w * p 1, len additions in sequence)
      log domain: up = log1p(r), r = Delta mel / (mel + offset); down = -log1p(-r), and never below log(offset): pw and the weights are
      >= 0, so acc >= 0 and got >= logf(offset) -- that guards r >= 1;  + c_log U32 |log| for logf and 1 U32 for acc + offset (frame_mel)."""
    S = (ref['l2'] if norm == 'l2' else ref['l1'])[:, None]
    dX = c_fft * U32 * S
    dp = 2 * ref['absX'] * dX + dX * dX + c_pow * U32 * ref['p'] + F32_TINY
    c_sum = ref['fb_len'][None, :] + 1 if c_sum is None else c_sum
    dmel = dp @ ref['W'] + c_sum * U32 * ref['mel']
    tot = ref['mel'] + ref['offset']
    r = dmel / tot
    add = c_log * U32 * ref['out'].abs() + U32
    up = torch.log1p(r)
    floor = torch.log1p(ref['mel'] / ref['offset'])
    down = torch.where(r < 1, -torch.log1p(-r.clamp_max(1 - 1e-16)), floor)
    return up + add, torch.minimum(down, floor) + add


def logmel_check(got, ref, **kw):
    """violations of -down <= got - ref <= up, every element; a wrong shape, NaN and Inf violate"""
    if tuple(got.shape) != tuple(ref['out'].shape):
        return [('logmel: shape %s, expected %s' % (tuple(got.shape), tuple(ref['out'].shape)), -1, float('nan'), 0.0, got.numel())]
    up, down = logmel_bound(ref, **kw)
    err = got.detach().to(ref['out'].device).double() - ref['out']
    bound = torch.where(err >= 0, up, down)
    return violations('logmel', err, torch.zeros_like(err), bound)


def logmel_ratio(got, ref, **kw):
    """worst |error| / bound (the margin the model leaves: reported, not asserted)"""
    up, down = logmel_bound(ref, **kw)
    err = got.detach().to(ref['out'].device).double() - ref['out']
    return float((err.abs() / torch.where(err >= 0, up, down)).max())


# ------------------------------------------------------------------------------------------------ log-mel: the cases
LOGMEL_LENGTHS = (1, 255, 256, 257, 1023, 1024, 1025, 2047, 2304, 4219)
TONE = 64.0 / 2048.0          # cycles per sample: bin 64 of the 2048-point frame, no leakage past the window's main lobe in interior frames
# signal -> the lengths it is crossed with: each has an odd length and a multiple of hop; together every length is run
LOGMEL_CASES = {
    'zeros':            (1, 256, 1025, 4219),
    'impulse_first':    (1, 255, 1024, 2304),
    'impulse_last':     (1, 257, 1024, 2047, 2304),
    'impulse_mid':      (255, 1023, 2304, 4219),
    'tone_1e-3':        (257, 1024, 4219),
    'tone_0.3':         (255, 2304, 4219),
    'tone_30':          (1023, 1024, 4219),
    'two_tone':         (1025, 2304, 4219),
    'constant':         (1, 256, 2047, 4219),
    'nyquist':          (255, 256, 1025, 4219),
    'noise_1e-4':       (257, 2047, 2304, 4219),
    'test_logmel_wave': (1023, 1024, 1025, 4219),
}


def logmel_cases():
    return [(s, n) for s, ns in LOGMEL_CASES.items() for n in ns]


def logmel_signal(name, n):
    """fp32 [n], evaluated in fp64 and rounded once"""
    i = torch.arange(n, dtype=torch.float64)
    x = torch.zeros(n, dtype=torch.float64)
    if name == 'impulse_first':
        x[0] = 1.0
    elif name == 'impulse_last':
        x[n - 1] = 1.0
    elif name == 'impulse_mid':
        x[n // 2] = 1.0
    elif name.startswith('tone_'):
        x = float(name[5:]) * torch.sin(2 * math.pi * TONE * i)
    elif name == 'two_tone':
        x = torch.sin(2 * math.pi * TONE * i) + 1e-4 * torch.sin(2 * math.pi * (700.0 / 2048.0) * i)
    elif name == 'constant':
        x = torch.ones(n, dtype=torch.float64)
    elif name == 'nyquist':
        x = 1.0 - 2.0 * (i % 2)
    elif name == 'noise_1e-4':
        x = 1e-4 * torch.randn(n, generator=torch.Generator().manual_seed(n), dtype=torch.float64)
    elif name == 'test_logmel_wave':           # tests/test_kernels_gpu.py::test_logmel, its first n samples
        g = torch.Generator().manual_seed(5)
        full = 16000 * 2 + 123
        tt = torch.arange(full) / 16000.0
        w = 0.3 * torch.sin(2 * math.pi * 220.0 * tt) * torch.exp(-2.0 * tt) + 0.1 * torch.sin(2 * math.pi * 1760.0 * tt) + 0.01 * torch.randn(full, generator=g)
        return w[:n].float().contiguous()
    else:
        assert name == 'zeros', name
    return x.float()


# ================================================================================================ resampler
RESAMPLE_RATES = (44100, 48000, 22050, 32000, 8000, 11025, 96000)
RESAMPLE_N_OUT = (255, 256, 257, 513)          # around the 256 outputs of a workgroup (olast, f1 and wlen of resample_kernel), and a third block


def resample_table(sr_in, sr_out=16000):
    """(fp32 kernel table [up, taps] as the device holds it, up, down, width)"""
    from hftt_hip import ops
    kern, up, down, width = ops.resample_kernel_table(sr_in, sr_out)
    return kern.float().contiguous(), up, down, width


def resample_n_out(n, up, down):
    return -(-n * up // down)


def resample_lengths(up, down, taps):
    """1, 2, down - 1, down, down + 1, taps - 1 and, for each T of RESAMPLE_N_OUT, the smallest n whose n_out reaches T (n_out = T wherever a
    length gives it: up-sampling steps n_out by more than one, 8000 -> 16000 gives 256 / 258 / 514); n >= 1, without repeats"""
    ns = [1, 2, down - 1, down, down + 1, taps - 1] + [(T - 1) * down // up + 1 for T in RESAMPLE_N_OUT]
    out = []
    for n in ns:
        if n >= 1 and n not in out:
            out.append(n)
    for T, n in zip(RESAMPLE_N_OUT, ns[6:]):
        assert T <= resample_n_out(n, up, down) < T + max(1, -(-up // down)) and resample_n_out(n - 1, up, down) < T
    return out


def _resample_index(n_out, up, down, width, taps, dev, base_shift=0):
    o = torch.arange(n_out, device=dev)
    f, ph = o // up, o % up
    s = (f * down - width + base_shift)[:, None] + torch.arange(taps, device=dev)[None, :]      # [n_out, taps] input sample of tap t
    return f, ph, s


def resample_ref(wave, kern, up, down, width):
    """fp64 polyphase sum on the fp32 table: out[o] = sum_t x[(o / up) down - width + t] kernel[o % up][t]; and sum_t |x k| for the bound"""
    wave = wave.detach().reshape(-1)
    n, taps = wave.numel(), kern.shape[1]
    n_out = resample_n_out(n, up, down)
    _, ph, s = _resample_index(n_out, up, down, width, taps, wave.device)
    ok = (s >= 0) & (s < n)
    x = torch.where(ok, wave.double()[s.clamp(0, n - 1)], torch.zeros((), dtype=torch.float64, device=wave.device))
    prod = x * kern.to(wave.device).double()[ph]
    return dict(out=prod.sum(1), scale=prod.abs().sum(1), taps=taps)


def _fma(a, b, c):
    """fmaf on fp32 tensors: the product of two fp32 is exact in fp64; the sum is rounded to fp64, then to fp32 (a double rounding only at
    an fp64 tie: the criterion does not rest on the last bit)"""
    return (a.double() * b.double() + c.double()).float()


def resample_emul(wave, kern, up, down, width, defect=None):
    """resample_kernel (logmel.hip) in fp32: four interleaved fma accumulators over the taps, a0 takes the tail, (a0 + a1) + (a2 + a3)"""
    assert defect is None or defect in RESAMPLE_DEFECTS
    wave = wave.detach().reshape(-1).float()
    dev = wave.device
    n, taps = wave.numel(), kern.shape[1]
    n_out = resample_n_out(n, up, down)
    f, ph, s = _resample_index(n_out, up, down, width, taps, dev, base_shift=width if defect == 'window_base_ignores_width' else 0)
    if defect == 'phase_row_off_by_one':
        ph = (ph + 1) % up
    ok = (s >= 0) & (s < n)
    if defect == 'block_window_one_frame_short':        # wlen = (f1 - f0) * down + taps - down: what lies past it is not staged (read as 0 here)
        o = torch.arange(n_out, device=dev)
        o0 = o // 256 * 256
        olast = torch.clamp(o0 + 255, max=n_out - 1)
        f0, f1 = o0 // up, olast // up
        wlen = (f1 - f0) * down + taps - down
        ok = ok & (((f - f0) * down)[:, None] + torch.arange(taps, device=dev)[None, :] < wlen[:, None])
    w = torch.where(ok, wave[s.clamp(0, n - 1)], torch.zeros((), device=dev))
    k = kern.to(dev)[ph]
    a = [torch.zeros(n_out, device=dev) for _ in range(4)]
    t = 0
    while t + 4 <= taps:
        for q in range(4):
            a[q] = _fma(w[:, t + q], k[:, t + q], a[q])
        t += 4
    if defect != 'tail_taps_dropped':
        while t < taps:
            a[0] = _fma(w[:, t], k[:, t], a[0])
            t += 1
    return (a[0] + a[1]) + (a[2] + a[3])


def resample_bound(ref):
    """an accumulator takes taps / 4 fma of one rounding each (resample_kernel, the tap loop), then two additions (its last line): (taps / 4 + 2) U32 of
    sum |x_t k_t|, + F32_TINY for a result below the normal range.  (The count charges every term the whole chain; only a chain's first
    term passes all of it, so the <= 3 tail taps of a0 (the loop behind the unrolled one), whose table entries are the smallest of the row, fit inside.)"""
    return (ref['taps'] / 4 + 2) * U32 * ref['scale'] + F32_TINY


def resample_check(got, ref):
    if tuple(got.shape) != tuple(ref['out'].shape):
        return [('resample: shape %s, expected %s' % (tuple(got.shape), tuple(ref['out'].shape)), -1, float('nan'), 0.0, got.numel())]
    return violations('resample', got, ref['out'], resample_bound(ref))


def resample_ratio(got, ref):
    err = (got.detach().to(ref['out'].device).double() - ref['out']).abs()
    return float((err / resample_bound(ref)).max())


def resample_impulse_expected(kern, up, down, width, n, s_imp):
    """the response to a unit impulse at sample s_imp, to the bit: kernel[o % up][s_imp - ((o / up) down - width)], +0.0 outside [0, taps).
    (fmaf(1, k, 0) = k and every other tap adds an exact zero; `+ 0.0` is what the sum of the four accumulators makes of a table entry of
    -0.0: the outermost taps underflow to it.)"""
    taps = kern.shape[1]
    n_out = resample_n_out(n, up, down)
    o = torch.arange(n_out)
    tap = s_imp - ((o // up) * down - width)
    ok = (tap >= 0) & (tap < taps)
    return torch.where(ok, kern[o % up, tap.clamp(0, taps - 1)], torch.zeros(())) + 0.0


def resample_noise(n, seed):
    return (torch.rand(n, generator=torch.Generator().manual_seed(seed)) * 2 - 1).float()
