"""hftt_clip_room restated on the host (a helper, not a test): the fp64 convolution of given fp32 dry samples and taps with its worst-case
fp32 bound, the pseudo-file tables in plain Python, and an fp64 log-mel frame picking that follows hftt_clip_logmel's rule for which column
is a frame and which is fill -- enough to show that the tables make a plain clip log-mel over the scratch see the whole wet file."""
import numpy as np

HOP, NFFT, WIDTH = 256, 2048, 20
FILL = -18.420681
LENS = (9000, 700, 0)                       # the common corpus: noise, a file shorter than most responses, an empty file
# (file, first frame): from frame -3 of file 0; over file 0's end; wholly behind it; the short file; the empty file; no file
WINDOWS = ((0, -3), (0, 25), (0, 40), (1, 0), (2, 0), (-1, 0))
U = 2.0 ** -24


def corpus_waves(seed=11):
    """the three files as fp32: uniform noise at amplitude 0.5"""
    r = np.random.RandomState(seed)
    return [r.uniform(-0.5, 0.5, n).astype(np.float32) for n in LENS]


def quantize_i16(w):
    return np.clip(np.round(w.astype(np.float64) * 32768.0), -32768, 32767).astype(np.int16)


def dequantize(q):
    return (q.astype(np.float32) * np.float32(1.0 / 32768.0)).astype(np.float32)


def gamma(n):
    """the worst-case relative error of an n-term fp32 dot product in any order, with or without fma"""
    return n * U / (1.0 - n * U)


def wet_ref(dry, h, taps=None):
    """fp64 [n]: sum over k < taps of h[k] dry[i - k], the tail behind the file's end cut; and the bound's sum of |h[k]| |dry[i - k]|"""
    dry, h = np.asarray(dry, np.float32).astype(np.float64), np.asarray(h, np.float32).astype(np.float64)
    taps = len(h) if taps is None else min(max(int(taps), 1), len(h))
    n = len(dry)
    if n == 0:
        return np.zeros(0), np.zeros(0)
    return np.convolve(dry, h[:taps])[:n], np.convolve(np.abs(dry), np.abs(h[:taps]))[:n]


def wet_bound(mag, taps):
    """gamma(taps) * sum |h| |dry| + taps * 2^-126: a worst-case bound, so it takes no further margin"""
    return gamma(taps) * mag + taps * 2.0 ** -126


def wet_fp32(dry, h, taps=None, reverse=False):
    """the convolution in fp32 numpy, one fixed tap order: forward (k = 0 first) or reverse"""
    dry, h = np.asarray(dry, np.float32), np.asarray(h, np.float32)
    taps = len(h) if taps is None else min(max(int(taps), 1), len(h))
    n = len(dry)
    acc = np.zeros(n, np.float32)
    for k in (range(taps - 1, -1, -1) if reverse else range(taps)):
        if k < n:
            acc[k:] = acc[k:] + h[k] * dry[:n - k]
    return acc


def lead(hop=HOP, n_fft=NFFT):
    return -(-(n_fft // 2) // hop)


def span_of(width=WIDTH, hop=HOP, n_fft=NFFT):
    return (lead(hop, n_fft) + width - 1) * hop + n_fft // 2


def pseudo_tables(n_prime, win_start, width=WIDTH, hop=HOP, n_fft=NFFT, span=None):
    """n_prime[b]: samples of window b's (warped) file, negative for a window without a valid file, warp or response.  -> dict(o, e [B]: the
    pseudo-file's extent in the wet file; samp0 int64 [2 B + 1], win_file, win_start int32 [B]: what the kernel writes)"""
    span = span_of(width, hop, n_fft) if span is None else span
    B, P = len(n_prime), lead(hop, n_fft)
    o, e = np.zeros(B, np.int64), np.zeros(B, np.int64)
    samp0, wf, ws = np.zeros(2 * B + 1, np.int64), np.zeros(B, np.int32), np.zeros(B, np.int32)
    for b in range(B):
        s, n = int(win_start[b]), int(n_prime[b])
        o[b] = max(0, s - P) * hop
        e[b] = min(n, (s + width - 1) * hop + n_fft // 2)
        valid = n >= 0 and o[b] <= n
        length = max(0, e[b] - o[b]) if valid else 0
        e[b] = o[b] + length
        samp0[2 * b], samp0[2 * b + 1] = b * span, b * span + length
        wf[b], ws[b] = (2 * b if valid else -1), s - o[b] // hop
    samp0[2 * B] = B * span
    return {'o': o, 'e': e, 'samp0': samp0, 'win_file': wf, 'win_start': ws}


def frames_fp64(x, hop=HOP, n_fft=NFFT, bands=8):
    """[1 + n / hop, bands] fp64: frame t = samples t hop - n_fft / 2 .. + n_fft of x, zeros outside, Hann window, |rDFT|^2 summed over `bands`
    equal bands, log(. + 1e-8)"""
    x = np.asarray(x, np.float64)
    nf = 1 + len(x) // hop
    ext = np.concatenate([np.zeros(n_fft // 2), x, np.zeros(n_fft // 2 + hop)])
    win = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n_fft) / n_fft)
    out = np.zeros((nf, bands))
    for t in range(nf):
        p = np.abs(np.fft.rfft(ext[t * hop:t * hop + n_fft] * win)) ** 2
        out[t] = np.log(p[:n_fft // 2].reshape(bands, -1).sum(1) + 1e-8)
    return out


def clip_frames(wave, samp0, win_file, win_start, width=WIDTH, hop=HOP, n_fft=NFFT, fill=FILL, bands=8):
    """hftt_clip_logmel's frame picking in fp64 -> [B, bands, width]: column c of window b is frame win_start[b] + c of file win_file[b] (samples
    samp0[f] .. samp0[f + 1] of `wave`) where 0 <= frame < 1 + n / hop, else fill; a file index outside the table is all fill"""
    B = len(win_file)
    out = np.full((B, bands, width), fill)
    for b in range(B):
        f = int(win_file[b])
        if f < 0 or f + 1 >= len(samp0):
            continue
        fr = frames_fp64(wave[int(samp0[f]):int(samp0[f + 1])], hop, n_fft, bands)
        for c in range(width):
            t = int(win_start[b]) + c
            if 0 <= t < len(fr):
                out[b, :, c] = fr[t]
    return out
