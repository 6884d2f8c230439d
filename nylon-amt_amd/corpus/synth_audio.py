"""Synthetic plucked-string audio with its generating note list: decaying harmonic plucks at MIDI 40-88,
16 kHz mono.  One place for the recipe so that the training set (tools/train_config5.py), the timed inference run
(tools/config5_inference.py) and the tests draw from the same generator -- with different seeds: the scored file is seed 1234, training
files take seeds the scored file never uses.  The reference has no such generator (it trains on MAESTRO, hftt_code/corpus/*): this is the
stand-in corpus of a box without network; what it feeds follows the reference's formats (note dicts as conv_midi2note.py writes them:
pitch / onset / offset / velocity; labels through corpus.conv_note2label)."""
import numpy as np
import torch

SR = 16000


def pluck_notes(seed, dur=60.0):
    """the seed-1234 recipe of round 1 (kept draw for draw: same notes for the same seed)"""
    rng = np.random.RandomState(seed)
    notes, t = [], 0.25
    while t < dur - 2.0:
        notes.append({'pitch': int(rng.randint(40, 89)), 'onset': t, 'offset': t + float(rng.uniform(0.3, 1.2)), 'velocity': int(rng.randint(40, 110))})
        t += float(rng.uniform(0.08, 0.35))
    return notes


def pluck_wave(notes, dur=60.0, sr=SR, device='cpu'):
    """sum over notes of three decaying harmonics (1, 1/2, 1/4), amplitude velocity / 127 * 0.1, envelope exp(-3 (t - onset)) gated to
    [onset, offset + 0.3 s) -- evaluated on each note's own sample range only (identical samples to the whole-array form of round 1)"""
    n = int(sr * dur)
    wave = torch.zeros(n, dtype=torch.float32, device=device)
    for nt in notes:
        i0 = max(0, int(np.floor(nt['onset'] * sr)) - 1)
        i1 = min(n, int(np.ceil((nt['offset'] + 0.3) * sr)) + 1)
        tt = torch.arange(i0, i1, dtype=torch.float32, device=device) / sr
        f0 = 440.0 * 2.0 ** ((nt['pitch'] - 69) / 12.0)
        env = torch.exp(-3.0 * (tt - nt['onset']).clamp(min=0)) * ((tt >= nt['onset']) & (tt < nt['offset'] + 0.3))
        seg = torch.zeros_like(tt)
        for h, a in ((1, 1.0), (2, 0.5), (3, 0.25)):
            if f0 * h < sr / 2:
                seg += (nt['velocity'] / 127.0) * 0.1 * a * torch.sin(2 * np.pi * f0 * h * tt) * env
        wave[i0:i1] += seg
    return wave


def default_config():
    """hftt_code/corpus/config.json with the two keys make_dataset.py adds (min_value, n_bins)"""
    return {'feature': {'sr': 16000, 'hop_sample': 256, 'mel_bins': 256, 'n_bins': 256, 'fft_bins': 2048, 'window_length': 2048,
                        'log_offset': 1e-8, 'window': 'hann', 'pad_mode': 'constant'},
            'input': {'margin_b': 32, 'margin_f': 32, 'num_frame': 128, 'min_value': -18.420681},
            'midi': {'note_min': 21, 'note_max': 108, 'num_note': 88, 'num_velocity': 128}}


def reference_roll(notes, n_frames, sr=SR, hop=256, note_min=21):
    roll = np.zeros((n_frames, 88), bool)
    for nt in notes:
        roll[int(nt['onset'] * sr / hop):int(nt['offset'] * sr / hop), nt['pitch'] - note_min] = True
    return roll


def synth_room_bank(n, sr=SR, taps=4096, rt60=(0.15, 0.8), drr_db=(0.0, 12.0), seed=0):
    """n synthetic room impulse responses for hftt_hip.ops.RoomBank -> (ir fp32 [n, taps], ir_taps int32 [n]).  Per response, in fp64, rounded
    once: tap 0 is 1 (the direct path: no onset moves), a pre-delay uniform in 1 .. 10 ms of silence, and from there a tail of Gaussian noise
    times the envelope 10^(-3 k / (rt60 sr)) (k samples behind the pre-delay: 60 dB down after rt60 seconds, rt60 uniform in its range),
    scaled so that the direct-to-reverberant ratio 10 log10(1 / sum tail^2) is drr_db (uniform in its range).  ir_taps is where the envelope
    has fallen by 60 dB, or `taps` if that lies behind the response; the entries behind it are zero.  The whole response is then normalised
    to unit L2 norm, so that a wet clip keeps the level of a dry one on noise-like signals."""
    if n < 1 or taps < 1:
        raise ValueError('synth_room_bank: n=%r and taps=%r must be positive' % (n, taps))
    rng = np.random.RandomState(seed)
    ir, ir_taps = np.zeros((n, taps), np.float64), np.zeros(n, np.int32)
    for r in range(n):
        t60 = float(rng.uniform(rt60[0], rt60[1]))
        drr = float(rng.uniform(drr_db[0], drr_db[1]))
        d = int(round(float(rng.uniform(0.001, 0.010)) * sr))
        noise = rng.standard_normal(taps)                                       # (drawn whole, whatever the pre-delay: one draw count per response)
        end = min(taps, d + int(np.ceil(t60 * sr)))                             # the envelope is 60 dB down here
        h = np.zeros(taps, np.float64)
        if end > max(d, 1):
            k = np.arange(end - max(d, 1), dtype=np.float64) + (max(d, 1) - d)
            tail = noise[max(d, 1):end] * np.power(10.0, -3.0 * k / (t60 * sr))
            energy = float(np.sum(tail * tail))
            if energy > 0.0:
                h[max(d, 1):end] = tail * np.sqrt(np.power(10.0, -drr / 10.0) / energy)
        h[0] = 1.0
        ir[r] = h / np.sqrt(np.sum(h * h))
        ir_taps[r] = max(1, end)
    return ir.astype(np.float32), ir_taps


def align_ir(h):
    """a measured impulse response (or an equalisation filter) as the room takes it: the sample of largest |h| moves to tap 0 (what lies in
    front of it is dropped, zeros fill the end), and the result has unit L2 norm -> fp32, the length of h"""
    h = np.asarray(h, np.float64)
    if h.ndim != 1 or h.size < 1 or not np.isfinite(h).all() or not np.any(h):
        raise ValueError('align_ir: a response is a 1-d array of finite samples, not all zero')
    p = int(np.argmax(np.abs(h)))
    out = np.zeros_like(h)
    out[:h.size - p] = h[p:]
    return (out / np.sqrt(np.sum(out * out))).astype(np.float32)
