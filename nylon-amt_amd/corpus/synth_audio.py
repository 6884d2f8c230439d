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


def _pitch_hz(config):
    cm = config['midi']
    return 440.0 * np.power(2.0, (int(cm['note_min']) + np.arange(int(cm['num_note']), dtype=np.float64) - 69.0) / 12.0)


def _inc_q32(freq, sr):
    """phase increments in turns per sample as Q32 (uint32), 0 for a partial at or above Nyquist; and the mask of the partials below it"""
    below = freq < 0.5 * sr
    return np.where(below, np.round(freq / sr * 4294967296.0), 0.0).astype(np.uint64).astype(np.uint32), below


def synth_voice_bank(n, config, seed, partials=16, inharmonicity=(1e-5, 4e-4), detune_cents=6.0, pluck_pos=(0.08, 0.45), rolloff=(0.6, 1.6),
                     t60=(0.8, 4.0), pitch_damping=(0.3, 0.8), partial_damping=(0.02, 0.4), release_t60=(0.03, 0.25), attack_ms=(0.3, 4.0),
                     level=(0.03, 0.12), velocity_exponent=(0.7, 1.8), headroom_cents=0.0):
    """n voices of a plucked-string family for hftt_hip.ops.VoiceBank -> dict(inc uint32 [n, N, H], amp, dec fp32 [n, N, H], vel_gain fp32
    [n, 128], rel fp32 [n], attack, release int32 [n]); N = config.midi.num_note pitches from note_min, H = partials, sr = config.feature.sr.
    Everything is drawn and formed in fp64 and rounded once.  Per voice, each quantity uniform in its range (log-uniform where it spans decades):
        partial k = 1 .. H of the pitch with fundamental f0:  frequency k f0 sqrt(1 + B k^2) 2^(c_k / 1200) -- B the string's inharmonicity,
            c_k a detune uniform in +-detune_cents per partial (well under 50: the label's pitch stays the nearest one); at or above Nyquist the
            partial is off (amp = 0)
        amplitude  level |sin(k pi beta)| / k^rho, scaled so that the strongest partial of a pitch has `level` -- beta the pluck position
            (the comb of a string plucked at beta of its length), rho the roll-off
        decay      sigma_k = (sigma0 + sigma1 k^2) (f0 / 261.6 Hz)^gamma per second, sigma0 = 3 ln 10 / t60 (the fundamental of middle C is 60 dB
            down after t60 seconds), sigma1 = partial_damping sigma0; as log2 units per sample: sigma_k log2(e) / sr
        release    behind the offset the note falls by a further 60 dB in release_t60 seconds and is cut there; attack: a linear ramp of
            attack_ms; velocity curve (velocity / 127)^e with e in velocity_exponent
    headroom_cents: a partial within that margin below Nyquist is off too, so that a clip may be tuned up by as much (training.dataset.SynthPlay's
    tune_cents) without a partial folding over: the kernel does not check the tuned increment."""
    sr = float(config['feature']['sr'])
    H = int(partials)
    if n < 1 or H < 1:
        raise ValueError('synth_voice_bank: n=%r and partials=%r must be positive' % (n, partials))
    if not 0.0 <= float(detune_cents) < 50.0:
        raise ValueError('synth_voice_bank: detune_cents=%r outside 0 .. 50' % (detune_cents,))
    if not 0.0 <= float(headroom_cents) <= 1200.0:
        raise ValueError('synth_voice_bank: headroom_cents=%r outside 0 .. 1200' % (headroom_cents,))
    margin = float(np.power(2.0, float(headroom_cents) / 1200.0))
    rng = np.random.RandomState(seed)
    f0 = _pitch_hz(config)
    N = len(f0)
    k = np.arange(1, H + 1, dtype=np.float64)
    uni = lambda r: float(rng.uniform(r[0], r[1]))
    logu = lambda r: float(np.exp(rng.uniform(np.log(r[0]), np.log(r[1]))))
    out = {'inc': np.zeros((n, N, H), np.uint32), 'amp': np.zeros((n, N, H), np.float32), 'dec': np.zeros((n, N, H), np.float32),
           'vel_gain': np.zeros((n, 128), np.float32), 'rel': np.zeros(n, np.float32), 'attack': np.zeros(n, np.int32), 'release': np.zeros(n, np.int32)}
    for v in range(n):
        B, beta, rho = logu(inharmonicity), uni(pluck_pos), uni(rolloff)
        sigma0 = 3.0 * np.log(10.0) / logu(t60)
        gamma, sigma1 = uni(pitch_damping), logu(partial_damping) * sigma0
        rt60, att, lev, ve = logu(release_t60), logu(attack_ms), logu(level), uni(velocity_exponent)
        cents = rng.uniform(-detune_cents, detune_cents, H)
        freq = k[None, :] * f0[:, None] * np.sqrt(1.0 + B * k[None, :] ** 2) * np.power(2.0, cents[None, :] / 1200.0)
        inc, below = _inc_q32(freq, sr)
        below = below & (freq * margin < 0.5 * sr)
        inc = np.where(below, inc, 0).astype(np.uint32)
        a = np.abs(np.sin(k * np.pi * beta)) / np.power(k, rho)
        a = np.where(below, a[None, :], 0.0)
        a = lev * a / np.maximum(a.max(axis=1, keepdims=True), 1e-300)
        sigma = (sigma0 + sigma1 * k[None, :] ** 2) * np.power(f0[:, None] / 261.6255653, gamma)
        out['inc'][v], out['amp'][v], out['dec'][v] = inc, a, sigma * np.log2(np.e) / sr
        out['vel_gain'][v] = np.power(np.arange(128, dtype=np.float64) / 127.0, ve)
        out['rel'][v] = 3.0 * np.log(10.0) / rt60 * np.log2(np.e) / sr
        out['attack'][v], out['release'][v] = max(1, int(round(att * 1e-3 * sr))), int(np.ceil(rt60 * sr))
    return out


def pluck_voice(config):
    """ONE voice with pluck_wave's recipe, for continuity with the corpus every trained fixture rests on: partials 1, 1/2, 1/4 at f0, 2 f0, 3 f0
    (off at or above Nyquist), envelope exp(-3 t) from the onset, sounding until 0.3 s behind the offset without a further decay, amplitude
    velocity / 127 * 0.1, no attack ramp.  NOT sample-equal to pluck_wave: there the phase is sin(2 pi f t) of the ABSOLUTE time t in fp32, here it
    runs from the note's onset sample (and the onset is rounded to a sample); the two differ by a phase per note and by pluck_wave's fp32 time."""
    sr = float(config['feature']['sr'])
    f0 = _pitch_hz(config)
    freq = f0[:, None] * np.arange(1, 4, dtype=np.float64)[None, :]
    inc, below = _inc_q32(freq, sr)
    amp = np.where(below, 0.1 * np.array([1.0, 0.5, 0.25])[None, :], 0.0)
    return {'inc': inc[None], 'amp': amp[None].astype(np.float32), 'dec': np.full((1,) + freq.shape, 3.0 * np.log2(np.e) / sr, np.float32),
            'vel_gain': (np.arange(128, dtype=np.float64) / 127.0).astype(np.float32)[None], 'rel': np.zeros(1, np.float32),
            'attack': np.ones(1, np.int32), 'release': np.full(1, int(round(0.3 * sr)), np.int32)}


def render_file(table, bank, file, voice, nsamp, hop=256, n_fft=2048, play=None, tune=None, part=None, file_nsamp=None):
    """the whole synthetic file `file` of `table` (an ops.LabelsTable) under voice `voice` of `bank` (an ops.VoiceBank), nsamp samples long ->
    fp32 [nsamp] on the table's device: hftt_clip_synth with ONE window that covers the file, for listening and for the tests.
    play (an ops.Warp of one window), tune (one Q31 factor) and part (an ops.SynthPart of one window) play it as ops.clip_synth does
    (hftt_clip_synth_parts); nsamp is then the PLAYED file's length, and file_nsamp int64 [n_files] gives the partner file's."""
    from hftt_hip import ops
    nsamp = int(nsamp)
    width = max(1, -(-(nsamp - n_fft // 2) // hop) + 1)                         # (width - 1) hop + n_fft / 2 >= nsamp
    if play is None and tune is None and part is None:
        file_nsamp = torch.zeros(table.n_files, dtype=torch.int64)
        file_nsamp[file] = nsamp
        out, samp0, _, _ = ops.clip_synth(table, file_nsamp.to(table.device), bank, [voice], [file], [0], width, hop, table.sr, n_fft=n_fft)
        return out[0, :nsamp]
    if file_nsamp is None:
        if part is not None:
            raise ValueError('render_file: a part needs file_nsamp (the partner file\'s length)')
        file_nsamp = torch.zeros(table.n_files, dtype=torch.int64)
    out, samp0, _, _ = ops.clip_synth(table, torch.as_tensor(file_nsamp).to(table.device), bank, [voice], [file], [0], width, hop, table.sr, n_fft=n_fft,
                                      play=play, tune=None if tune is None else [int(tune)], part=part, nsamp=[nsamp])
    return out[0, :nsamp]
