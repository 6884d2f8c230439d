#!/usr/bin/env python3
"""Time a training batch from WaveClipStore (int16 waveforms + notes resident; log-mel windows by hftt_clip_logmel, labels by
hftt_labels_render) against the same clips from NoteClipStore (fp32 log-mel features + notes resident), and count the bytes both keep in HBM
(GPU box).

  python tools/bench_wave_store.py --files 2 --out profiles/wave_store.json [--step-ms 27.5]

Corpus: `--files` synthetic minutes of corpus.synth_audio (pluck_notes / pluck_wave) at the paper clip geometry (128 frames + 2 x 32 margin,
256 mel bins, 88 pitches); the note store's features are ops.LogMel of the same waveforms.  Three stores gather the SAME shuffled batches of
`--batch` clips: the note store, the wave store without augmentation, the wave store with gain and noise drawn per clip, and the wave store
under the warp (pitch shift -2 .. 2 semitones, 20 cents detune, time offset: hftt_clip_logmel_warp + hftt_labels_render_warp, every clip warped).  A
call is timed with one device event on each side, after a warm-up, the stores alternating; the median of `--calls` calls is reported.
--step-ms: the benchmark's median step time on the same box (bench.py --gpus 1), to state the extra time of a batch as a share of a step.

  python tools/bench_wave_store.py --mix-out profiles/clip_mix.json

The mixed leg (clip mixing: hftt_clip_logmel_mix[_warp] + hftt_labels_render_mix): WaveClipStore.batch with mix_p 0, 0.5 and 1, without and with
the warp above, on the same batches.  `--mix-repeats` repeats, the six stores interleaved inside each (the order rotates); a repeat's figure
is the median of `--mix-calls` calls, the reported figure the median of the repeats, next to every repeat's.  mix_p = 0 is the un-mixed
leg the others are read against.  Measured, no threshold.

  python tools/bench_wave_store.py --room-out profiles/clip_room.json [--room-taps 4096] [--step-ms 27.65]

The room leg (reverb: hftt_clip_room + the plain hftt_clip_logmel on its scratch): WaveClipStore.batch without augmentation and with room_p = 1
(every clip wet, a bank of 32 responses from corpus.synth_audio.synth_room_bank with its own lengths), interleaved as above, and the launches
alone under draws made beforehand: hftt_clip_room, the clip log-mel on the source corpus and on the scratch.

  python tools/bench_wave_store.py --synth-out profiles/clip_synth.json [--synth-voices 64] [--synth-partials 16] [--step-ms 27.65]

The synth leg (modal synthesis: hftt_clip_synth + the plain hftt_clip_logmel on its scratch): SynthClipStore.batch (the notes alone resident, a
bank of plucked-string voices from corpus.synth_audio.synth_voice_bank, a voice drawn per clip) against WaveClipStore.batch on the same
clip ids of the same corpus, interleaved as above, the launches alone under draws made beforehand (hftt_clip_synth with lead 0 and with the
lead a 4,096-tap room needs), the played clip synth as single launches prepared beforehand (hftt_clip_synth for comparison, then
hftt_clip_synth_parts under an identity performance, under a drawn play and with a second part), and the bytes both stores keep in HBM."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'nylon-amt_amd'))
import numpy as np
import torch
from corpus import synth_audio as SA
from corpus.make_dataset import assemble_note_store, assemble_synth_store, assemble_wave_store, finalize_config, prepare_config
from hftt_hip import ops
from training.dataset import NoteClipStore, SynthClipStore, SynthPlay, WaveAugment, WaveClipStore, warped_frame


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def mixed_leg(wstore, config, dev, chunks, repeats=5, calls=60, warmup=10, mix_ps=(0.0, 0.5, 1.0)):
    """{leg: {'ms': median over the repeats, 'repeats': [...]}} for mix_p x (plain, warped); the legs interleaved inside every repeat"""
    legs = {}
    for warp in (False, True):
        for p in mix_ps:
            kw = dict(seed=1)
            if warp:
                kw.update(pitch_semitones=(-2, 2), detune_cents=20.0, shift=True)
            if p > 0.0:
                kw.update(mix_p=p)
            aug = WaveAugment(**kw) if (warp or p > 0.0) else None
            legs['mix_p_%g%s' % (p, '_warped' if warp else '')] = WaveClipStore(wstore, config, dev, wave_dtype='int16', augment=aug)
    names = list(legs)
    assert len(chunks) >= warmup + calls, 'corpus too small for %d calls' % (warmup + calls)
    per = {n: [] for n in names}
    for r in range(repeats):
        t = {n: [] for n in names}
        for i, c in enumerate(chunks[:warmup + calls]):
            for n in names[r % len(names):] + names[:r % len(names)]:
                ms, _ = timed(lambda: legs[n].batch(c))
                if i >= warmup:
                    t[n].append(ms)
        for n in names:
            per[n].append(float(np.median(t[n])))
    out = {n: {'ms': float(np.median(v)), 'repeats': v} for n, v in per.items()}
    if len(mix_ps) > 1:
        out['calls'] = mixed_calls(legs['mix_p_%g' % mix_ps[-1]], legs['mix_p_%g_warped' % mix_ps[-1]], chunks, repeats, calls, warmup)
    for warp in ('', '_warped'):
        base = out['mix_p_0' + warp]['ms']
        for p in mix_ps[1:]:
            out['mix_p_%g%s' % (p, warp)]['extra_ms_over_unmixed'] = out['mix_p_%g%s' % (p, warp)]['ms'] - base
    return out


def mixed_calls(store, warped, chunks, repeats, calls, warmup):
    """the two launches alone (through their ops wrappers, which derive cut / t_scale / t_delay), with and without a partner for every window,
    under draws made beforehand: {call: median over the repeats of the median ms}"""
    c = chunks[0]
    B = len(c)
    file, frame = store.clip_file[c], store.clip_frame[c]
    on, partner, gain = store.augment.draw_mix(B, len(store))
    pfile, pframe = store.clip_file[partner], store.clip_frame[partner]
    w, pw = warped._draw_warp(file), warped._draw_warp(pfile)
    width, mb = store.mb + store.T + store.mf, store.mb
    af, afw = ops.audio_frames(store.waves, store.logmel.hop, file), ops.audio_frames(store.waves, store.logmel.hop, file, w)
    mix = lambda off, pwarp: ops.Mix(pfile, pframe - off, gain, pwarp)
    fns = {'clip_logmel': lambda: ops.clip_logmel(store.waves, store.logmel, file, frame - mb, width, store.fill),
           'clip_logmel_mix': lambda: ops.clip_logmel(store.waves, store.logmel, file, frame - mb, width, store.fill, mix=mix(mb, None)),
           'clip_logmel_warp': lambda: ops.clip_logmel(store.waves, store.logmel, file, frame - mb, width, store.fill, warp=w),
           'clip_logmel_mix_warp': lambda: ops.clip_logmel(store.waves, store.logmel, file, frame - mb, width, store.fill, warp=w, mix=mix(mb, pw)),
           'labels_render': lambda: ops.labels_render(store.table, file, frame, store.T),
           'labels_render_mix': lambda: ops.labels_render(store.table, file, frame, store.T, mix=mix(0, None), a_frames=af),
           'labels_render_warp': lambda: ops.labels_render(store.table, file, frame, store.T, warp=w),
           'labels_render_mix_warp': lambda: ops.labels_render(store.table, file, frame, store.T, warp=w, mix=mix(0, pw), a_frames=afw)}
    per = {n: [] for n in fns}
    for r in range(repeats):
        t = {n: [] for n in fns}
        for i in range(warmup + calls):
            for n, fn in fns.items():
                ms, _ = timed(fn)
                if i >= warmup:
                    t[n].append(ms)
        for n in fns:
            per[n].append(float(np.median(t[n])))
    return {n: float(np.median(v)) for n, v in per.items()}


def room_leg(wstore, config, dev, chunks, repeats=5, calls=60, warmup=10, taps=4096, n_ir=32):
    """{leg: {'ms': median over the repeats, 'repeats': [...]}} for the store without and with the room (every clip wet), interleaved inside every
    repeat (the order rotates), and 'calls': the launches alone"""
    ir, ir_taps = SA.synth_room_bank(n_ir, config['feature']['sr'], taps=taps, seed=1)
    bank = ops.RoomBank(ir, dev, taps=ir_taps)
    legs = {'room_off': WaveClipStore(wstore, config, dev, wave_dtype='int16'),
            'room_on': WaveClipStore(wstore, config, dev, wave_dtype='int16', augment=WaveAugment(seed=1, room_p=1.0, room_bank=bank))}
    names = list(legs)
    assert len(chunks) >= warmup + calls, 'corpus too small for %d calls' % (warmup + calls)
    store = legs['room_on']
    c = chunks[0]
    file, start = store.clip_file[c], store.clip_frame[c] - store.mb
    width = store.mb + store.T + store.mf
    index = store.augment.draw_room(len(c))
    wet, samp0, ofile, ostart = ops.clip_room(store.waves, file, start, width, bank, index, store.logmel.hop)
    scratch = ops.WetTable(wet, samp0)
    fns = {'clip_room': lambda: ops.clip_room(store.waves, file, start, width, bank, index, store.logmel.hop),
           'clip_logmel': lambda: ops.clip_logmel(store.waves, store.logmel, file, start, width, store.fill),
           'clip_logmel_on_scratch': lambda: ops.clip_logmel(scratch, store.logmel, ofile, ostart, width, store.fill)}
    per, per_fn = {n: [] for n in names}, {n: [] for n in fns}
    for r in range(repeats):
        t, tf = {n: [] for n in names}, {n: [] for n in fns}
        for i, c in enumerate(chunks[:warmup + calls]):
            for n in names[r % len(names):] + names[:r % len(names)]:
                ms, _ = timed(lambda: legs[n].batch(c))
                if i >= warmup:
                    t[n].append(ms)
            for n, fn in fns.items():
                ms, _ = timed(fn)
                if i >= warmup:
                    tf[n].append(ms)
        for n in names:
            per[n].append(float(np.median(t[n])))
        for n in fns:
            per_fn[n].append(float(np.median(tf[n])))
    out = {n: {'ms': float(np.median(v)), 'repeats': v} for n, v in per.items()}
    out['room_on']['extra_ms_over_room_off'] = out['room_on']['ms'] - out['room_off']['ms']
    out['calls'] = {n: {'ms': float(np.median(v)), 'repeats': v} for n, v in per_fn.items()}
    gmac = float((ir_taps[index.cpu().numpy()].astype(np.float64) * np.diff(samp0.cpu().numpy())[::2]).sum()) / 1e9
    out['bank'] = {'n_ir': n_ir, 'L': taps, 'ir_taps_min_median_max': [int(ir_taps.min()), int(np.median(ir_taps)), int(ir_taps.max())],
                   'clip_room_gmac_of_the_timed_call': gmac, 'scratch_bytes': wet.numel() * 4, 'bank_bytes': bank.nbytes()}
    return out


def parts_launches(store, bank, voice, file, start, width, hop):
    """the played clip synth on the clips of the timed call, each row ONE launch with everything in front of it prepared (ops._clip_synth_prepare):
    hftt_clip_synth itself for comparison; hftt_clip_synth_parts under an identity performance, under a play (transposition, tempo, delay and
    tune drawn per clip) and with a second part (another clip of the batch under a voice and a play of its own)"""
    B, dev = file.numel(), file.device
    play = SynthPlay(transpose=(-3, 3), tune_cents=30.0, tempo=(0.8, 1.25), shift=True, duet_p=1.0)
    gen = torch.Generator(device=dev).manual_seed(2)
    semis = lambda f: (-store.table.pitch_min[f.long()], store.table.N - 1 - store.table.pitch_max[f.long()])
    warp, tune = play.draw_play(gen, B, hop, *semis(file))
    _, _, pvoice, pgain = play.draw_duet(gen, B, len(store), bank.V)
    pfile, pstart = file.roll(1), start.roll(1)                                 # the partner: the neighbouring clip of the batch, as dense as the primary
    pwarp, ptune = play.draw_play(gen, B, hop, *semis(pfile))
    part = ops.SynthPart(pfile, warped_frame(pstart + store.mb, pwarp, hop) - store.mb, pvoice, pgain, pwarp, ptune)
    args = (store.table, store.file_nsamp, bank, voice, file)
    ident = ops.synth_nsamp(store.table, store.file_nsamp, file)
    mapped = ops.synth_nsamp(store.table, store.file_nsamp, file, warp)
    wstart = warped_frame(start + store.mb, warp, hop) - store.mb
    rows = {'clip_synth_launch': ops._clip_synth_prepare(*args, start, width, hop, store.sr, 0, 2048, None, None, None, None),
            'clip_synth_parts_identity': ops._clip_synth_prepare(*args, start, width, hop, store.sr, 0, 2048, None, None, None, ident),
            'clip_synth_parts_play': ops._clip_synth_prepare(*args, wstart, width, hop, store.sr, 0, 2048, warp, tune, None, mapped),
            'clip_synth_parts_duet': ops._clip_synth_prepare(*args, wstart, width, hop, store.sr, 0, 2048, warp, tune, part, mapped)}
    return {name: launch for name, (launch, _) in rows.items()}


def synth_leg(wstore, notes, config, dev, batch, repeats=5, calls=60, warmup=10, voices=64, partials=16):
    """{leg: {'ms': median over the repeats, 'repeats': [...]}} for the wave store and the synth store on the same clip ids, interleaved inside
    every repeat (the order rotates); 'calls': the launches alone; and what both stores keep resident"""
    bank_host = SA.synth_voice_bank(voices, config, seed=1, partials=partials)
    bank = ops.VoiceBank(device=dev, **bank_host)
    sstore = assemble_synth_store(notes, config, release_samples=int(bank_host['release'].max()))
    legs = {'wave_store': WaveClipStore(wstore, config, dev, wave_dtype='int16'), 'synth_store': SynthClipStore(sstore, config, dev, bank, seed=1)}
    # The two clip lists differ: a synthetic file ends `release` behind its last offset, the recorded minute runs on.  The timed batches are
    # drawn from the clips BOTH stores hold -- (file, frame) with frame below both files' counts -- as ids of either store, checked on the host.
    nf_w, nf_s = np.bincount(wstore['clip_file']), np.bincount(sstore['clip_file'])
    first_w, first_s = np.concatenate([[0], np.cumsum(nf_w)[:-1]]), np.concatenate([[0], np.cumsum(nf_s)[:-1]])
    file = np.repeat(np.arange(len(nf_w)), np.minimum(nf_w, nf_s))
    frame = np.concatenate([np.arange(n) for n in np.minimum(nf_w, nf_s)])
    id_w, id_s = first_w[file] + frame, first_s[file] + frame
    assert id_w.max() < len(wstore['clip_file']) and id_s.max() < len(sstore['clip_file'])
    assert np.array_equal(wstore['clip_file'][id_w], sstore['clip_file'][id_s]) and np.array_equal(wstore['clip_frame'][id_w], sstore['clip_frame'][id_s])
    order = torch.randperm(len(file), generator=torch.Generator().manual_seed(1)).numpy()
    chunks = [order[i:i + batch] for i in range(0, len(order) - batch + 1, batch)][:warmup + calls]
    ids = {'wave_store': lambda c: torch.from_numpy(id_w[c]).to(dev), 'synth_store': lambda c: torch.from_numpy(id_s[c]).to(dev)}
    names = list(legs)
    assert len(chunks) >= warmup + calls, 'corpus too small for %d calls' % (warmup + calls)
    store = legs['synth_store']
    c = ids['synth_store'](chunks[0])
    file, start = store.clip_file[c], store.clip_frame[c] - store.mb
    assert torch.equal(file, legs['wave_store'].clip_file[ids['wave_store'](chunks[0])])
    width, hop = store.mb + store.T + store.mf, store.logmel.hop
    voice = store.draw_voice(len(c))
    lead = -(-4096 // hop)
    out0, samp0, ofile, ostart = ops.clip_synth(store.table, store.file_nsamp, bank, voice, file, start, width, hop, store.sr)
    scratch = ops.WetTable(out0, samp0)
    fns = {'clip_synth': lambda: ops.clip_synth(store.table, store.file_nsamp, bank, voice, file, start, width, hop, store.sr),
           'clip_synth_lead_%d' % lead: lambda: ops.clip_synth(store.table, store.file_nsamp, bank, voice, file, start, width, hop, store.sr, lead=lead),
           **parts_launches(store, bank, voice, file, start, width, hop),
           'clip_logmel_on_scratch': lambda: ops.clip_logmel(scratch, store.logmel, ofile, ostart, width, store.fill),
           'labels_render': lambda: ops.labels_render(store.table, file, store.clip_frame[c], store.T)}
    per, per_fn = {n: [] for n in names}, {n: [] for n in fns}
    for r in range(repeats):
        t, tf = {n: [] for n in names}, {n: [] for n in fns}
        for i, ch in enumerate(chunks[:warmup + calls]):
            for n in names[r % len(names):] + names[:r % len(names)]:
                ms, _ = timed(lambda: legs[n].batch(ids[n](ch)))
                if i >= warmup:
                    t[n].append(ms)
            for n, fn in fns.items():
                ms, _ = timed(fn)
                if i >= warmup:
                    tf[n].append(ms)
        for n in names:
            per[n].append(float(np.median(t[n])))
        for n in fns:
            per_fn[n].append(float(np.median(tf[n])))
    out = {n: {'ms': float(np.median(v)), 'repeats': v} for n, v in per.items()}
    out['synth_store']['extra_ms_over_wave_store'] = out['synth_store']['ms'] - out['wave_store']['ms']
    out['calls'] = {n: {'ms': float(np.median(v)), 'repeats': v} for n, v in per_fn.items()}
    # the polyphony of the timed call: records that sound, averaged over the samples its rows hold
    tab, sr = sstore['table'], float(config['feature']['sr'])
    lens = np.diff(samp0.cpu().numpy())[::2]
    o = (np.maximum(0, start.cpu().numpy().astype(np.int64) - -(-1024 // hop)) * hop)
    sounding = 0.0
    for b in range(len(c)):
        f, v = int(file[b]), int(voice[b])
        rows = tab['notes'][tab['row_ptr'][f * tab['N']]:tab['row_ptr'][(f + 1) * tab['N']]]
        on = (rows['onset_sec'] * sr + 0.5).astype(np.int64)
        end = np.maximum((rows['offset_sec'] * sr + 0.5).astype(np.int64), on + 1) + int(bank_host['release'][v])
        sounding += float(np.clip(np.minimum(end, o[b] + lens[b]) - np.maximum(on, o[b]), 0, None).sum())
    out['timed_call'] = {'samples': int(lens.sum()), 'mean_sounding_records_per_sample': sounding / max(int(lens.sum()), 1), 'partials': partials,
                         'voices': voices, 'scratch_bytes': out0.numel() * 4}
    out['resident_bytes'] = {'wave_store': int(legs['wave_store'].resident_bytes()), 'synth_store': int(store.resident_bytes()), 'voice_bank': int(bank.nbytes()),
                             'note_table': int(store.table.nbytes())}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--files', type=int, default=2, help='synthetic one-minute files')
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--calls', type=int, default=300)
    ap.add_argument('--warmup', type=int, default=30)
    ap.add_argument('--step-ms', type=float, default=0.0)
    ap.add_argument('--out', default='profiles/wave_store.json')
    ap.add_argument('--mix-out', default='', help='run the mixed leg alone and write it here')
    ap.add_argument('--mix-repeats', type=int, default=5)
    ap.add_argument('--mix-calls', type=int, default=60)
    ap.add_argument('--room-out', default='', help='run the room leg alone and write it here')
    ap.add_argument('--room-taps', type=int, default=4096)
    ap.add_argument('--synth-out', default='', help='run the synth leg alone and write it here')
    ap.add_argument('--synth-voices', type=int, default=64)
    ap.add_argument('--synth-partials', type=int, default=16)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    config = finalize_config(prepare_config(SA.default_config()))
    notes = [SA.pluck_notes(2000 + i) for i in range(args.files)]
    waves = [SA.pluck_wave(a, device=dev) for a in notes]
    if args.synth_out:
        wstore = assemble_wave_store([w.cpu().numpy() for w in waves], notes, config)
        n = len(wstore['clip_file'])
        ids = torch.randperm(n, generator=torch.Generator().manual_seed(1))
        chunks = [ids[i:i + args.batch].to(dev) for i in range(0, n - args.batch + 1, args.batch)]
        cin = config['input']
        res = {'what': 'SynthClipStore.batch (notes alone resident, the audio rendered by hftt_clip_synth) against WaveClipStore.batch (int16 waveforms resident) on the same clip ids, and the launches alone: device events around each call; per repeat the median of the calls, reported the median of the repeats',
               'device': torch.cuda.get_device_name(0), 'files': args.files, 'clips': n, 'batch': args.batch, 'window_frames': cin['margin_b'] + cin['num_frame'] + cin['margin_f'],
               'mel_bins': config['feature']['mel_bins'], 'repeats': args.mix_repeats, 'calls': args.mix_calls, 'warmup': 10,
               'legs': synth_leg(wstore, notes, config, dev, args.batch, args.mix_repeats, args.mix_calls, 10, args.synth_voices, args.synth_partials)}
        if args.step_ms > 0.0:
            res['benchmark_step_ms_median'] = args.step_ms
            res['clip_synth_share_of_step'] = res['legs']['calls']['clip_synth']['ms'] / args.step_ms
            res['synth_extra_share_of_step'] = res['legs']['synth_store']['extra_ms_over_wave_store'] / args.step_ms
        os.makedirs(os.path.dirname(os.path.abspath(args.synth_out)), exist_ok=True)
        with open(args.synth_out, 'w') as fh:
            json.dump(res, fh, indent=1)
            fh.write('\n')
        print(json.dumps(res))
        return
    if args.room_out:
        wstore = assemble_wave_store([w.cpu().numpy() for w in waves], notes, config)
        n = len(wstore['clip_file'])
        ids = torch.randperm(n, generator=torch.Generator().manual_seed(1))
        chunks = [ids[i:i + args.batch].to(dev) for i in range(0, n - args.batch + 1, args.batch)]
        cin = config['input']
        res = {'what': 'WaveClipStore.batch without and with the room (room_p = 1, every clip wet) and the launches alone: device events around each call; per repeat the median of the calls, reported the median of the repeats',
               'device': torch.cuda.get_device_name(0), 'files': args.files, 'clips': n, 'batch': args.batch, 'window_frames': cin['margin_b'] + cin['num_frame'] + cin['margin_f'],
               'mel_bins': config['feature']['mel_bins'], 'repeats': args.mix_repeats, 'calls': args.mix_calls, 'warmup': 10,
               'legs': room_leg(wstore, config, dev, chunks, args.mix_repeats, args.mix_calls, 10, args.room_taps)}
        if args.step_ms > 0.0:
            res['benchmark_step_ms_median'] = args.step_ms
            res['room_extra_share_of_step'] = res['legs']['room_on']['extra_ms_over_room_off'] / args.step_ms
            res['clip_room_share_of_step'] = res['legs']['calls']['clip_room']['ms'] / args.step_ms
        os.makedirs(os.path.dirname(os.path.abspath(args.room_out)), exist_ok=True)
        with open(args.room_out, 'w') as fh:
            json.dump(res, fh, indent=1)
            fh.write('\n')
        print(json.dumps(res))
        return
    if args.mix_out:
        wstore = assemble_wave_store([w.cpu().numpy() for w in waves], notes, config)
        n = len(wstore['clip_file'])
        g = torch.Generator().manual_seed(1)
        ids = torch.randperm(n, generator=g)
        chunks = [ids[i:i + args.batch].to(dev) for i in range(0, n - args.batch + 1, args.batch)]
        cin = config['input']
        res = {'what': 'WaveClipStore.batch under clip mixing (mix_p 0 / 0.5 / 1, plain and warped): device events around each call; per repeat the median of the calls, reported the median of the repeats',
               'device': torch.cuda.get_device_name(0), 'files': args.files, 'clips': n, 'batch': args.batch, 'window_frames': cin['margin_b'] + cin['num_frame'] + cin['margin_f'],
               'mel_bins': config['feature']['mel_bins'], 'repeats': args.mix_repeats, 'calls': args.mix_calls, 'warmup': 10,
               'legs': mixed_leg(wstore, config, dev, chunks, args.mix_repeats, args.mix_calls, 10)}
        os.makedirs(os.path.dirname(os.path.abspath(args.mix_out)), exist_ok=True)
        with open(args.mix_out, 'w') as fh:
            json.dump(res, fh, indent=1)
            fh.write('\n')
        print(json.dumps(res))
        return
    lm = ops.LogMel(dev)
    feats = [lm(w).cpu().numpy() for w in waves]
    waves = [w.cpu().numpy() for w in waves]
    old = NoteClipStore(assemble_note_store(feats, notes, config), config, dev)
    wstore = assemble_wave_store(waves, notes, config)
    new = WaveClipStore(wstore, config, dev, wave_dtype='int16')
    aug = WaveClipStore(wstore, config, dev, wave_dtype='int16', augment=WaveAugment(gain_db=(-6.0, 6.0), noise_dbfs=(-60.0, -40.0), seed=1))
    warped = WaveClipStore(wstore, config, dev, wave_dtype='int16', augment=WaveAugment(pitch_semitones=(-2, 2), detune_cents=20.0, shift=True, seed=1))
    assert len(old) == len(new) == len(aug) == len(warped)
    chunks = old.loader(args.batch, shuffle=True, seed=1, drop_last=True).chunks
    chunks = [c.to(dev) for c in chunks[:args.warmup + args.calls]]
    assert len(chunks) == args.warmup + args.calls, 'corpus too small for %d calls' % (args.warmup + args.calls)
    t_old, t_new, t_aug, t_kernel, t_warp, t_kernel_warp = [], [], [], [], [], []
    cin = config['input']
    width = cin['margin_b'] + cin['num_frame'] + cin['margin_f']
    for i, c in enumerate(chunks):
        ms_old, a = timed(lambda: old.batch(c))
        ms_new, b = timed(lambda: new.batch(c))
        ms_aug, _ = timed(lambda: aug.batch(c))
        file, start = new.clip_file[c], new.clip_frame[c] - cin['margin_b']
        ms_k, _ = timed(lambda: ops.clip_logmel(new.waves, new.logmel, file, start, width, new.fill))
        ms_warp, _ = timed(lambda: warped.batch(c))
        w = warped.augment.draw_warp(len(c), new.logmel.hop)         # (the kernel alone under a fresh draw; the source-frame window, which is as long)
        ms_kw, _ = timed(lambda: ops.clip_logmel(new.waves, new.logmel, file, start, width, new.fill, warp=w))
        if i == 0:
            assert all(torch.equal(x, y) for x, y in zip(a[1:], b[1:])), 'the labels of the two stores disagree'
            worst = float((a[0] - b[0]).abs().max())            # int16 audio against fp32 audio: reported, the tests hold the kernel to fp64
        if i >= args.warmup:
            t_old.append(ms_old); t_new.append(ms_new); t_aug.append(ms_aug); t_kernel.append(ms_k); t_warp.append(ms_warp); t_kernel_warp.append(ms_kw)
    med = lambda v: float(np.median(v))
    p = lambda v: [float(np.percentile(v, 10)), float(np.percentile(v, 90))]
    frames = sum(f.shape[0] for f in feats)
    res = {'what': 'WaveClipStore.batch (int16 waveforms; plain and with gain + noise) against NoteClipStore.batch on the same clip ids (device events around each call, median)',
           'device': torch.cuda.get_device_name(0), 'files': args.files, 'audio_frames': frames, 'samples': int(wstore['file_nsamp'].sum()), 'clips': len(old),
           'notes': int(new.table.n_notes), 'batch': args.batch, 'window_frames': width, 'mel_bins': config['feature']['mel_bins'], 'calls': args.calls, 'warmup': args.warmup,
           'note_store_batch_ms': med(t_old), 'wave_store_batch_ms': med(t_new), 'wave_store_augmented_batch_ms': med(t_aug), 'clip_logmel_call_ms': med(t_kernel),
           'wave_store_warped_batch_ms': med(t_warp), 'clip_logmel_warp_call_ms': med(t_kernel_warp), 'extra_ms_per_batch_warped': med(t_warp) - med(t_new),
           'extra_ms_per_batch': med(t_new) - med(t_old), 'extra_ms_per_batch_augmented': med(t_aug) - med(t_old),
           'spread_ms': {'note_store_p10_p90': p(t_old), 'wave_store_p10_p90': p(t_new), 'wave_store_augmented_p10_p90': p(t_aug), 'wave_store_warped_p10_p90': p(t_warp)},
           'first_batch_max_abs_spec_difference_int16_audio': worst,
           'note_store_resident_bytes': int(old.resident_bytes()), 'wave_store_resident_bytes': int(new.resident_bytes()),
           'note_store_bytes_per_frame': old.resident_bytes() / frames, 'wave_store_bytes_per_frame': new.resident_bytes() / frames}
    if args.step_ms > 0.0:
        res['benchmark_step_ms_median'] = args.step_ms
        res['extra_share_of_step'] = res['extra_ms_per_batch'] / args.step_ms
        res['extra_share_of_step_augmented'] = res['extra_ms_per_batch_augmented'] / args.step_ms
        res['extra_share_of_step_warped'] = res['extra_ms_per_batch_warped'] / args.step_ms
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
