#!/usr/bin/env python3
"""Train the path on the synthetic plucked-string corpus and score config 5 with weights that mean something (GPU box).

  python tools/train_config5.py --config tiny --minutes 6 --out gpurun_out/config5_tiny.pkl

Corpus: `--files` one-minute files from corpus.synth_audio (seeds 2000.., never the scored file's seed 1234) -> HIP log-mel
(model.amt.AMT.wave2feature) -> frame labels (corpus.conv_note2label.note2label_arrays, the reference's label recipe) -> one MAESTRO-format
store (corpus.make_dataset.assemble_store) resident in HBM (training.dataset.DeviceClipStore); with --note-store the corpus keeps the NOTES
instead of the label tracks (assemble_note_store, NoteClipStore) and every batch's labels are rendered on the device; with --wave-store it keeps the
WAVEFORMS (int16) and the notes (assemble_wave_store, WaveClipStore): no feature pass, every batch's log-mel windows are computed on the device,
optionally under --aug-gain-db LO HI / --aug-noise-dbfs LO HI (per-clip gain and additive noise, new for every batch) and --aug-pitch LO HI /
--aug-detune-cents C / --aug-shift / --aug-warp-p P (per-clip pitch shift, detune and time offset: the clip is resampled and its labels move with it)
and --aug-mix-p P / --aug-mix-gain-db LO HI (clip mixing: a second clip summed in, the labels those of the sum) and --aug-room-p P with
--aug-room-rt60 LO HI / --aug-room-drr-db LO HI / --aug-room-taps L or --aug-room-bank FILE.npz (reverb: the clip convolved with an impulse
response of a synthetic or supplied bank, the labels unchanged).  Training: the product's own step
(hftt_hip.trainer.TrainStep: forward + fused loss + backward + fused Adam) in the chosen precision mode, dropout 0.1, batch 8, until the
time budget is spent.  The model is pickled the way m_training.py:372-373 does it (whole module, protocol 4).

With --synth-store [--synth-voices V] [--synth-partials H] [--synth-seed S] the corpus keeps the NOTES alone: every batch's audio is rendered on
the device under a plucked-string voice drawn per clip (assemble_synth_store, SynthClipStore, corpus.synth_audio.synth_voice_bank); the gain,
noise and room options apply, warp and mix do not.  What is PLAYED varies instead: --synth-transpose LO HI, --synth-tune-cents C,
--synth-tempo LO HI, --synth-shift, --synth-play-p P and --synth-duet-p P [--synth-duet-gain-db LO HI] (training.dataset.SynthPlay: every key,
tuning, tempo and pairing of the note corpus, the labels rendered to match).

Criteria: --onset-pos-weight A / --offset-pos-weight A / --mpe-pos-weight A (a positive-class weight on those BCE heads, A and B alike),
--focal-gamma G (the soft-label focal factor |y - p|^G on all six), --velocity-silence-weight W (class 0, "no note", weighs W in the
velocity cross-entropy, the others 1) and --label-smoothing E: hftt_hip.criteria.BalancedBCELoss / nn.CrossEntropyLoss(weight=,
label_smoothing=) inside the fused loss launch (hftt_loss_w).  All default to neutral, and with all neutral the tool builds the reference's
criteria (hftt_loss).

Scoring (config 5): the seed-1234 minute -> log-mel -> 30 clips through AMT.transcript -> mpe2note -> note-F1 (onset, 50 ms) and frame-F1
against the GENERATING notes, in x3, bf16 and parity mode, plus the frame-level agreement of the modes with each other.  One JSON line."""
import argparse, json, math, os, pickle, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'nylon-amt_amd'))
import numpy as np
import torch
import bench
from corpus import synth_audio as SA
from corpus.conv_note2label import note2label_arrays
from corpus.make_dataset import assemble_note_store, assemble_store, assemble_synth_store, assemble_wave_store
from training.dataset import MyDataset, DeviceClipStore, NoteClipStore, SynthClipStore, SynthPlay, WaveAugment, WaveClipStore
from model.amt import AMT
from hftt_hip import ops
from evaluation.metrics import note_metrics, frame_metrics

ROOM_BANK_SIZE = 32          # responses of the synthetic room bank (--aug-room-p without --aug-room-bank)


def build_corpus(config, files, dev, n_slice=8, note_store=False, wave_store=False, augment=None, synth=None, play=None):
    """`files` one-minute plucked-string files (seeds 2000..) -> HIP log-mel -> reference-recipe labels -> one MAESTRO-format store in HBM;
    note_store: features + note table in HBM instead, labels rendered per batch (a file is then as long as its label track, not cut to its
    feature array); wave_store: waveforms (int16) + note table in HBM, no feature pass, `augment` a WaveAugment or None;
    synth = (voices, partials, seed): the NOTES alone in HBM and a bank of that many plucked-string voices, every batch's audio rendered on the
    device (no waveform is made here at all), `play` a SynthPlay or None (its tune_cents is also the bank's Nyquist headroom)"""
    t0 = time.time()
    if synth is not None:
        note_lists = [SA.pluck_notes(2000 + i) for i in range(files)]
        voices = SA.synth_voice_bank(synth[0], config, seed=synth[2], partials=synth[1], headroom_cents=play.tune_cents if play is not None else 0.0)
        store = assemble_synth_store(note_lists, config, release_samples=int(voices['release'].max()))
        clips = SynthClipStore(store, config, dev, ops.VoiceBank(device=dev, **voices), n_slice, seed=synth[2], augment=augment, play=play)
        return clips, {'files': files, 'samples': int(store['file_nsamp'].sum()), 'clips': len(clips), 'notes': clips.table.n_notes, 'voices': synth[0],
                       'partials': synth[1], 'resident_bytes': clips.resident_bytes(), 'seconds_to_build': round(time.time() - t0, 1)}
    if wave_store:
        note_lists = [SA.pluck_notes(2000 + i) for i in range(files)]
        store = assemble_wave_store([SA.pluck_wave(notes, device=dev).cpu().numpy() for notes in note_lists], note_lists, config)
        clips = WaveClipStore(store, config, dev, n_slice, wave_dtype='int16', augment=augment)
        return clips, {'files': files, 'samples': int(store['file_nsamp'].sum()), 'clips': len(clips), 'notes': clips.table.n_notes,
                       'resident_bytes': clips.resident_bytes(), 'seconds_to_build': round(time.time() - t0, 1)}
    tmp = tempfile.mkdtemp()
    with open(os.path.join(tmp, 'init.pkl'), 'wb') as fh:
        pickle.dump(bench.build_model(bench.CONFIGS['tiny'], 1, 0.1, 'cpu'), fh, protocol=4)
    fe = AMT(config, os.path.join(tmp, 'init.pkl'), batch_size=1)              # (front end only)
    feats, labs, note_lists = [], [], []
    for i in range(files):
        notes = SA.pluck_notes(2000 + i)
        f = fe.wave2feature(SA.pluck_wave(notes, device=dev).unsqueeze(0), SA.SR).numpy()
        if note_store:
            feats.append(f); note_lists.append(notes)
            continue
        lab = note2label_arrays(config, notes)
        n = f.shape[0]
        lab = {k: (np.concatenate([v, np.zeros((n - len(v),) + v.shape[1:], v.dtype)]) if len(v) < n else v[:n]) for k, v in lab.items()}
        feats.append(f); labs.append(lab)
    if note_store:
        store = assemble_note_store(feats, note_lists, config)
        clips = NoteClipStore(store, config, dev, n_slice)
        return clips, {'files': files, 'frames': int(store['feature'].shape[0]), 'clips': len(clips), 'notes': clips.table.n_notes,
                       'resident_bytes': clips.resident_bytes(), 'seconds_to_build': round(time.time() - t0, 1)}
    store = assemble_store(feats, labs, config)
    ds = MyDataset.from_arrays(store['feature'], store['label_onset'], store['label_offset'], store['label_mpe'], store['label_velocity'],
                               store['idx'], config, n_slice)
    clips = DeviceClipStore(ds, dev)
    return clips, {'files': files, 'frames': int(store['feature'].shape[0]), 'clips': len(clips), 'seconds_to_build': round(time.time() - t0, 1)}


def scale_position_embeddings_(model, scale):
    """multiply the three position tables (encoder bins, decoder notes, decoder frames) by `scale` -- an INITIALISATION choice of this tool.
    Why: the reference applies xavier_uniform_ to its nn.Embedding tables too (m_training.py:31-33: |w| <= 0.11 at 256 x 256) and adds them to
    token embeddings multiplied by sqrt(hid_dim) (model_spec2midi.py:95,190) whose entries are in the hundreds on raw log-mel input, so at
    initialisation the position of a bin / frame is 1e-3 of what LayerNorm sees and the model sits on the predict-the-prior plateau until
    Adam has grown the tables (tens of thousands of steps).  Measured with the fp32 CPU oracle itself: same
    seed, 600 steps: held-out ranking AUC 0.61 with the reference's tables, 0.99 with the tables x 30."""
    if scale == 1.0:
        return
    with torch.no_grad():
        for name, p in model.named_parameters():
            if 'pos_embedding' in name:
                p.mul_(scale)


def add_loss_arguments(ap):
    ap.add_argument('--onset-pos-weight', type=float, default=1.0, metavar='A', help='positive-class weight of the onset BCE heads, BalancedBCELoss(pos_weight=A) (1 = nn.BCELoss)')
    ap.add_argument('--offset-pos-weight', type=float, default=1.0, metavar='A', help='positive-class weight of the offset BCE heads')
    ap.add_argument('--mpe-pos-weight', type=float, default=1.0, metavar='A', help='positive-class weight of the mpe BCE heads')
    ap.add_argument('--focal-gamma', type=float, default=0.0, metavar='G', help='soft-label focal factor |y - p|^G on the six BCE heads: 0 (off), or in [1, 4]')
    ap.add_argument('--velocity-silence-weight', type=float, default=1.0, metavar='W', help='weight of velocity class 0 ("no note") in the cross-entropy, the other classes 1')
    ap.add_argument('--label-smoothing', type=float, default=0.0, metavar='E', help='label smoothing of the velocity cross-entropy, in [0, 1)')


def build_criteria(args, V=128):
    """the eight criteria of training.train.train's order (onset, offset, mpe, velocity for A, then for B) from the criterion flags; all
    neutral: the reference's 6x nn.BCELoss() + 2x nn.CrossEntropyLoss() (training/train.py:141-153)"""
    import torch.nn as nn
    from hftt_hip.criteria import BalancedBCELoss

    def bce(a):
        return nn.BCELoss() if a == 1.0 and args.focal_gamma == 0.0 else BalancedBCELoss(pos_weight=a, gamma=args.focal_gamma)

    def ce():
        w = None
        if args.velocity_silence_weight != 1.0:
            w = torch.ones(V)
            w[0] = args.velocity_silence_weight
        return nn.CrossEntropyLoss(weight=w, label_smoothing=args.label_smoothing)
    side = lambda: [bce(args.onset_pos_weight), bce(args.offset_pos_weight), bce(args.mpe_pos_weight), ce()]      # noqa: E731
    return tuple(side() + side())


def lr_at(step, lr, warmup=0, total=0, final_frac=1.0):
    """learning rate of optimizer step `step` (1-based): linear warm-up from lr / warmup to lr over `warmup` steps, then constant, or -- with
    `total` and `final_frac` < 1 -- a half cosine from lr down to lr * final_frac at step `total` (held there afterwards).  This schedule is
    the TOOL's (the reference's loop has ReduceLROnPlateau only, m_training.py:147): a post-LN transformer of the paper's width does not
    leave the loss plateau at a constant rate in the time one GPU call allows."""
    if warmup and step <= warmup:
        return lr * step / warmup
    if total and final_frac < 1.0:
        x = min(1.0, (step - warmup) / max(1, total - warmup))
        return lr * (final_frac + (1.0 - final_frac) * 0.5 * (1.0 + math.cos(math.pi * x)))
    return lr


def train_loop(model, clips, dev, precision, lr, steps=0, minutes=0.0, batch=8, seed=77, warmup=0, final_frac=1.0, clip=0.0, log_every=250,
               on_step=None, tag='', guard=False, weight_decay=0.0, groups=None, ema=None, ema_warmup=False, criteria=None):
    """the product's own training step until `steps` (or the time budget); returns (TrainStep, steps done, epochs started, loss curve, seconds).
    clip > 0 / guard / weight_decay > 0 are FusedAdam's max_grad_norm / guard / weight_decay: the same TrainStep call, a guarded optimizer.
    groups: keyword arguments of hftt_hip.trainer.stage_groups (fine-tuning: frozen stages, per-stage rates, no decay on 1-D tensors); every
    group's rate follows the schedule from its own base rate.  ema: FusedAdam's ema_decay (the averaged weights ride in the Adam launch;
    ts.opt.averaged_model() holds them afterwards), ema_warmup its warm-up schedule.  criteria: the eight criteria (build_criteria); None or
    the reference's: hftt_loss, otherwise the fused loss with their options (hftt_loss_w) -- criteria it does not compute are an error here."""
    from hftt_hip.criteria import LossSpec
    from hftt_hip.trainer import FusedAdam, TrainStep, stage_groups
    model.hftt_precision = precision
    model.train()
    params = model if not groups else stage_groups(model, **groups)
    ts = TrainStep(model, optimizer=FusedAdam(params, lr=lr, max_grad_norm=clip if clip > 0.0 else None, guard=guard, weight_decay=weight_decay,
                                              model=model, ema_decay=ema, ema_warmup=ema_warmup))
    if criteria is not None:
        spec = LossSpec.from_criteria(criteria, ts.engine.N, ts.engine.V, dev)
        if spec is False:
            raise ops.HfttError('train_loop: these criteria are not ones the fused loss computes (hftt_hip.criteria.LossSpec.from_criteria)')
        ts.loss_spec = spec
    group = ts.opt.param_groups[0]
    base = [g['lr'] for g in ts.opt.param_groups]
    t0, step, epoch, curve = time.time(), 0, 0, []
    acc = torch.zeros(9, device=dev)
    done = False
    while not done:
        for b in clips.loader(batch, shuffle=True, seed=seed + epoch, drop_last=True):
            for g, lr_g in zip(ts.opt.param_groups, base):
                g['lr'] = lr_at(step + 1, lr_g, warmup, steps, final_frac)
            acc += ts(b[0], *b[1:])
            step += 1
            if on_step is not None:
                on_step(ts, step)
            if step % log_every == 0:
                l = (acc / log_every).tolist(); acc.zero_()
                curve.append((step, round(l[0], 4)))
                print('%sstep %6d  loss %.4f  lr %.2e  (%.0f s, %.0f clips/s)' % (tag, step, l[0], group['lr'], time.time() - t0, step * batch / (time.time() - t0)), flush=True)
                if l[0] != l[0] or (steps and step >= steps) or (not steps and time.time() - t0 > minutes * 60.0):
                    done = True
                    break
        epoch += 1
    torch.cuda.synchronize()
    return ts, step, epoch, curve, time.time() - t0


def save_state(ts, step, path):
    eng, opt = ts.engine, ts.opt
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    torch.save({'step': step, 'flat_params': eng.flat_params.cpu(), 'exp_avg': opt.exp_avg.cpu(), 'exp_avg_sq': opt.exp_avg_sq.cpu(),
                'adam_steps': opt.step_count, 'dropout_counter': int(eng.step_counter), 'lr': opt.param_groups[0]['lr']}, path)
    print('state of step %d -> %s' % (step, path), flush=True)


def load_state(ts, path):
    st = torch.load(path, weights_only=False)
    eng, opt = ts.engine, ts.opt
    eng.flat_params.copy_(st['flat_params']); opt.exp_avg.copy_(st['exp_avg']); opt.exp_avg_sq.copy_(st['exp_avg_sq'])
    opt.step_count = int(st['adam_steps']); eng.step_counter = int(st['dropout_counter'])
    opt.param_groups[0]['lr'] = st['lr']
    eng._prepared_frozen = False
    return st


def score(pkl, precision, dev, notes, wave, config):
    """config 5 on one precision mode -> (line fragment, mpe posteriorgram)"""
    amt = AMT(config, pkl, batch_size=32)
    amt.model.hftt_precision = precision
    for _ in range(2):                                     # (first pass builds plans and workspaces)
        t0 = time.time()
        feat = amt.wave2feature(wave.unsqueeze(0), SA.SR)
        torch.cuda.synchronize(); t1 = time.time()
        outs = amt.transcript(feat.numpy())
        torch.cuda.synchronize(); t2 = time.time()
        est = amt.mpe2note(a_onset=outs[4], a_offset=outs[5], a_mpe=outs[6], a_velocity=outs[7])
        t3 = time.time()
    n_clips = -(-feat.shape[0] // 128)
    roll = SA.reference_roll(notes, feat.shape[0])
    nm = note_metrics(notes, est)
    fm = frame_metrics(roll, outs[6], threshold=0.5)
    return ({'clips': n_clips, 'clips_per_s_model': round(n_clips / (t2 - t1), 1), 'seconds': {'logmel': round(t1 - t0, 4), 'model': round(t2 - t1, 4), 'mpe2note_cpu': round(t3 - t2, 4)},
             'clips_per_s_end_to_end': round(n_clips / (t3 - t0), 1), 'n_ref_notes': len(notes), 'n_est_notes': len(est),
             'note': {k: round(float(v), 4) for k, v in nm.items() if k != 'matching'},
             'frame': {k: round(float(v), 4) for k, v in fm.items()}}, outs[6])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='tiny', choices=['tiny', 'paper'])
    ap.add_argument('--precision', default='x3')
    ap.add_argument('--minutes', type=float, default=6.0)
    ap.add_argument('--steps', type=int, default=0, help='stop after this many steps instead of the time budget')
    ap.add_argument('--files', type=int, default=48)
    ap.add_argument('--lr', type=float, default=3e-4)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--seed', type=int, default=77)
    ap.add_argument('--warmup', type=int, default=0, help='linear warm-up steps (lr_at)')
    ap.add_argument('--final-frac', type=float, default=1.0, help='< 1 with --steps: cosine decay to lr * final_frac at the last step')
    ap.add_argument('--pos-scale', type=float, default=1.0, help='multiply the position-embedding tables by this at initialisation (scale_position_embeddings_)')
    ap.add_argument('--clip', type=float, default=0.0, help='global gradient-norm clip, FusedAdam(max_grad_norm=...) (0 = off, as the reference)')
    ap.add_argument('--guard', action='store_true', help='skip a step whose gradient norm is not finite, FusedAdam(guard=True) (--clip and --weight-decay imply it)')
    ap.add_argument('--weight-decay', type=float, default=0.0, help='decoupled (AdamW) weight decay on every parameter, FusedAdam(weight_decay=...) (0 = off, as the reference)')
    ap.add_argument('--save-state', default='', help='pattern with one %%d: write the full training state there at the steps of --save-state-at')
    ap.add_argument('--save-state-at', default='')
    ap.add_argument('--note-store', action='store_true', help='keep notes instead of label tracks in HBM and render every batch\'s labels on the device (NoteClipStore)')
    ap.add_argument('--wave-store', action='store_true', help='keep int16 waveforms and notes in HBM and compute every batch\'s log-mel windows and labels on the device (WaveClipStore)')
    ap.add_argument('--synth-store', action='store_true', help='keep the NOTES alone in HBM and render every batch\'s audio from them on the device under a voice per clip (SynthClipStore); gain, noise and room augmentation apply')
    ap.add_argument('--synth-voices', type=int, default=None, metavar='V', help='with --synth-store: voices of the plucked-string bank (default 64)')
    ap.add_argument('--synth-partials', type=int, default=None, metavar='H', help='with --synth-store: partials per voice (default 16, at most 32)')
    ap.add_argument('--synth-seed', type=int, default=None, metavar='S', help='with --synth-store: seed of the bank and of the voice draws (default: --seed)')
    ap.add_argument('--aug-gain-db', type=float, nargs=2, metavar=('LO', 'HI'), default=None, help='with --wave-store: per-clip gain, uniform in dB, new for every batch')
    ap.add_argument('--aug-noise-dbfs', type=float, nargs=2, metavar=('LO', 'HI'), default=None, help='with --wave-store: per-clip additive noise level, uniform in dB re full scale')
    ap.add_argument('--aug-pitch', type=int, nargs=2, metavar=('LO', 'HI'), default=None,
                    help='with --wave-store: per-clip pitch shift of k semitones, uniform in LO .. HI (tape speed: note times scale with it; the labels follow)')
    ap.add_argument('--aug-detune-cents', type=float, default=0.0, metavar='C', help='with --wave-store: per-clip detune, uniform in +-C cents (C <= 50)')
    ap.add_argument('--aug-shift', action='store_true', help='with --wave-store: per-clip time offset, uniform in [0, hop) samples')
    ap.add_argument('--aug-warp-p', type=float, default=1.0, metavar='P', help='probability that a clip is warped at all (pitch, detune, shift)')
    ap.add_argument('--synth-transpose', type=int, nargs=2, metavar=('LO', 'HI'), default=None, help='with --synth-store: transpose each clip by a whole number of semitones uniform in LO .. HI (-11 .. 11), labels moved to match')
    ap.add_argument('--synth-tune-cents', type=float, default=None, metavar='C', help='with --synth-store: tune each clip by an offset uniform in +-C cents (at most 50)')
    ap.add_argument('--synth-tempo', type=float, nargs=2, metavar=('LO', 'HI'), default=None, help='with --synth-store: play each clip at a tempo log-uniform in LO .. HI (inside 0.5 .. 2); decays do not scale')
    ap.add_argument('--synth-shift', action='store_true', help='with --synth-store: delay each clip by a draw from [0, hop) samples')
    ap.add_argument('--synth-play-p', type=float, default=None, metavar='P', help='with --synth-store: probability that a clip is played under its draws at all (default 1)')
    ap.add_argument('--synth-duet-p', type=float, default=None, metavar='P', help='with --synth-store: probability that a clip gets a second part, another clip under a voice and a play of its own (the labels are those of the sum)')
    ap.add_argument('--synth-duet-gain-db', type=float, nargs=2, metavar=('LO', 'HI'), default=None, help='with --synth-duet-p: the second part\'s gain, uniform in dB (default -6 0)')
    ap.add_argument('--aug-mix-p', type=float, default=0.0, metavar='P', help='with --wave-store: probability that a clip is summed with another clip of the corpus (the labels are those of the sum)')
    ap.add_argument('--aug-mix-gain-db', type=float, nargs=2, metavar=('LO', 'HI'), default=None, help='with --aug-mix-p: the partner clip\'s gain, uniform in dB (default -6 0)')
    ap.add_argument('--aug-room-p', type=float, default=0.0, metavar='P', help='with --wave-store: probability that a clip is convolved with an impulse response of the room bank (the labels are unchanged)')
    ap.add_argument('--aug-room-rt60', type=float, nargs=2, metavar=('LO', 'HI'), default=None, help='with --aug-room-p: reverberation time of the synthetic bank in seconds, uniform (default 0.15 0.8)')
    ap.add_argument('--aug-room-drr-db', type=float, nargs=2, metavar=('LO', 'HI'), default=None, help='with --aug-room-p: direct-to-reverberant ratio of the synthetic bank in dB, uniform (default 0 12)')
    ap.add_argument('--aug-room-taps', type=int, default=None, metavar='L', help='with --aug-room-p: taps of the synthetic bank (default 4096, at most 8192)')
    ap.add_argument('--aug-room-bank', default='', metavar='FILE.npz', help='with --aug-room-p: a bank of measured responses or equalisation filters instead (arrays ir [n, L] and taps [n])')
    ap.add_argument('--ema', type=float, default=None, metavar='D', help='keep the exponential moving average of the weights inside the Adam launch, FusedAdam(ema_decay=D); '
                    'both the raw and the averaged weights are scored, and --out saves the AVERAGED model (the raw one goes next to it as *_raw.pkl)')
    ap.add_argument('--ema-warmup', action='store_true', help='with --ema, from scratch: the decay of call t is min(D, (1 + t) / (10 + t)), FusedAdam(ema_warmup=True)')
    add_loss_arguments(ap)
    ap.add_argument('--out', default='gpurun_out/config5_tiny.pkl')
    ap.add_argument('--score-only', default='', help='skip training: score this pickled model')
    ap.add_argument('--init', default='', help='start from this pickled model (weights only: the optimizer state starts afresh) -- chains runs that are each bounded by the GPU call limit')
    ap.add_argument('--freeze', default='', choices=['', 'encoder', 'encoder+freq'],
                    help='fine-tuning (with --init): keep these stages\' bits; the backward stops where nothing trainable remains')
    ap.add_argument('--lr-encoder', type=float, default=None, help='learning rate of the encoder (default: --lr)')
    ap.add_argument('--lr-freq', type=float, default=None, help='learning rate of the frequency decoder and heads A (default: --lr)')
    ap.add_argument('--lr-time', type=float, default=None, help='learning rate of the time decoder and heads B (default: --lr)')
    ap.add_argument('--no-decay-1d', action='store_true', help='with --weight-decay: none on biases and LayerNorm parameters')
    args = ap.parse_args()
    if args.synth_store and (args.wave_store or args.note_store):
        ap.error('--synth-store, --wave-store and --note-store are exclusive: each names what the corpus keeps in HBM')
    if not args.synth_store and any(x is not None for x in (args.synth_voices, args.synth_partials, args.synth_seed)):
        ap.error('--synth-voices / --synth-partials / --synth-seed describe the voice bank: they need --synth-store')
    synth_play = (args.synth_shift or any(x is not None for x in (args.synth_transpose, args.synth_tune_cents, args.synth_tempo, args.synth_play_p,
                                                                  args.synth_duet_p, args.synth_duet_gain_db)))
    if synth_play and not args.synth_store:
        ap.error('--synth-transpose / --synth-tune-cents / --synth-tempo / --synth-shift / --synth-play-p / --synth-duet-p / --synth-duet-gain-db '
                 'say how the notes are played: they need --synth-store')
    play = None
    if synth_play:
        try:
            play = SynthPlay(transpose=args.synth_transpose, tune_cents=args.synth_tune_cents or 0.0, tempo=args.synth_tempo, shift=args.synth_shift,
                             p_play=1.0 if args.synth_play_p is None else args.synth_play_p, duet_p=args.synth_duet_p or 0.0,
                             duet_gain_db=args.synth_duet_gain_db or (-6.0, 0.0))
        except ops.HfttError as e:
            ap.error(str(e))
    waveform = args.wave_store or args.synth_store          # the stores with a waveform to augment
    warp_aug = args.aug_pitch is not None or args.aug_detune_cents != 0.0 or args.aug_shift or args.aug_warp_p != 1.0
    mix_aug = args.aug_mix_p != 0.0 or args.aug_mix_gain_db is not None
    if (warp_aug or mix_aug) and args.synth_store:
        ap.error('--synth-store takes gain, noise and room: an augment that warps or mixes is not built there (pitch and polyphony are the note list\'s)')
    if warp_aug and not args.wave_store:
        ap.error('--aug-pitch / --aug-detune-cents / --aug-shift / --aug-warp-p act on the waveform: they need --wave-store')
    if mix_aug and not args.wave_store:
        ap.error('--aug-mix-p / --aug-mix-gain-db act on the waveform: they need --wave-store')
    room_synth = args.aug_room_rt60 is not None or args.aug_room_drr_db is not None or args.aug_room_taps is not None
    room_aug = args.aug_room_p != 0.0 or room_synth or bool(args.aug_room_bank)
    if room_aug and not waveform:
        ap.error('--aug-room-p / --aug-room-rt60 / --aug-room-drr-db / --aug-room-taps / --aug-room-bank act on the waveform: they need --wave-store')
    if room_synth and args.aug_room_bank:
        ap.error('--aug-room-bank supplies the responses: --aug-room-rt60 / --aug-room-drr-db / --aug-room-taps describe the synthetic bank')
    try:
        criteria = build_criteria(args, V=bench.CONFIGS[args.config].n_velocity)
    except ValueError as e:
        ap.error(str(e))
    if not 0.0 <= args.label_smoothing < 1.0 or args.velocity_silence_weight < 0.0:
        ap.error('--label-smoothing is in [0, 1) and --velocity-silence-weight is not negative')
    if args.freeze and not args.init:
        ap.error('--freeze keeps pretrained weights fixed: it needs --init')
    groups = None
    if args.freeze or args.no_decay_1d or any(x is not None for x in (args.lr_encoder, args.lr_freq, args.lr_time)):
        frozen = {'': (), 'encoder': ('encoder',), 'encoder+freq': ('encoder', 'freq')}[args.freeze]
        groups = {st: dict(lr=args.lr if rate is None else rate, **({'frozen': True} if st in frozen else {}))
                  for st, rate in (('encoder', args.lr_encoder), ('freq', args.lr_freq), ('time', args.lr_time))}
        groups['no_decay_1d'] = args.no_decay_1d
    dev = torch.device('cuda:0')
    config = SA.default_config()
    cfg = bench.CONFIGS[args.config]
    log = {'config': args.config, 'precision': args.precision}
    pkl = args.score_only
    raw_pkl = ''
    if args.ema_warmup and args.ema is None:
        ap.error('--ema-warmup shapes the decay of --ema: give --ema D')
    if not pkl:
        # ---- corpus ----
        model = bench.build_model(cfg, args.seed, 0.1, 'cpu')
        scale_position_embeddings_(model, args.pos_scale)
        if args.init:
            with open(args.init, 'rb') as fh:
                model.load_state_dict(pickle.load(fh).state_dict())
            log['init'] = args.init
        if (args.aug_gain_db or args.aug_noise_dbfs) and not waveform:
            ap.error('--aug-gain-db / --aug-noise-dbfs act on the waveform: they need --wave-store')
        augment = None
        if args.aug_gain_db or args.aug_noise_dbfs or warp_aug or mix_aug or room_aug:
            bank = None
            if args.aug_room_p > 0.0:
                if args.aug_room_bank:
                    with np.load(args.aug_room_bank) as z:
                        bank = ops.RoomBank(z['ir'], dev, taps=z['taps'])
                else:
                    ir, taps = SA.synth_room_bank(ROOM_BANK_SIZE, config['feature']['sr'], taps=args.aug_room_taps or 4096, rt60=args.aug_room_rt60 or (0.15, 0.8),
                                                  drr_db=args.aug_room_drr_db or (0.0, 12.0), seed=args.seed)
                    bank = ops.RoomBank(ir, dev, taps=taps)
            augment = WaveAugment(gain_db=args.aug_gain_db, noise_dbfs=args.aug_noise_dbfs, seed=args.seed, pitch_semitones=args.aug_pitch,
                                  detune_cents=args.aug_detune_cents, shift=args.aug_shift, p_warp=args.aug_warp_p, mix_p=args.aug_mix_p,
                                  mix_gain_db=args.aug_mix_gain_db or (-6.0, 0.0), room_p=args.aug_room_p, room_bank=bank)
        clips, log['corpus'] = build_corpus(config, args.files, dev, note_store=args.note_store, wave_store=args.wave_store, augment=augment,
                                           synth=(args.synth_voices or 64, args.synth_partials or 16, args.seed if args.synth_seed is None else args.synth_seed) if args.synth_store else None,
                                           play=play)
        if play is not None:
            log['synth_play'] = {'transpose': play.transpose, 'tune_cents': play.tune_cents, 'tempo': play.tempo, 'shift': play.shift, 'p_play': play.p_play,
                                 'duet_p': play.duet_p, 'duet_gain_db': play.duet_gain_db}
        if waveform:
            log['augment'] = {'gain_db': args.aug_gain_db, 'noise_dbfs': args.aug_noise_dbfs, 'pitch_semitones': args.aug_pitch,
                              'detune_cents': args.aug_detune_cents, 'shift': args.aug_shift, 'p_warp': args.aug_warp_p,
                              'mix_p': args.aug_mix_p, 'mix_gain_db': args.aug_mix_gain_db, 'room_p': args.aug_room_p,
                              'room_bank': None if augment is None or augment.room_bank is None else
                              {'source': args.aug_room_bank or 'synth_room_bank', 'n_ir': augment.room_bank.n_ir, 'L': augment.room_bank.L}}
        # ---- training ----
        model = model.to(dev)
        saver = None
        if args.save_state:                       # full training state at chosen steps (parameters, both Adam moments, counters) for tools/ab_modes.py
            at = set(int(x) for x in args.save_state_at.split(',') if x)
            def saver(ts, step):
                if step in at:
                    save_state(ts, step, args.save_state % step)
        ts, step, epoch, curve, secs = train_loop(model, clips, dev, args.precision, args.lr, steps=args.steps, minutes=args.minutes, batch=args.batch,
                                                   seed=args.seed, warmup=args.warmup, final_frac=args.final_frac, clip=args.clip, on_step=saver,
                                                   guard=args.guard, weight_decay=args.weight_decay, groups=groups, ema=args.ema,
                                                   ema_warmup=args.ema_warmup, criteria=criteria)
        if curve and curve[-1][1] != curve[-1][1]:
            log['diverged_at_step'] = step
        log['training'] = {'steps': step, 'epochs_started': epoch, 'seconds': round(secs, 1), 'lr': args.lr, 'warmup': args.warmup, 'final_frac': args.final_frac,
                           'clip': args.clip, 'guard': args.guard, 'weight_decay': args.weight_decay,
                           'criteria': {'onset_pos_weight': args.onset_pos_weight, 'offset_pos_weight': args.offset_pos_weight, 'mpe_pos_weight': args.mpe_pos_weight,
                                        'focal_gamma': args.focal_gamma, 'velocity_silence_weight': args.velocity_silence_weight,
                                        'label_smoothing': args.label_smoothing, 'fused_launch': 'hftt_loss' if ts.loss_spec is None else 'hftt_loss_w'},
                           'groups': [{k: v for k, v in g.items() if k in ('stage', 'lr', 'weight_decay', 'frozen')} for g in ts.opt.param_groups] if groups else None,
                           'frozen_stages': ts.opt.frozen_stages(),
                           'skipped_steps': ts.opt.skipped_steps, 'clipped_steps': ts.opt.clipped_steps, 'pos_scale': args.pos_scale, 'batch': args.batch, 'dropout': 0.1, 'seed': args.seed,
                           'clips_per_s': round(step * args.batch / secs, 1), 'loss_curve': curve[:: max(1, len(curve) // 24)]}
        model.eval()
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        if args.ema is not None:                  # --out holds the averaged weights, the raw iterate goes next to it: both are scored below
            log['training']['ema'] = {'decay': args.ema, 'warmup': args.ema_warmup, 'updates': ts.opt.ema_updates}
            averaged = ts.opt.averaged_model()
            raw_pkl = os.path.splitext(args.out)[0] + '_raw.pkl'
            with open(raw_pkl, 'wb') as fh:
                pickle.dump(model.cpu(), fh, protocol=4)
            model = averaged
            log['checkpoint_raw'] = {'path': raw_pkl, 'bytes': os.path.getsize(raw_pkl)}
        with open(args.out, 'wb') as fh:
            pickle.dump(model.cpu(), fh, protocol=4)              # m_training.py:372-373
        pkl = args.out
        log['checkpoint'] = {'path': args.out, 'bytes': os.path.getsize(args.out)}
    # ---- config 5 ----
    notes = SA.pluck_notes(1234)
    wave = SA.pluck_wave(notes, device=dev)
    res, mpe = {}, {}
    for mode in ('x3', 'bf16', 'parity'):
        res[mode], mpe[mode] = score(pkl, mode, dev, notes, wave, config)
    agree = {}
    for mode in ('x3', 'bf16'):
        a, b = mpe[mode] >= 0.5, mpe['parity'] >= 0.5
        agree[mode] = {'frame_decisions_differing_from_parity_mode': int((a != b).sum()), 'of': int(a.size),
                       'frame_f1_against_parity_mode': round(float(frame_metrics(b, a)['f1']) if 'f1' in frame_metrics(b, a) else -1.0, 5),
                       'max_abs_posterior_difference': round(float(np.abs(mpe[mode] - mpe['parity']).max()), 6)}
    log['config5'] = {'workload': '60 s synthetic plucked-string audio (seed 1234) -> HIP log-mel -> %d clips -> AMT.transcript -> mpe2note, scored against the generating notes' % res['x3']['clips'],
                      'modes': res, 'agreement_with_parity_mode': agree}
    if raw_pkl:                                   # the averaged weights were scored above (--out); the raw iterate in the default mode beside them
        log['config5']['weights'] = 'averaged (ema_decay %g)' % args.ema
        log['config5_raw'] = {'weights': 'raw iterate of the last step', 'modes': {'x3': score(raw_pkl, 'x3', dev, notes, wave, config)[0]}}
    print(json.dumps(log))


if __name__ == '__main__':
    main()
