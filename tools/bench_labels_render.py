#!/usr/bin/env python3
"""Time a training batch from NoteClipStore (features + notes resident, labels rendered by hftt_labels_render) against the same clips from
DeviceClipStore (four dense label tracks resident), and count the bytes both keep in HBM (GPU box).

  python tools/bench_labels_render.py --files 4 --out profiles/labels_render.json [--step-ms 41.3]

Corpus: `--files` synthetic minutes at the paper clip geometry (128 frames + 2 x 32 margin, 256 mel bins, 88 pitches): random features (their
values do not matter to a gather) and the note lists of corpus.synth_audio.pluck_notes (about 4.6 notes per second).  Each store gathers the
SAME shuffled batches of `--batch` clips; a call is timed with one device event on each side, after a warm-up, and the median of `--calls`
calls is reported, the two stores alternating.  --step-ms: the benchmark's median step time on the same box (bench.py --gpus 1), to state the
extra time of a rendered batch as a share of a step."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'nylon-amt_amd'))
import numpy as np
import torch
from corpus import synth_audio as SA
from corpus.conv_note2label import note2label_arrays
from corpus.make_dataset import assemble_note_store, assemble_store
from hftt_hip import ops
from training.dataset import DeviceClipStore, MyDataset, NoteClipStore


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--files', type=int, default=4, help='synthetic one-minute files')
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--calls', type=int, default=300)
    ap.add_argument('--warmup', type=int, default=30)
    ap.add_argument('--step-ms', type=float, default=0.0)
    ap.add_argument('--out', default='profiles/labels_render.json')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    config = SA.default_config()
    config['input']['max_value'] = 0.0
    rng = np.random.RandomState(0)
    notes = [SA.pluck_notes(2000 + i) for i in range(args.files)]
    feats = [rng.randn(3751, config['feature']['mel_bins']).astype(np.float32) for _ in range(args.files)]
    dense = assemble_store(feats, [note2label_arrays(config, a) for a in notes], config)
    sparse = assemble_note_store(feats, notes, config)
    assert np.array_equal(dense['idx'], sparse['idx'])
    ds = MyDataset.from_arrays(dense['feature'], dense['label_onset'], dense['label_offset'], dense['label_mpe'], dense['label_velocity'], dense['idx'], config, 1)
    old, new = DeviceClipStore(ds, dev), NoteClipStore(sparse, config, dev)
    chunks = old.loader(args.batch, shuffle=True, seed=1, drop_last=True).chunks
    chunks = [c.to(dev) for c in chunks[:args.warmup + args.calls]]
    assert len(chunks) == args.warmup + args.calls, 'corpus too small for %d calls' % (args.warmup + args.calls)
    t_old, t_new, t_render = [], [], []
    T = config['input']['num_frame']
    for i, c in enumerate(chunks):
        ms_old, a = timed(lambda: old.batch(c))
        ms_new, b = timed(lambda: new.batch(c))
        s = new.idx[c]
        file = (torch.bucketize(s, new.file_row0, right=True) - 1).int()
        start = (s - new.file_row0[file.long()]).int()
        ms_r, _ = timed(lambda: ops.labels_render(new.table, file, start, T))
        if i == 0:
            assert all(torch.equal(x, y) for x, y in zip(a, b)), 'the two stores disagree'
        if i >= args.warmup:
            t_old.append(ms_old); t_new.append(ms_new); t_render.append(ms_r)
    med = lambda v: float(np.median(v))
    frames = int(dense['feature'].shape[0])
    old_bytes = sum(t.numel() * t.element_size() for t in (old.feature, old.label_onset, old.label_offset, old.label_mpe, old.label_velocity, old.idx))
    res = {'what': 'NoteClipStore.batch against DeviceClipStore.batch on the same clip ids (device events around each call, median)',
           'device': torch.cuda.get_device_name(0), 'files': args.files, 'store_frames': frames, 'clips': len(old), 'notes': int(new.table.n_notes),
           'batch': args.batch, 'frames_per_clip': T, 'pitches': config['midi']['num_note'], 'calls': args.calls, 'warmup': args.warmup,
           'clip_store_batch_ms': med(t_old), 'note_store_batch_ms': med(t_new), 'labels_render_call_ms': med(t_render),
           'extra_ms_per_batch': med(t_new) - med(t_old),
           'spread_ms': {'clip_store_p10_p90': [float(np.percentile(t_old, 10)), float(np.percentile(t_old, 90))],
                         'note_store_p10_p90': [float(np.percentile(t_new, 10)), float(np.percentile(t_new, 90))]},
           'clip_store_resident_bytes': int(old_bytes), 'note_store_resident_bytes': int(new.resident_bytes()),
           'clip_store_bytes_per_frame': old_bytes / frames, 'note_store_bytes_per_frame': new.resident_bytes() / frames}
    if args.step_ms > 0.0:
        res['benchmark_step_ms_median'] = args.step_ms
        res['extra_share_of_step'] = res['extra_ms_per_batch'] / args.step_ms
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
