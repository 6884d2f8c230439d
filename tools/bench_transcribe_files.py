#!/usr/bin/env python3
"""A file list in one pass against the per-file loop (GPU box): AMT.transcript_notes_files(files) and
[AMT.transcript_notes(f) for f in files], features on the device -> sorted note lists on the host, one process, warm-up first, then five
interleaved repeats (the same-box A/B rule).  Workloads: 64 synthetic 30-second files (15 clips each: the short-file
case the packing is for) and 4 synthetic 10-minute files.  Models: the tiny trained model of tests/golden and a paper-size random-init model
(its notes mean nothing; the times are real).  batch_size 32; output 'B' against one loop, 'AB' against the two loops it replaces.
Prints one JSON line.  Usage: python tools/bench_transcribe_files.py [x3|bf16] [repeats]"""
import json, os, pickle, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'nylon-amt_amd'))
import torch
import bench                                  # paper-size workload table + model builder (no oracle on this path)
from corpus import synth_audio as SA
from model.amt import AMT

precision = sys.argv[1] if len(sys.argv) > 1 else 'x3'
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
config = SA.default_config()
T = config['input']['num_frame']
tmp = tempfile.mkdtemp()
paper = bench.build_model(bench.CONFIGS['paper'], 1234, 0.1, 'cpu')
paper.hftt_precision = precision
with open(os.path.join(tmp, 'paper.pkl'), 'wb') as fh:
    pickle.dump(paper, fh, protocol=4)
MODELS = {'tiny_trained': os.path.join(ROOT, 'tests', 'golden', 'config5_tiny_trained.pkl'), 'paper_random_init_%s' % precision: os.path.join(tmp, 'paper.pkl')}
WORKLOADS = {'64 files of 30 s': (64, 30.0), '4 files of 600 s': (4, 600.0)}


def features(amt, n_files, dur):
    """synthetic plucked-string audio (corpus/synth_audio.py, one seed per file) -> log-mel on the device"""
    out = []
    for f in range(n_files):
        wave = SA.pluck_wave(SA.pluck_notes(1234 + f, dur), dur, SA.SR, device='cuda')
        out.append(amt.wave2feature(wave.unsqueeze(0), SA.SR, on_device=True))
    torch.cuda.synchronize()
    return out


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.time()
    res = fn()                                 # the note lists are on the host when the call returns: nothing left in flight
    return res, time.time() - t0


def median(v):
    return sorted(v)[len(v) // 2]


result = {'tool': 'tools/bench_transcribe_files.py', 'batch_size': 32, 'repeats': repeats, 'runs': []}
for mname, path in MODELS.items():
    amt = AMT(config, path, batch_size=32)
    for wname, (n_files, dur) in WORKLOADS.items():
        files = features(amt, n_files, dur)
        clips = sum(-(-f.shape[0] // T) for f in files)
        legs = {'packed_B': lambda: amt.transcript_notes_files(files),
                'loop_B': lambda: [amt.transcript_notes(f) for f in files],
                'packed_AB': lambda: amt.transcript_notes_files(files, output='AB'),
                'loops_A_and_B': lambda: list(zip([amt.transcript_notes(f, output='A') for f in files], [amt.transcript_notes(f) for f in files]))}
        got = {k: fn() for k, fn in legs.items()}                               # warm-up (plans, workspaces) and the comparison
        sec = {k: [] for k in legs}
        for _ in range(repeats):
            for k, fn in legs.items():                                          # interleaved
                sec[k].append(round(timed(fn)[1], 5))
        med = {k: median(v) for k, v in sec.items()}
        result['runs'].append({
            'model': mname, 'workload': wname, 'files': n_files, 'frames': int(sum(f.shape[0] for f in files)), 'clips': clips,
            'model_calls': {'packed': -(-clips // 32), 'loop': sum(-(-(-(-f.shape[0] // T)) // 32) for f in files)},
            'notes_B': sum(len(x) for x in got['packed_B']),
            'packed_equals_loop': {'B': got['packed_B'] == got['loop_B'], 'AB': got['packed_AB'] == got['loops_A_and_B']},
            'seconds': sec, 'median_seconds': med,
            'clips_per_s': {k: round(clips / v, 1) for k, v in med.items()},
            'loop_over_packed': {'B': round(med['loop_B'] / med['packed_B'], 3), 'AB': round(med['loops_A_and_B'] / med['packed_AB'], 3)}})
        print('done: %s, %s: %s' % (mname, wname, json.dumps(med)), file=sys.stderr, flush=True)
        del files
        torch.cuda.empty_cache()
print(json.dumps(result))
