#!/usr/bin/env python3
"""The wave side of the streaming transcription on a GPU box: seconds per NoteStream.push_wave of 2.048 s of audio per stream (128 frames: one
clip's worth), for S = 1, 2, 4, ... streams, on the tiny trained model and on the paper-size model, with the samples at the feature rate
(16000) and at 44100 (open_stream(sr=44100): resampled on the device with the state carried forward), beside `push` of the same frames --
the floor that the front end adds to -- and beside the offline front end (ops.resample + ops.LogMel) over the same seconds of audio.

One process; every shape (model, rate, S, call) keeps its own open stream object and is warmed up with two pushes; then `repeats`
interleaved rounds, each round one timed push of every shape in turn, each timed window closed by a device synchronise; medians with p10 /
p90.  The chunks are host tensors, as live audio is.  A model's S stops doubling once a push takes longer than the audio it covers.

--root DIR imports the package from another checkout (a tree without open_stream(sr=) runs the 16000 lines only): the same tool on two
commits, alternated process by process by the caller, is the A/B of the 16 kHz path.  --merge A.json B.json ... prints the per-shape
medians of several result files side by side.

Writes profiles/stream_wave_mi355x.json (or --out) and prints it.
Usage: python tools/bench_stream_wave.py [--root DIR] [--out FILE] [--repeats 9] [--max-s 256] [--models tiny,paper] [--rates 16000,44100] [--precision x3]"""
import argparse, inspect, json, os, pickle, sys, tempfile, time

ap = argparse.ArgumentParser()
ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument('--out', default=None)
ap.add_argument('--repeats', type=int, default=9)
ap.add_argument('--max-s', type=int, default=256)
ap.add_argument('--models', default='tiny,paper')
ap.add_argument('--rates', default='16000,44100')
ap.add_argument('--precision', default='x3')
ap.add_argument('--merge', nargs='+', default=None)
args = ap.parse_args()


def pct(v):
    v = sorted(v)
    q = lambda p: v[min(len(v) - 1, int(p * len(v)))]
    return {'median': q(0.5), 'p10': q(0.1), 'p90': q(0.9)}


if args.merge:
    rows = {}
    for f in args.merge:
        r = json.load(open(f))
        for line in r['lines']:
            rows.setdefault((line['model'], line['rate'], line['call'], line['S']), []).append((r['label'], line['seconds']))
    for key in sorted(rows):
        print('%-6s %6d %-9s S=%-4d ' % key + '  '.join('%s %.5f [%.5f, %.5f]' % (lab, s['median'], s['p10'], s['p90']) for lab, s in rows[key]))
    sys.exit(0)

ROOT = os.path.abspath(args.root)
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'nylon-amt_amd'))
import torch
import bench                                  # paper-size workload table + model builder
from corpus import synth_audio as SA
from hftt_hip import ops
from model.amt import AMT

HAS_SR = 'sr' in inspect.signature(AMT.open_stream).parameters
rates = [int(r) for r in args.rates.split(',') if int(r) == SA.SR or HAS_SR]
WARM, SEC = 2, 2.048
n_push = WARM + args.repeats
config = SA.default_config()
T, hop = config['input']['num_frame'], config['feature']['hop_sample']
assert abs(T * hop / SA.SR - SEC) < 1e-9
wave16 = SA.pluck_wave(SA.pluck_notes(77, SEC * (n_push + 1)), SEC * (n_push + 1), SA.SR, device='cuda')
waves = {r: (wave16 if r == SA.SR else ops.resample(wave16, SA.SR, r)).cpu() for r in rates}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def shapes_of(mname, path):
    """every (rate, call, S) of one model as [key, stream object, per-push function]; S grows while a warm-up push stays below real time"""
    amt = AMT(config, path, batch_size=32)
    feat = amt.wave2feature(wave16.unsqueeze(0), SA.SR, on_device=True)
    out = []
    for rate, call in [(r, 'push_wave') for r in rates] + [(SA.SR, 'push')]:
        S = 1
        while S <= args.max_s:
            st = amt.open_stream(n_streams=S, sr=rate) if HAS_SR else amt.open_stream(n_streams=S)
            n = int(round(SEC * rate))
            if call == 'push':
                fn = lambda k, st=st, S=S: st.push([feat[k * T:(k + 1) * T]] * S)
            else:
                fn = lambda k, st=st, S=S, w=waves[rate], n=n: st.push_wave([w[k * n:(k + 1) * n]] * S)
            warm = [timed(lambda: fn(k)) for k in range(WARM)]
            out.append([(mname, rate, call, S), fn, []])
            print('warm: %s %d %s S=%d %.4f s' % (mname, rate, call, S, warm[-1]), file=sys.stderr, flush=True)
            if warm[-1] >= SEC:
                break
            S *= 2
    return out


tmp = tempfile.mkdtemp()
paths = {'tiny': os.path.join(ROOT, 'tests', 'golden', 'config5_tiny_trained.pkl')}
if 'paper' in args.models.split(','):
    paper = bench.build_model(bench.CONFIGS['paper'], 1234, 0.1, 'cpu')
    paper.hftt_precision = args.precision
    paths['paper'] = os.path.join(tmp, 'paper.pkl')
    with open(paths['paper'], 'wb') as fh:
        pickle.dump(paper, fh, protocol=4)
shapes = []
for m in args.models.split(','):
    shapes += shapes_of(m, paths[m])
# the offline front end over the same seconds of audio (bench.py's front_end is this quantity per minute)
lm = ops.LogMel('cuda', sr=SA.SR, n_fft=config['feature']['fft_bins'], hop=hop, n_mels=config['feature']['mel_bins'], log_offset=config['feature']['log_offset'])
offline = {r: [] for r in rates}
for r in rates:
    n = int(round(SEC * r))
    piece = waves[r][:n].cuda()
    for k in range(WARM):
        lm(ops.resample(piece, r, SA.SR) if r != SA.SR else piece)
for rep in range(args.repeats):
    k = WARM + rep
    for key, fn, sec in shapes:
        sec.append(round(timed(lambda: fn(k)), 6))
    for r in rates:
        n = int(round(SEC * r))
        piece = waves[r][:n].cuda()
        offline[r].append(round(timed(lambda: lm(ops.resample(piece, r, SA.SR) if r != SA.SR else piece)), 6))
    print('done: repeat %d' % rep, file=sys.stderr, flush=True)
lines = [{'model': k[0], 'rate': k[1], 'call': k[2], 'S': k[3], 'seconds': pct(sec), 'all': sec, 'real_time': pct(sec)['median'] < SEC} for k, _, sec in shapes]
best = {}
for l in lines:
    if l['real_time']:
        key = '%s/%d/%s' % (l['model'], l['rate'], l['call'])
        best[key] = max(best.get(key, 0), l['S'])
result = {'tool': 'tools/bench_stream_wave.py', 'label': os.path.basename(ROOT) if ROOT != os.path.dirname(os.path.dirname(os.path.abspath(__file__))) else 'this',
          'has_open_stream_sr': HAS_SR, 'repeats': args.repeats, 'audio_seconds_per_push': SEC, 'precision': args.precision, 'lines': lines,
          'offline_front_end_seconds': {str(r): pct(v) for r, v in offline.items()}, 'largest_real_time_S_tried': best}
out = args.out or os.path.join(ROOT, 'profiles', 'stream_wave_mi355x.json')
with open(out, 'w') as fh:
    json.dump(result, fh, indent=1)
print(json.dumps(result))
