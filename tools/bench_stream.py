#!/usr/bin/env python3
"""The streaming note decoder on a GPU box: the cost of one hftt_notes_stream_step, its independence of the stream's age, and the end-to-end
cost of a push (AMT.open_stream).  One process, warm-up first, interleaved repeats, medians with p10 / p90.

  step        128 new rows at N = 88 for S = 1 and S = 32 streams (random posteriors of tests/notes_stream_emul.py::tracks, tiled), timed with
              device events around ops.notes_stream_step without its copy back (host=False) and with room for every note (these tracks
              give some 1,300 notes per stream and step, far above the default room, and a step without room runs twice); the yardstick
              is hftt_notes_decode_seg over the same 128 * S rows as S segments.
  age         the same step at step number 10 and at step number 1,000 of one stream (ring of 512 rows: several wraps), the same 128 rows
              each time; the two p10-p90 ranges must overlap (bounded work, not a speed target).
  end to end  pushes of one clip's worth of frames (num_frame) per stream into AMT.open_stream, tiny trained and paper-size random-init
              model, S = 1, 2, 4, ... : seconds per push against the audio it covers; the largest S that stays below real time.

Writes profiles/notes_stream_mi355x.json and prints it.  Usage: python tools/bench_stream.py [x3|bf16] [repeats]"""
import json, os, pickle, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'nylon-amt_amd')); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch
import bench                                  # paper-size workload table + model builder (no oracle on this path)
import notes_stream_emul as E
from corpus import synth_audio as SA
from hftt_hip import ops
from model.amt import AMT

precision = sys.argv[1] if len(sys.argv) > 1 else 'x3'
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 9
dev = torch.device('cuda')
N, ROWS, H = 88, 128, 512
HOP = E.HOP


def pct(v):
    v = sorted(v)
    q = lambda p: v[min(len(v) - 1, int(p * len(v)))]
    return {'median': q(0.5), 'p10': q(0.1), 'p90': q(0.9)}


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def feed(st, rows):
    """the same 128 rows behind every stream's row_end (ring rows are a multiple of 128: no wrap inside a block)"""
    for s in range(st.S):
        r0 = st.row_end[s] % st.H
        for ring, a in zip(st.rings, rows):
            ring[s, r0:r0 + ROWS] = a
    st.deliver([ROWS] * st.S)


def step_cost(S):
    tr = E.tracks(5, ROWS, N)
    rows = [torch.from_numpy(a).to(dev) for a in tr]
    st = ops.notes_stream_state(S, N, H, dev)
    seg = [torch.cat([r] * S, dim=0).contiguous() for r in rows]
    seg_rows = [ROWS * s for s in range(S + 1)]
    kw = dict(thred_onset=0.6, thred_offset=0.55, thred_mpe=0.5)
    legs = {'stream_step': [], 'decode_seg': []}
    notes = 0
    for k in range(3 + repeats):
        feed(st, rows)
        out = []
        t = event_ms(lambda: out.append(ops.notes_stream_step(st, HOP, host=False, capacity=S * N * ROWS // 4, **kw)))
        u = event_ms(lambda: ops.notes_decode_seg(*seg, seg_rows, HOP, **kw))
        if k >= 3:
            legs['stream_step'].append(round(t, 4)); legs['decode_seg'].append(round(u, 4))
            notes = int(out[0][0].numel())
    return {'S': S, 'rows_per_stream': ROWS, 'N': N, 'notes_per_step': notes, 'ms': legs, 'stats_ms': {k: pct(v) for k, v in legs.items()}}


def age():
    tr = E.tracks(6, ROWS, N)
    rows = [torch.from_numpy(a).to(dev) for a in tr]
    kw = dict(thred_onset=0.6, thred_offset=0.55, thred_mpe=0.5)
    ms = {10: [], 1000: []}
    for rep in range(repeats):
        st = ops.notes_stream_state(1, N, H, dev)
        for k in range(1, 1001):
            feed(st, rows)
            if k in ms:
                ms[k].append(round(event_ms(lambda: ops.notes_stream_step(st, HOP, host=False, capacity=N * ROWS // 4, **kw)), 4))
            else:
                ops.notes_stream_step(st, HOP, host=False, capacity=N * ROWS // 4, **kw)
    stats = {str(k): pct(v) for k, v in ms.items()}
    a, b = stats['10'], stats['1000']
    return {'ring_rows': H, 'rows_per_step': ROWS, 'ms': {str(k): v for k, v in ms.items()}, 'stats_ms': stats,
            'ranges_overlap': a['p10'] <= b['p90'] and b['p10'] <= a['p90']}


def end_to_end(mname, path):
    config = SA.default_config()
    T = config['input']['num_frame']
    amt = AMT(config, path, batch_size=32)
    wave = SA.pluck_wave(SA.pluck_notes(77, 30.0), 30.0, SA.SR, device='cuda')
    feat = amt.wave2feature(wave.unsqueeze(0), SA.SR, on_device=True)
    audio = T * config['feature']['hop_sample'] / config['feature']['sr']
    runs, best = [], 0
    S = 1
    while S <= 256:
        st = amt.open_stream(n_streams=S)
        sec = []
        for k in range(feat.shape[0] // T):
            torch.cuda.synchronize()
            t0 = time.time()
            st.push([feat[k * T:(k + 1) * T]] * S)
            sec.append(time.time() - t0)
        st.close()
        stats = pct([round(x, 5) for x in sec[2:]])                             # the first pushes build plans and find no ready clip
        runs.append({'S': S, 'seconds_per_push': stats, 'audio_seconds_per_push': audio, 'real_time': stats['median'] < audio})
        print('done: %s S=%d %s' % (mname, S, json.dumps(stats)), file=sys.stderr, flush=True)
        if stats['median'] >= audio:
            break
        best = S
        S *= 2
    return {'model': mname, 'pushes_of_frames': T, 'runs': runs, 'largest_real_time_S_tried': best}


result = {'tool': 'tools/bench_stream.py', 'repeats': repeats, 'step': [step_cost(1), step_cost(32)], 'age': age()}
print('done: step and age', file=sys.stderr, flush=True)
tmp = tempfile.mkdtemp()
paper = bench.build_model(bench.CONFIGS['paper'], 1234, 0.1, 'cpu')
paper.hftt_precision = precision
with open(os.path.join(tmp, 'paper.pkl'), 'wb') as fh:
    pickle.dump(paper, fh, protocol=4)
result['end_to_end'] = [end_to_end('tiny_trained', os.path.join(ROOT, 'tests', 'golden', 'config5_tiny_trained.pkl')),
                        end_to_end('paper_random_init_%s' % precision, os.path.join(tmp, 'paper.pkl'))]
out = os.path.join(ROOT, 'profiles', 'notes_stream_mi355x.json')
if os.environ.get('HFTT_BENCH_OUT'):
    out = os.environ['HFTT_BENCH_OUT']
with open(out, 'w') as fh:
    json.dump(result, fh, indent=1)
print(json.dumps(result))
