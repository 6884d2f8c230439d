#!/usr/bin/env python3
"""What the guarded optimizer step costs (GPU box): the training step of bench.py's workload (paper size, B = 8, default precision mode, dropout
0.1) with the plain FusedAdam against FusedAdam(guard=True, max_grad_norm=1.0), two TrainSteps in ONE process measured in interleaved pairs
(the A/B rule), plus the optimizer launches alone on the same flat buffers by device events.

  python tools/guard_step_cost.py [--config paper] [--batch 8] [--pairs 15] [--steps 10] [--out profiles/guard_step_cost.json]

One JSON line; both series and their medians go to --out (the record kept in profiles/)."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'nylon-amt_amd'))
import torch
import bench


def median(xs):
    s = sorted(xs)
    return s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='paper', choices=['paper', 'tiny'])
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--pairs', type=int, default=15)
    ap.add_argument('--steps', type=int, default=10, help='training steps per timed sample')
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default='profiles/guard_step_cost.json')
    args = ap.parse_args()
    from hftt_hip import ops
    from hftt_hip.trainer import FusedAdam, TrainStep
    dev = torch.device('cuda:0')
    cfg = bench.CONFIGS[args.config]
    spec, labels = bench.synthetic_batch(cfg, args.batch, 7, dev)
    steps = {}
    for name, kw in (('plain', {}), ('guarded', dict(guard=True, max_grad_norm=1.0))):
        model = bench.build_model(cfg, 1, 0.1, dev)
        model.train()
        steps[name] = TrainStep(model, optimizer=FusedAdam(model, lr=1e-4, **kw))

    def sample(ts, k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            ts(spec, *labels)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / k * 1e3

    for ts in steps.values():
        sample(ts, args.warmup)
    series = {'plain': [], 'guarded': []}
    for i in range(args.pairs):
        order = ('plain', 'guarded') if i % 2 == 0 else ('guarded', 'plain')          # alternate who goes first
        for name in order:
            series[name].append(round(sample(steps[name], args.steps), 4))
    g = steps['guarded'].opt
    # the optimizer launches alone, on the guarded engine's flat buffers, after the timed series (lr = 0: the parameters stay, the moments are not used again)
    eng = steps['guarded'].engine
    p, gr, m, v = eng.flat_params, eng.flat_grads, g.exp_avg, g.exp_avg_sq
    ctl, ws = ops.guard_buffers(p.numel(), dev)

    def events(fn, reps=200):
        for _ in range(10):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps * 1e3

    def guarded_launches():
        ops.grad_norm(gr, ctl, ws, max_norm=1.0)
        ops.adam_step_guarded(p, gr, m, v, 100, ctl, lr=0.0)
    kernels_us = {'adam_step': round(events(lambda: ops.adam_step(p, gr, m, v, 100, lr=0.0)), 2),
                  'grad_norm': round(events(lambda: ops.grad_norm(gr, ctl, ws, max_norm=1.0)), 2),
                  'grad_norm_plus_adam_step_guarded': round(events(guarded_launches), 2)}
    med = {k: round(median(x), 4) for k, x in series.items()}
    line = {'workload': 'TrainStep, %s size, B = %d, default precision mode, dropout 0.1: FusedAdam() against FusedAdam(guard=True, max_grad_norm=1.0), '
                        'interleaved pairs in one process, %d steps per sample' % (args.config, args.batch, args.steps),
            'flat_parameters': int(p.numel()), 'flat_gradient_MB': round(p.numel() * 4 / 1e6, 2),
            'step_ms': series, 'step_ms_median': med, 'step_ms_min': {k: min(x) for k, x in series.items()},
            'guarded_minus_plain_ms_median': round(med['guarded'] - med['plain'], 4),
            'guarded_over_plain_median': round(med['guarded'] / med['plain'], 5),
            'paired_difference_ms': [round(b - a, 4) for a, b in zip(series['plain'], series['guarded'])],
            'optimizer_launches_alone_us': kernels_us,
            'guarded_run': {'skipped_steps': g.skipped_steps, 'clipped_steps': g.clipped_steps, 'last_grad_norm': float(g.grad_norm),
                            'last_clip_coef': float(g.clip_coef)}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(line, fh, indent=1)
    print(json.dumps(line))


if __name__ == '__main__':
    main()
