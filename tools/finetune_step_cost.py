#!/usr/bin/env python3
"""What freezing stages saves (GPU box): the training step of bench.py's workload (paper size, B = 8, default precision mode, dropout 0.1)
all-trainable, with the encoder frozen, with encoder + frequency decoder frozen, and all-trainable AGAIN (a second, identically built
TrainStep: the run's own repeatability).  Four TrainSteps in ONE process, measured in interleaved rounds whose order rotates (DESIGN.md
section 8: the A/B rule).  The frozen steps run the pruned backward (HfttEngine.backward(frozen_stages=...)) and the grouped Adam kernel;
the forward plan is the same in all four.

  python tools/finetune_step_cost.py [--config paper] [--batch 8] [--rounds 12] [--steps 10] [--out profiles/finetune_step_cost.json]

One JSON line, also written to --out: ms per step (series, medians), launches per backward plan, the Adam step's bytes per step (counted
from the shapes: 28 bytes per trainable element -- p, g, m, v read, p, m, v written -- plus one map byte per quad in the grouped kernel),
and whether each pruned step is faster than the all-trainable step by more than the spread between the run's two all-trainable medians."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'nylon-amt_amd'))
import torch
import bench

CASES = (('all', {}), ('encoder', dict(encoder=dict(frozen=True))), ('encoder+freq', dict(encoder=dict(frozen=True), freq=dict(frozen=True))),
         ('all_again', {}))


def median(xs):
    s = sorted(xs)
    return s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='paper', choices=['paper', 'tiny'])
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--rounds', type=int, default=12)
    ap.add_argument('--steps', type=int, default=10, help='training steps per timed sample')
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default='profiles/finetune_step_cost.json')
    args = ap.parse_args()
    from hftt_hip.trainer import FusedAdam, TrainStep, stage_groups
    dev = torch.device('cuda:0')
    cfg = bench.CONFIGS[args.config]
    spec, labels = bench.synthetic_batch(cfg, args.batch, 7, dev)
    steps = {}
    for name, kw in CASES:
        model = bench.build_model(cfg, 1, 0.1, dev)
        model.train()
        steps[name] = TrainStep(model, optimizer=FusedAdam(stage_groups(model, **kw) if kw else model, lr=1e-4))

    def sample(ts, k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            ts(spec, *labels)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / k * 1e3

    for ts in steps.values():
        sample(ts, args.warmup)
    names = [n for n, _ in CASES]
    series = {n: [] for n in names}
    for i in range(args.rounds):
        for name in names[i % 4:] + names[:i % 4]:            # rotate who goes first
            series[name].append(round(sample(steps[name], args.steps), 4))
    med = {k: round(median(x), 4) for k, x in series.items()}
    spread = abs(med['all'] - med['all_again'])
    slower_all = max(med['all'], med['all_again'])
    faster_all = min(med['all'], med['all_again'])
    plans, adam = {}, {}
    for name in names[:3]:
        ts = steps[name]
        k = ts.opt.frozen_stages()
        plan, _ = ts.engine.backward_plan(args.batch, k)
        n = ts.engine.flat_params.numel()
        frozen = ts.opt._group_map()['frozen_elements']
        plans[name] = {'frozen_stages': k, 'backward_launches': len(plan), 'forward_launches': len(ts.engine.workspace(args.batch)['fwd'])}
        adam[name] = {'flat_elements': n, 'trainable_elements': n - frozen, 'bytes_per_step': 28 * (n - frozen) + (n // 4 if k else 0)}
    line = {'workload': 'TrainStep, %s size, B = %d, default precision mode, dropout 0.1: all trainable / encoder frozen / encoder + frequency decoder frozen / '
                        'all trainable again, interleaved rounds in one process, %d steps per sample' % (args.config, args.batch, args.steps),
            'step_ms': series, 'step_ms_median': med, 'step_ms_min': {k: min(x) for k, x in series.items()},
            'all_trainable_spread_ms': round(spread, 4),
            'pruned_over_all_median': {k: round(med[k] / med['all'], 5) for k in ('encoder', 'encoder+freq')},
            'saved_ms_against_the_faster_all_trainable_median': {k: round(faster_all - med[k], 4) for k in ('encoder', 'encoder+freq')},
            'faster_than_all_by_more_than_the_spread': {k: bool(slower_all - med[k] > spread and faster_all - med[k] > spread) for k in ('encoder', 'encoder+freq')},
            'plans': plans, 'adam_step': adam}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(line, fh, indent=1)
    print(json.dumps(line))


if __name__ == '__main__':
    main()
