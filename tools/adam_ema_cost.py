#!/usr/bin/env python3
"""What carrying the averaged weights costs the optimizer launch (GPU box): hftt_adam_step (adam_kernel, 28 B per element: p, g, m, v read,
p, m, v written) against hftt_adam_step_ema (adam_ema_kernel, 44 B: ema and ema_c read and written on top) over flat buffers of the model's
own length, alone on the device.  Both launches in ONE process, timed with device events around `--launches` back-to-back launches per
sample, in interleaved rounds whose order alternates (the A/B rule), plus the plain launch a second time as the run's
own repeatability.

  python tools/adam_ema_cost.py [--config paper] [--rounds 12] [--launches 200] [--out profiles/adam_ema_cost.json]

One JSON line, also written to --out: the flat length, microseconds per launch (series, medians), the ratio against the traffic ratio
44 / 28, and the bytes per second each median amounts to (bytes counted from the shapes)."""
import argparse, json, os, sys
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
    ap.add_argument('--rounds', type=int, default=12)
    ap.add_argument('--launches', type=int, default=200, help='back-to-back launches per timed sample')
    ap.add_argument('--out', default='profiles/adam_ema_cost.json')
    args = ap.parse_args()
    from hftt_hip import ops
    from hftt_hip.layout import flat_offsets
    dev = torch.device('cuda:0')
    model = bench.build_model(bench.CONFIGS[args.config], 1, 0.1, 'cpu')
    _, n = flat_offsets((name, p.numel()) for name, p in model.named_parameters())
    g = torch.Generator().manual_seed(3)
    p, grad, ema = (torch.randn(n, generator=g).to(dev) * s for s in (0.05, 1e-3, 0.05))
    m, v, c = (torch.zeros(n, device=dev) for _ in range(3))
    step = [0]

    def plain():
        step[0] += 1
        ops.adam_step(p, grad, m, v, step[0], lr=1e-4)

    def averaged():
        step[0] += 1
        ops.adam_step_ema(p, grad, m, v, ema, c, step[0], 0.9999, lr=[1e-4])

    def sample(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.launches):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / args.launches * 1e3          # microseconds per launch

    cases = (('adam_step', plain), ('adam_step_ema', averaged), ('adam_step_again', plain))
    for _, fn in cases:
        sample(fn)
    series = {k: [] for k, _ in cases}
    for i in range(args.rounds):
        for name, fn in (cases if i % 2 == 0 else cases[::-1]):
            series[name].append(round(sample(fn), 3))
    med = {k: round(median(x), 3) for k, x in series.items()}
    nbytes = {'adam_step': 28 * n, 'adam_step_ema': 44 * n, 'adam_step_again': 28 * n}
    line = {'workload': 'the optimizer launch alone over flat buffers of the %s model\'s length, %d launches per sample, %d interleaved rounds, device events'
                        % (args.config, args.launches, args.rounds),
            'flat_elements': n, 'bytes_per_launch': nbytes, 'us_per_launch': series, 'us_per_launch_median': med,
            'us_per_launch_min': {k: min(x) for k, x in series.items()},
            'plain_spread_us': round(abs(med['adam_step'] - med['adam_step_again']), 3),
            'ema_over_plain_median': round(med['adam_step_ema'] / med['adam_step'], 4), 'traffic_ratio': round(44 / 28, 4),
            'tb_per_s_at_median': {k: round(nbytes[k] / (med[k] * 1e-6) / 1e12, 3) for k in med}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(line, fh, indent=1)
    print(json.dumps(line))


if __name__ == '__main__':
    main()
