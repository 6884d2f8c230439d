#!/usr/bin/env python3
"""Launch time of hftt_loss_w against hftt_loss from the same library, on the same inputs (GPU box).

  python tools/loss_w_cost.py [--rounds 20] [--calls 200] [--out profiles/loss_w_cost.json]

n = 8 * 128 * 88 label elements, V = 128 (the paper configuration at batch 8), gradients written.  Four entries, timed in alternation
(round by round, so that a drift of the shared host lands on all of them): hftt_loss; hftt_loss_w neutral (two launches); BCE options only
(per-pitch pos_weight and gamma 2 on all six heads, two launches); CE options with the pre-pass (class weights, smoothing 0.1, an
ignore_index inside [0, V): three launches).  A round is `calls` back-to-back calls between two device events, after a warm-up of every
entry; reported: the median over the rounds of the time per call and the spread (min, max).  The bytes a call must move are computed from
the shapes, so that the time can be read against the memory system.  One JSON line; no ratio is asserted."""
import argparse, ctypes as C, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'nylon-amt_amd'))
import torch
from hftt_hip import _capi

N, V, NN = 8 * 128 * 88, 128, 88


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('loss_w_cost: no GPU (a launch time is measured on the device or not at all)')
    dev = torch.device('cuda:0')
    L = _capi.lib()
    g = torch.Generator().manual_seed(1)
    probs = [torch.rand(N, generator=g).clamp_(1e-4, 1 - 1e-4).to(dev) for _ in range(6)]
    vel = [(torch.randn(N, V, generator=g) * 3).to(dev) for _ in range(2)]
    labels = [(torch.rand(N, generator=g) * (torch.rand(N, generator=g) < 0.02)).to(dev) for _ in range(2)] + [(torch.rand(N, generator=g) < 0.05).float().to(dev)]
    lv = (torch.randint(1, V, (N,), generator=g) * (torch.rand(N, generator=g) < 0.05)).to(dev)
    d_prob = [torch.empty(N, device=dev) for _ in range(6)]
    d_vel = [torch.empty(N, V, device=dev) for _ in range(2)]
    out = torch.zeros(16, device=dev)
    ws = torch.empty(L.hftt_loss_ws_bytes(N) // 4 + 16, device=dev)
    ws_w = torch.empty(L.hftt_loss_w_ws_bytes(N) // 4, device=dev)
    ramp = (0.5 * 16.0 ** (torch.arange(NN, dtype=torch.float64) / (NN - 1))).float().to(dev)
    cw = torch.ones(V, device=dev)
    cw[0] = 0.1

    def desc(pos_weight=None, gamma=0.0, class_weight=None, smoothing=0.0, ignore=-100):
        dw = _capi.LossWDesc()
        b = dw.base
        b.n, b.V = N, V
        for i in range(6):
            b.prob[i], b.d_prob[i] = probs[i].data_ptr(), d_prob[i].data_ptr()
            dw.pos_weight[i], dw.gamma[i] = (None if pos_weight is None else pos_weight.data_ptr()), gamma
        for s in range(2):
            b.vel[s], b.d_vel[s] = vel[s].data_ptr(), d_vel[s].data_ptr()
            dw.class_weight[s], dw.smoothing[s], dw.ignore_index[s] = (None if class_weight is None else class_weight.data_ptr()), smoothing, ignore
        b.label_onset, b.label_offset, b.label_mpe, b.label_velocity = labels[0].data_ptr(), labels[1].data_ptr(), labels[2].data_ptr(), lv.data_ptr()
        b.weight_A, b.weight_B, b.grad_scale = 1.0, 1.0, 1.0
        b.loss_out, b.ws = out.data_ptr(), ws.data_ptr()
        dw.Nn, dw.ws_w = NN, ws_w.data_ptr()
        return dw
    entries = {
        'hftt_loss': (desc(), True),
        'hftt_loss_w_neutral': (desc(), False),
        'hftt_loss_w_bce_options': (desc(pos_weight=ramp, gamma=2.0), False),
        'hftt_loss_w_ce_options_prepass': (desc(class_weight=cw, smoothing=0.1, ignore=3), False),
    }
    stream = torch.cuda.current_stream(dev).cuda_stream

    def call(name):
        dw, plain = entries[name]
        if plain:
            _capi.check(L.hftt_loss(C.byref(dw.base), stream), 'loss')
        else:
            _capi.check(L.hftt_loss_w(C.byref(dw), stream), 'loss_w')
    for name in entries:                                   # warm-up: code objects loaded, every shape seen
        for _ in range(20):
            call(name)
    torch.cuda.synchronize(dev)
    times = {name: [] for name in entries}
    for _ in range(args.rounds):
        for name in entries:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.calls):
                call(name)
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / args.calls)          # microseconds per call
    # bytes a call must move: 6 posteriors + 3 label tracks + 6 gradients (fp32), the int64 labels, two logit tensors read and two written
    moved = N * 4 * (6 + 3 + 6) + N * 8 + 4 * N * V * 4
    res = {'n': N, 'V': V, 'Nn': NN, 'rounds': args.rounds, 'calls_per_round': args.calls, 'bytes_per_call': moved,
           'prepass_extra_bytes': N * 8, 'us_per_call': {}}
    for name, t in times.items():
        med = statistics.median(t)
        res['us_per_call'][name] = {'median': round(med, 2), 'min': round(min(t), 2), 'max': round(max(t), 2), 'GB_per_s_at_median': round(moved / med / 1e3, 1)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
