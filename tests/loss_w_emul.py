"""fp32 restatement, fp64 reference and rounding-model criteria of the fused loss with class-balanced and focal criteria (csrc/loss_w.hip:
hftt_loss_w; definitions in include/hftt_hip.h), in the manner of tests/elementwise_emul.py, whose constants, inputs and loss bounds it
reuses: a head or side whose options are neutral is held to loss_ref's bounds, term by term (the counts below reduce to them).

  loss_w_ref    fp64 evaluation of the definitions (the kernels' clamps included) and the bounds;
  loss_w_emul   loss_w_kernel / loss_w_v4_kernel + loss_w_pre_kernel + loss_w_reduce_kernel in fp32, in the kernels' operation order (the two
                forms share every formula; reductions are torch.sum in fp32, the bounds are written for the kernels' deeper trees);
                defect=<name> selects one deliberately wrong variant (DEFECTS);
  loss_w_check  |got - ref| <= bound for loss_out[0..10] and every gradient element; returns the violations (empty = pass).
tests/test_loss_w_emul_bound.py shows on the CPU that the restatement passes and every defect fails; tests/test_loss_w_gpu.py holds the
kernels to the same bounds.
"""
import numpy as np
import torch

import elementwise_emul as E
from elementwise_emul import C_DIV, C_EXP, C_LOG, F32_TINY, K_SOFT, LOSS_D, LOSS_W, U32, f32, violations

DEFECTS = ('pos_weight_on_negative_part', 'pitch_el_div_Nn', 'ce_mean_over_n', 'ignored_rows_get_gradient', 'smoothing_without_class_weights',
           'focal_factor_constant_in_gradient', 'grad_scale_missing_from_focal_term')
IGNORE = 2                # the ignore_index the option sets use where they ignore (inside [0, V) for every V of SHAPES)
PRE_WGS = 256             # csrc/loss_w.hip: workgroups of the label pre-pass (256 threads each)

# (kernel form, V, n, Nn, grad_scale).  Forms as elementwise_emul.LOSS_CASES: 'v4' (aligned, V % 4 == 0, V <= 128: 8 elements per workgroup),
# 'general' (V > 128) and 'general_unaligned' (V = 128 through views offset by one element): 4 elements per workgroup.  n: one workgroup, odd n,
# one n just past the first grid pass (4096 workgroups: 32768 resp. 16384 elements).  Nn in {1, 3, 88} with n a multiple of Nn that is no
# multiple of 8 -- but for Nn = 88 = 8 * 11, where every multiple is one: 264 = 3 * 88 is an odd multiple.
SHAPES = (
    ('v4', 128, 8, 1, 1.0), ('v4', 128, 261, 3, 0.25), ('v4', 128, 264, 88, 1.0), ('v4', 128, 32769, 3, 0.25),
    ('v4', 4, 5, 1, 0.25), ('v4', 4, 261, 3, 1.0),
    ('general', 129, 3, 3, 1.0), ('general', 129, 130, 1, 0.25), ('general', 256, 514, 1, 1.0), ('general', 256, 264, 88, 0.25),
    ('general_unaligned', 128, 123, 3, 1.0), ('general_unaligned', 128, 16389, 3, 0.25),
)
OPTION_SETS = ('neutral', 'onset_A_only', 'bce', 'ce', 'ce_b', 'all', 'ignore_all')


def options(name, V, n, Nn, lv):
    """(opts, labels): opts = pos_weight[6] ([Nn] fp32 or None), gamma[6], class_weight[2] ([V] fp32 or None), smoothing[2], ignore[2];
    labels = lv with the ignored rows written in.
      neutral       nothing set
      onset_A_only  pos_weight 4 on head 0 alone
      bce           scalar weights 4 and 0.5, a per-pitch ramp 0.5 .. 8, gamma 0, 1, 1.5 and 2 over the six heads; the CE sides neutral (no pre-pass)
      ce            side A: class weights in [0.5, 2] with ONE ZERO entry, smoothing 0.1, nothing ignored; side B: no weights, smoothing 0,
                    ignore_index hitting every 7th row
      ce_b          side A neutral INSIDE a call with a pre-pass; side B: weights, smoothing 0.1 and ignore_index hitting every 7th row
      all           bce + ce_b's side B on both sides (side A without smoothing)
      ignore_all    side A: every label is the ignore_index (W = 0); side B: an ignore_index inside [0, V) that no label has"""
    g = torch.Generator().manual_seed(7000 + 10 * V + Nn)
    ramp = (0.5 * 16.0 ** (torch.arange(Nn, dtype=torch.float64) / max(Nn - 1, 1))).float()
    four, half = torch.full((Nn,), 4.0), torch.full((Nn,), 0.5)
    cw = 0.5 + 1.5 * torch.rand(V, generator=g)
    cw[1] = 0.0
    cw2 = 0.5 + 1.5 * torch.rand(V, generator=g)
    cw2[V - 1] = 0.0
    o = dict(Nn=Nn, pos_weight=[None] * 6, gamma=[0.0] * 6, class_weight=[None, None], smoothing=[0.0, 0.0], ignore=[-100, -100])
    lv = lv.clone()
    if name in ('bce', 'all'):
        o['pos_weight'] = [four, ramp, None, ramp, None, half]
        o['gamma'] = [0.0, 1.0, 1.5, 2.0, 2.0, 0.0]
    if name == 'onset_A_only':
        o['pos_weight'][0] = four
    if name == 'ce':
        o['class_weight'], o['smoothing'], o['ignore'] = [cw, None], [0.1, 0.0], [-100, IGNORE]
        lv[::7] = IGNORE
    if name == 'ce_b':
        o['class_weight'], o['smoothing'], o['ignore'] = [None, cw], [0.0, 0.1], [-100, IGNORE]
        lv[::7] = IGNORE
    if name == 'all':
        o['class_weight'], o['smoothing'], o['ignore'] = [cw2, cw], [0.0, 0.1], [IGNORE, IGNORE]
        lv[::7] = IGNORE
    if name == 'ignore_all':
        o['ignore'] = [3, IGNORE]
        lv[:] = 3
    return o, lv


def case(shape, opt, seed=0):
    """inputs of elementwise_emul.loss_inputs (saturated posteriors against both kinds of target, the +-80 logit row) with the option set"""
    _, V, n, Nn, gs = shape
    c = E.loss_inputs(V, n, seed)
    o, lv = options(opt, V, n, Nn, c['lv'])
    return dict(c, lv=lv, opts=o, gs=gs)


def needs_prepass(o, V):
    return [o['class_weight'][s] is not None or 0 <= o['ignore'][s] < V for s in range(2)]


def pre_depth(n):
    """roundings on W's summation path: a thread's labels in sequence, 6 for the 64 lanes, 2 for the four waves, and the same 6 + 2 again
    where the partials are summed"""
    n_pre = min(PRE_WGS, -(-n // 256))
    return -(-n // (n_pre * 256)) + 16


def _pitch(n, Nn, dev, defect=None):
    el = torch.arange(n, device=dev)
    return (el // Nn).clamp_max(Nn - 1) if defect == 'pitch_el_div_Nn' else el % Nn


# ================================================================================================ fp32 restatement
def loss_w_emul(c, defect=None):
    """returns out[11], d_prob[6], d_vel[2] -- csrc/loss_w.hip's arithmetic in fp32, contraction off as there"""
    assert defect is None or defect in DEFECTS
    n, V, o, gs = c['n'], c['V'], c['opts'], f32(c['gs'])
    F = lambda x: torch.tensor(x, dtype=torch.float32)      # noqa: E731
    inv_n = f32(1.0 / np.float32(n))
    bce, d_prob = [], []
    for h in range(6):
        p, y = c['probs'][h], E._bce_labels(c, h)
        a = torch.ones(n) if o['pos_weight'][h] is None else o['pos_weight'][h][_pitch(n, o['Nn'], p.device, defect)]
        gam = f32(o['gamma'][h])
        lp, l1p = torch.log(p).clamp_min(-100.0), torch.log1p(-p).clamp_min(-100.0)
        t2 = (1.0 - y) * l1p
        if defect == 'pos_weight_on_negative_part':
            t2 = (a * (1.0 - y)) * l1p
        nbase = (a * y) * lp + t2
        num = (p - y) - ((a - 1.0) * y) * (1.0 - p)
        den = ((1.0 - p) * p).clamp_min(f32(1e-12))
        w = LOSS_W[0] if h < 3 else LOSS_W[1]
        scale = f32(np.float32(w) * np.float32(inv_n) * np.float32(gs))
        if gam == 0.0:
            bce.append((-nbase).sum() / n)
            d_prob.append(num / den * scale)
            continue
        df = y - p
        ad = df.abs()
        m1 = torch.ones(n) if gam == 1.0 else torch.exp(F(gam - 1.0) * torch.log(ad))
        m = ad * m1
        bce.append((-(m * nbase)).sum() / n)
        t2g = nbase * ((F(gam) * m1) * torch.sign(df))
        if defect == 'focal_factor_constant_in_gradient':
            t2g = torch.zeros(n)
        if defect == 'grad_scale_missing_from_focal_term':
            d_prob.append((m * num) / den * scale + t2g * f32(np.float32(w) * np.float32(inv_n)))
        else:
            d_prob.append(((m * num) / den + t2g) * scale)
    pre = needs_prepass(o, V)
    lv = c['lv']
    in_range = (lv >= 0) & (lv < V)
    onehot = torch.nn.functional.one_hot(lv.clamp(0, V - 1), V).bool() & in_range[:, None]
    ce, d_vel, Ws = [], [], []
    for s in range(2):
        cw = torch.ones(V) if o['class_weight'][s] is None else o['class_weight'][s]
        live = lv != o['ignore'][s]
        wl = torch.where(in_range, cw[lv.clamp(0, V - 1)], torch.zeros(())) if o['class_weight'][s] is not None else torch.ones(n)
        W = (wl * (live & in_range)).sum() if pre[s] else F(float(n))
        if defect == 'ce_mean_over_n':
            W = F(float(n))
        on = bool(W > 0)
        omeps = f32(np.float32(1.0) - np.float32(o['smoothing'][s]))
        epsV = f32(np.float32(o['smoothing'][s]) / np.float32(V))
        inv_W = (1.0 / W) if on else F(0.0)
        wfac = (F(LOSS_W[s]) * inv_W) * F(gs)
        lg = c['vel'][s]
        mx = lg.max(1, keepdim=True).values
        ex = torch.exp(lg - mx)
        ssum = ex.sum(1, keepdim=True)
        lse = mx + torch.log(ssum)
        picked = torch.where(onehot, lg, torch.zeros(())).sum(1)
        coef = F(omeps) * wl
        row = coef * (lse[:, 0] - picked)
        sumw = cw.sum()
        cws = cw
        if defect == 'smoothing_without_class_weights':
            cws, sumw = torch.ones(V), F(float(V))
        if epsV != 0.0:
            row = row + F(epsV) * (cws[None, :] * (lse - lg)).sum(1)
        live_v = live & on
        total = torch.where(live_v, row, torch.zeros(())).sum()
        ce.append(total / W if on else F(0.0))
        q = ex * (1.0 / ssum)
        gq = (q - onehot.float()) * coef[:, None]
        if epsV != 0.0:
            gq = gq + F(epsV) * (q * sumw - cws[None, :])
        gq = gq * wfac
        if defect != 'ignored_rows_get_gradient':
            gq = torch.where(live_v[:, None], gq, torch.zeros(()))
        d_vel.append(gq)
        Ws.append((wl * (live & in_range)).sum() if pre[s] else F(float(n)))
    t = [bce[0], bce[1], bce[2], ce[0], bce[3], bce[4], bce[5], ce[1]]
    la = ((t[0] + t[1]) + t[2]) + t[3]; lb = ((t[4] + t[5]) + t[6]) + t[7]
    out = torch.stack([LOSS_W[0] * la + LOSS_W[1] * lb] + t + Ws)
    return out, d_prob, d_vel


# ================================================================================================ fp64 reference and bounds
def loss_w_ref(c):
    """fp64 evaluation of include/hftt_hip.h's definitions on the same fp32 inputs, and first-order bounds: U32 per fp32 rounding times a count
    read off csrc/loss_w.hip times the magnitude the rounding acts on (C_LOG, C_EXP, C_DIV, K_SOFT, LOSS_D: elementwise_emul).  Every count
    reduces to loss_ref's when the options are neutral, so neutral heads and sides are held to the existing yardstick.

    BCE head, element i.  base = P1 + P2 with P1 = a y (-lp), P2 = (1 - y)(-l1p), both >= 0:
        P1: a y 1 (exact when a == 1), log C_LOG, product 1; P2: (1 - y) 1, log C_LOG, product 1; sum 1:  k_b = 3 + C_LOG + [a != 1].
      m = ad * m1, ad = |y - p| (1), m1 = exp((g - 1) log ad): g - 1 is exact for g in [1, 4]; log ad carries C_LOG U32 |log ad| and ad's own
        rounding (U32, absolute on the log); the product with g - 1 one more on |(g - 1) log ad|; all absolute on the exponent, so relative on
        m1, plus C_EXP:   k_m1 = (g - 1) ((C_LOG + 1) |log ad| + 1) + C_EXP   (0 when g == 1: m1 = 1),   k_m = k_m1 + 2   (ad, product);
        an m1 below the normal range may be flushed: + F32_TINY absolute.
      value element m base: k_m + k_b + 1 (product); gamma == 0: k_b alone (no factor, no product).  Mean: + LOSS_D sum|.| / n, as loss_ref.
      gradient (T1 + T2) scale, T1 = m num / den, T2 = -base g m1 sign(y - p):
        num = A - B, A = p - y (1), B = ((a - 1) y)(1 - p) (4 on |B|), the subtraction 1 on |num| (a == 1: B = 0, the subtraction exact);
        den 2, division C_DIV, scale 3, last product 1 (loss_ref's 7 + C_DIV in all when gamma == 0 and a == 1);
        T1: k_m + 1 (m num) + 2 + C_DIV on |T1|, and err(num) m / den;  T2: k_b + k_m1 + 1 (g m1) + 1 (product) on |T2|;  T1 + T2: 1; scale 3 + 1.
    CE side.  t_c = lse - v_c >= 0 for any class c carries, as loss_ref's term: e(c) = K_SOFT + C_LOG |log s| + |lse| + |t_c|  (absolute, in U32).
      coef = (1 - eps) w[c_i]: k_c = [eps != 0] + [eps != 0 and weights]; the product coef t: + 1 unless coef is the exact 1 of a neutral side;
      S = sum_c w_c t_c: w_c e(c) + w_c t_c (product) each, depth 10 (the general form: 4 in sequence + 6 lane levels) on S (no cancellation);
      eps / V: C_DIV; the product with S 1; the sum of the two parts 1 on |row|.
      term = sum_live row / W: LOSS_D on sum|row| (the division by n counted there as in loss_ref), and W's own error pre_depth(n) U32 W when the
      pre-pass forms it (a sum of non-negative fp32 inputs; W = (float)n otherwise, exact).  loss_out[9], [10]: pre_depth(n) U32 W.
      gradient o = ((q - onehot) coef + (eps / V)(q sum_w - w_c)) wfac,  q = ex / s with loss_ref's k_q = C_EXP + 1 + K_SOFT + C_DIV + 1:
        first part: k_q q coef + (1 + k_c') |q - onehot| coef;  second: sum_w depth 10 (weights; exact V without), q sum_w: (k_q + 10 + 1) q sum_w,
        the subtraction 1, eps / V C_DIV + 1;  the sum 1;  wfac = weight / W * gs: 3 + pre_depth(n) when W is summed; last product 1;
        exp underflow (+-80 logits): F32_TINY (coef + (eps / V) sum_w) wfac absolute.  Neutral: wfac (k_q q + |d|) + 4 |o| = loss_ref's.
      Ignored rows, and every row when W == 0: exact zeros, bound 0."""
    n, V, o, gs = c['n'], c['V'], c['opts'], c['gs']
    dev = c['vel'][0].device
    wAB = LOSS_W
    bce, b_bce, d_prob, b_dprob = [], [], [], []
    for h in range(6):
        p, y = c['probs'][h].double(), E._bce_labels(c, h).double()
        pw = o['pos_weight'][h]
        a = torch.ones(n, dtype=torch.float64, device=dev) if pw is None else pw.to(dev).double()[_pitch(n, o['Nn'], dev)]
        g = float(f32(o['gamma'][h]))
        lp, l1p = torch.log(p).clamp_min(-100.0), torch.log1p(-p).clamp_min(-100.0)
        base = -(a * y * lp + (1.0 - y) * l1p)
        k_b = 3 + C_LOG + (a != 1.0).double()
        A, B = p - y, (a - 1.0) * y * (1.0 - p)
        num = A - B
        e_num = A.abs() + (a != 1.0).double() * (4 * B.abs() + num.abs())
        den = ((1.0 - p) * p).clamp_min(f32(1e-12))
        scale = (wAB[0] if h < 3 else wAB[1]) / n * gs
        if g == 0.0:
            ti = base
            bce.append(ti.sum() / n)
            b_bce.append(U32 * ((k_b + LOSS_D) * ti.abs()).sum() / n)
            gr = num / den * scale
            d_prob.append(gr)
            b_dprob.append(U32 * (e_num / den * scale + (6 + C_DIV) * gr.abs()))
            continue
        df = y - p
        ad = df.abs()
        m1 = ad.pow(g - 1.0) if g != 1.0 else torch.ones_like(ad)
        m = ad * m1
        lad = torch.where(ad > 0, torch.log(ad.clamp_min(1e-300)).abs(), torch.zeros_like(ad))
        k_m1 = ((g - 1.0) * ((C_LOG + 1) * lad + 1) + C_EXP) if g != 1.0 else torch.zeros_like(ad)
        k_m = k_m1 + 2
        ti = m * base
        bce.append(ti.sum() / n)
        b_bce.append((U32 * ((k_m + k_b + 1 + LOSS_D) * ti.abs()) + F32_TINY * ad * base).sum() / n)
        T1 = m * num / den
        T2 = -base * g * m1 * torch.sign(df)
        gr = (T1 + T2) * scale
        d_prob.append(gr)
        b_dprob.append(U32 * (scale * ((k_m + 3 + C_DIV) * T1.abs() + m / den * e_num + (k_b + k_m1 + 2) * T2.abs()) + 5 * gr.abs())
                       + scale * F32_TINY * (ad * num.abs() / den + base * g))
    pre = needs_prepass(o, V)
    D_PRE = pre_depth(n)
    lv = c['lv'].to(dev)
    in_range = (lv >= 0) & (lv < V)
    onehot = torch.nn.functional.one_hot(lv.clamp(0, V - 1), V).bool() & in_range[:, None]
    k_q = C_EXP + 1 + K_SOFT + C_DIV + 1
    ce, b_ce, d_vel, b_dvel, Ws, b_Ws = [], [], [], [], [], []
    for s in range(2):
        has_w = o['class_weight'][s] is not None
        cw = o['class_weight'][s].to(dev).double() if has_w else torch.ones(V, dtype=torch.float64, device=dev)
        eps = float(f32(o['smoothing'][s]))
        live = (lv != o['ignore'][s])
        wl = cw[lv.clamp(0, V - 1)] * in_range
        W = (wl * live).sum() if pre[s] else torch.tensor(float(n), dtype=torch.float64, device=dev)
        dW = D_PRE if pre[s] else 0
        Ws.append(W); b_Ws.append(U32 * dW * W)
        lg = c['vel'][s].double()
        mx = lg.max(1, keepdim=True).values
        ssum = torch.exp(lg - mx).sum(1, keepdim=True)
        lse = mx + torch.log(ssum)
        t_all = lse - lg                                                       # [n, V], >= 0
        e_all = K_SOFT + C_LOG * torch.log(ssum).abs() + lse.abs() + t_all.abs()
        t_i = torch.where(onehot, t_all, torch.zeros_like(t_all)).sum(1)
        e_i = torch.where(onehot, e_all, torch.zeros_like(e_all)).sum(1)
        coef = (1.0 - eps) * wl
        k_c = (1 if eps != 0.0 else 0) + (1 if (eps != 0.0 and has_w) else 0)
        k_c1 = k_c + (0 if (eps == 0.0 and not has_w) else 1)
        row = coef * t_i
        e_row = coef * e_i + k_c1 * row.abs()
        if eps != 0.0:
            S = (cw[None, :] * t_all).sum(1)
            part2 = eps / V * S
            row = row + part2
            e_row = e_row + eps / V * ((cw[None, :] * e_all).sum(1) + (12 + C_DIV) * S) + row.abs()
        if float(W) > 0.0:
            term = (row * live).sum() / W
            b_term = U32 * ((e_row * live).sum() + LOSS_D * (row.abs() * live).sum()) / W + U32 * dW * term.abs()
            wfac = wAB[s] / W * gs
            q = torch.exp(lg - mx) / ssum
            d = q - onehot.double()
            first = d * coef[:, None]
            e_g = k_q * q * coef[:, None] + (1 + k_c1) * first.abs()
            gq = first
            sumw = cw.sum()
            if eps != 0.0:
                inner = q * sumw - cw[None, :]
                E2 = eps / V * inner
                gq = first + E2
                e_g = e_g + eps / V * ((k_q + (10 if has_w else 0) + 1) * q * sumw + inner.abs()) + (C_DIV + 1) * E2.abs() + gq.abs()
            gr = gq * wfac * live[:, None]
            b_gr = (U32 * (wfac * e_g + (4 + dW) * (gq * wfac).abs()) + wfac * F32_TINY * (coef[:, None] + eps / V * sumw)) * live[:, None]
        else:                                                                  # W == 0: the deviation from torch (NaN there), exact zeros here
            term, b_term = torch.zeros((), dtype=torch.float64, device=dev), torch.zeros((), dtype=torch.float64, device=dev)
            gr, b_gr = torch.zeros_like(lg), torch.zeros_like(lg)
        ce.append(term); b_ce.append(b_term); d_vel.append(gr); b_dvel.append(b_gr)
    t = [bce[0], bce[1], bce[2], ce[0], bce[3], bce[4], bce[5], ce[1]]
    b = [b_bce[0], b_bce[1], b_bce[2], b_ce[0], b_bce[3], b_bce[4], b_bce[5], b_ce[1]]
    total = wAB[0] * sum(t[:4]) + wAB[1] * sum(t[4:])
    b_total = wAB[0] * sum(b[:4]) + wAB[1] * sum(b[4:]) + 9 * U32 * total.abs()
    return dict(out=torch.stack([total] + t + Ws).to(dev), b_out=torch.stack([b_total] + b + b_Ws).to(dev),
                d_prob=d_prob, b_dprob=b_dprob, d_vel=d_vel, b_dvel=b_dvel)


OUT_NAMES = ('total',) + E.LOSS_ORDER + ('W_A', 'W_B')


def loss_w_check(out, d_prob, d_vel, ref):
    """out[0..10] IN ORDER, then every gradient element"""
    bad = []
    for k, name in enumerate(OUT_NAMES):
        bad += violations('loss_out[%d] %s' % (k, name), out[k:k + 1], ref['out'][k:k + 1], ref['b_out'][k:k + 1])
    if d_prob is not None:
        for i in range(6):
            bad += violations('d_prob[%d]' % i, d_prob[i], ref['d_prob'][i], ref['b_dprob'][i])
    if d_vel is not None:
        for i in range(2):
            bad += violations('d_vel[%d]' % i, d_vel[i], ref['d_vel'][i], ref['b_dvel'][i])
    return bad
