"""fp32 restatements, fp64 references and rounding-model criteria of the non-MFMA kernels of csrc/ln_bwd.hip, guard.hip, loss.hip and glue.hip: LayerNorm backward, the
fused Adam step, the fused loss, the two-stage column sum and the time-embedding backward -- in the forms hftt_hip/engine.py launches.

Three things per kernel, all in torch and device-agnostic (the GPU tests evaluate the fp64 reference where the tensors live):

  *_ref    the fp64 evaluation of the same operation on the same, already rounded, inputs, plus the magnitudes the bound needs;
  *_emul   the kernel's arithmetic in fp32, in the kernel's operation order element by element.  Reductions are torch.sum in fp32 (its
           blocked tree, not the kernel's lane / wave / workgroup tree): the bound is written for the DEEPER of the two, the kernel's.
           defect=<name> selects one deliberately wrong variant (DEFECTS lists them per kernel);
  *_check  |got - ref| <= bound element by element; returns the list of violations (empty = pass).  NaN / Inf in `got` violate.

The bounds are first-order rounding models: U32 = 2^-24 per fp32 rounding (UBF = 2^-8 for a bf16-stored output) times a count read off the
kernel source times the magnitude that rounding acts on.  The device contracts a*b + c into one fma where it can; that removes roundings,
so the counts below (no contraction) hold for either code.  No criterion excludes an element: exact zeros and clamps are reproduced exactly
by a correct kernel and bounded by 0.  tests/test_elementwise_emul_bound.py shows on the CPU that every criterion passes the restatement
and fails every defect; tests/test_elementwise_fp64_gpu.py holds the kernels to them.
"""
import math

import numpy as np
import torch

import util

U32 = 2.0 ** -24          # unit roundoff of fp32 (round to nearest: half an ulp, relative)
UBF = 2.0 ** -8           # unit roundoff of bf16: 8 significand bits (7 stored), so half an ulp is 2^-8 of the value (2^-9 is half an ulp of
                          # the value's upper binade end only: a correctly rounded store of 1 + 2^-8 misses it)
F32_TINY = 2.0 ** -126    # smallest normal fp32: below it a result may be flushed or lose bits, an ABSOLUTE error of at most this
BF16 = torch.bfloat16

# device math library: the HIP math API documents logf, log1pf and expf at 1 ulp = 2 U32 (not correctly rounded).  The criteria count each
# call as 2 ulp = 4 U32: the documented ulp plus one of margin.  The restatement's own error (torch on the CPU) is measured in
# tests/test_elementwise_emul_bound.py::test_cpu_transcendentals_are_within_the_margin and recorded in that module's docstring.
C_LOG = 4.0               # logf / log1pf, in units of U32 of the result
C_EXP = 4.0               # expf, in units of U32 of the result
# sqrtf and the fp32 division: correctly rounded (1 U32) under hipcc's defaults, counted as 2 U32 each (1 ulp) should a build relax them
C_SQRT = 2.0
C_DIV = 2.0

DEFECTS = {
    'ln_bwd': ('mean_over_n_minus_1', 'ragged_last_row_drops_s2', 'clamped_row_counted', 'r_rounded_to_bf16'),
    'adam': ('eps_inside_bias_correction', 'one_minus_beta2_in_fp32', 'grad_scale_not_in_v', 'bias_correction_step_minus_1'),
    'loss': ('log1p_clamp_missing', 'ce_grad_mean_over_nV', 'terms_swapped', 'grad_scale_missing_from_d_vel'),
    'colsum': ('last_split_dropped', 'beta_on_partials'),
    'time_embed_bwd': ('accumulate_overwrites', 'scale_on_dym'),
}


def f32(x):
    """a python float rounded to fp32 (how a scalar kernel argument arrives)"""
    return float(np.float32(x))


def bf_round(t):
    return t.to(BF16).to(t.dtype)


def violations(name, got, ref, bound):
    """[(name, index of the worst element, |err|, bound there, count)] or [] -- `not (err <= bound)`, so a NaN violates"""
    got = got.detach().to(torch.float64).reshape(-1)
    ref = ref.reshape(-1); bound = bound.reshape(-1).to(ref.device)
    got = got.to(ref.device)
    err = (got - ref).abs()
    bad = ~(err <= bound)
    if not bool(bad.any()):
        return []
    ratio = torch.where(bad, torch.nan_to_num(err / (bound + 1e-300), nan=float('inf')), torch.zeros_like(err))
    i = int(ratio.argmax())
    return [(name, i, float(err[i]), float(bound[i]), int(bad.sum()))]


# ================================================================================================ LayerNorm backward
# branch table of hftt_ln_bwd (csrc/ln_bwd.hip): name -> N, storage of dy / r / dr, the dropped copy (None, 'f32', 'bf16'), operands
# offset by one element (the unaligned fallbacks), R = rows a wave takes per step (the ragged-M handling), and the M values: 1, R +- 1 and
# multiples +- 1, and one M just past the kernel's first grid pass (hftt_ln_bwd_wgs caps at 1024 workgroups of 4 waves: 4096 * R rows).
_M2 = (1, 2, 3, 7, 9, 8193)
_M4 = (1, 3, 4, 5, 15, 17, 16385)
_M1 = (1, 2, 3, 5, 4097)
LN_BRANCHES = {
    'n256_f32':          dict(N=256, dy_bf=False, r_bf=False, dr_bf=False, drop='f32', off=0, R=2, Ms=_M2),     # ln_bwd256_rows_kernel<2, true>
    'n256_x3mix':        dict(N=256, dy_bf=False, r_bf=True, dr_bf=False, drop=None, off=0, R=2, Ms=_M2),
    'n256_x3mix_drop32': dict(N=256, dy_bf=False, r_bf=True, dr_bf=False, drop='f32', off=0, R=2, Ms=_M2),
    'n256_x3mix_dropbf': dict(N=256, dy_bf=False, r_bf=True, dr_bf=False, drop='bf16', off=0, R=2, Ms=_M2),
    'n256_bf16':         dict(N=256, dy_bf=True, r_bf=True, dr_bf=True, drop='bf16', off=0, R=4, Ms=_M4),       # ln_bwd256_bf16_kernel
    'n128_f32':          dict(N=128, dy_bf=False, r_bf=False, dr_bf=False, drop='f32', off=0, R=1, Ms=_M1),     # ln_bwd_kernel<2>
    'n64_f32':           dict(N=64, dy_bf=False, r_bf=False, dr_bf=False, drop='f32', off=0, R=4, Ms=_M4),      # ln_bwd64_kernel
    'n64_bf16':          dict(N=64, dy_bf=True, r_bf=True, dr_bf=True, drop='bf16', off=0, R=4, Ms=_M4),
    'n64_unaligned':     dict(N=64, dy_bf=False, r_bf=False, dr_bf=False, drop='f32', off=1, R=1, Ms=_M1),      # ln_bwd_kernel<1>
    'n256_unaligned':    dict(N=256, dy_bf=False, r_bf=True, dr_bf=False, drop='bf16', off=1, R=1, Ms=_M1),     # ln_bwd_kernel<4>
}
LN_FAMILIES = ('row_scales', 'offset_mean', 'constant_and_zero_rows')
LN_DROP = dict(p=0.2, site=3, seed=99)


def ln_cases():
    return [(b, f, M) for b, spec in LN_BRANCHES.items() for f in LN_FAMILIES for M in spec['Ms']]


def ln_inputs(branch, family, M):
    """fp32 tensors whose values are representable in the branch's storage formats; mean / rstd are the fp32 roundings of the fp64
    statistics of the stored r (eps = 1e-5), as the forward kernels save them."""
    spec = LN_BRANCHES[branch]
    N = spec['N']
    g = torch.Generator().manual_seed(1000 * N + 10 * M + LN_FAMILIES.index(family))
    r = torch.randn(M, N, generator=g) * 2 + 0.5
    dy = torch.randn(M, N, generator=g)
    gamma = 1 + 0.2 * torch.randn(N, generator=g)
    if family == 'row_scales':                 # dy of row i at 10^(-8 i / (M - 1)): the LAST rows (the ragged ones) are the small ones
        dy = dy * (10.0 ** (-8.0 * torch.arange(M, dtype=torch.float64) / max(M - 1, 1))).float()[:, None]
    elif family == 'offset_mean':              # |mean| = 50 std: (r - mean) cancels, a bf16-stored r keeps 3 bits of the deviation
        r = 50.0 + torch.randn(M, N, generator=g)
    else:                                      # a constant row (var = 0, rstd = 1 / sqrt(eps)), LAST so that it is a ragged one, and a zero-dy row
        r[M - 1] = 3.0
        if M >= 3:
            dy[0] = 0.0
    if spec['r_bf']:
        r = bf_round(r)
    if spec['dy_bf']:
        dy = bf_round(dy)
    r64 = r.double()
    mean = r64.mean(1).float()
    rstd = (1.0 / torch.sqrt(r64.var(1, unbiased=False) + 1e-5)).float()
    return dict(dy=dy, r=r, mean=mean, rstd=rstd, gamma=gamma, M=M, N=N)


def ln_mask(M, N, p, site, seed):
    return util.keep_mask_t(seed, site, (M, N), p) if p > 0 else None


def ln_bwd_ref(c, mask=None, p=0.0):
    """fp64 LayerNorm backward from the saved fp32 statistics, on the device of c's tensors; mask: bool keep mask of the dropped copy"""
    dy, r, gam = c['dy'].double(), c['r'].double(), c['gamma'].double()
    mean, rstd = c['mean'].double()[:, None], c['rstd'].double()[:, None]
    xh = (r - mean) * rstd
    gg = dy * gam
    s1 = gg.mean(1, keepdim=True); s2 = (gg * xh).mean(1, keepdim=True)
    dr = rstd * (gg - s1 - xh * s2)
    out = dict(dr=dr, dg=(dy * xh).sum(0), db=dy.sum(0))
    # the magnitudes the roundings act on: per element of its ROW, per column
    out['dr_scale'] = rstd * (gg.abs() + gg.abs().mean(1, keepdim=True) + xh.abs() * (gg * xh).abs().mean(1, keepdim=True))
    out['dg_scale'] = (dy * xh).abs().sum(0); out['db_scale'] = dy.abs().sum(0)
    if mask is not None:
        out['drd'] = dr * mask.to(dr.device).double() * util.keep_scale(p)
    return out


def ln_bwd_emul(c, R=1, dr_bf=False, drop=None, mask=None, p=0.0, defect=None):
    """the kernels' fp32 arithmetic: xh = (r - mean) * rstd, g = dy * gamma, dr = rstd * ((g - mean g) - xh * mean(g xh)), the dropped copy
    from the UNROUNDED dr, dgamma / dbeta summed over the valid rows.  R: rows per wave step (where the ragged-M defects bite)."""
    assert defect is None or defect in DEFECTS['ln_bwd']
    dy, r, gam, mean, rstd = c['dy'], c['r'], c['gamma'], c['mean'][:, None], c['rstd'][:, None]
    M, N = dy.shape
    if defect == 'r_rounded_to_bf16':
        r = bf_round(r)
    xh = (r - mean) * rstd
    gg = dy * gam
    s1 = gg.sum(1, keepdim=True) * f32(1.0 / (N - 1 if defect == 'mean_over_n_minus_1' else N))
    s2 = (gg * xh).sum(1, keepdim=True) * f32(1.0 / N)
    o = rstd * (gg - s1 - xh * s2)
    ragged = M % R != 0
    if defect == 'ragged_last_row_drops_s2' and ragged:
        o[M - 1] = (rstd * (gg - s1))[M - 1]
    dg = (dy * xh).sum(0); db = dy.sum(0)
    if defect == 'clamped_row_counted' and ragged:            # the R - M % R invalid rows of the last step load row M - 1 (clamped)
        k = float(R - M % R)
        dg = dg + k * (dy * xh)[M - 1]; db = db + k * dy[M - 1]
    out = dict(dr=bf_round(o) if dr_bf else o, dg=dg, db=db)
    if drop is not None and mask is not None:
        od = torch.where(mask, o * f32(util.keep_scale(p)), torch.zeros_like(o))
        out['drd'] = bf_round(od) if drop == 'bf16' else od
    return out


# dr, per element, against S = rstd (|g_e| + mean|g| + |xh_e| mean|g xh|) of its row.  D = depth of the row sums s1, s2 in the deepest
# kernel (ln_bwd256_bf16_kernel: 16 elements per lane in sequence + 4 lane levels = 20; rows<2>: 8 + 5; ln_bwd_kernel<4>: 4 + 6).
#   on |g_e|:               g = dy * gamma 1, (g - s1) 1, (.. - xh s2) 1, rstd * .. 1                                   =  4
#   on mean|g|:             s1's sum D + 1 (its terms g), (g - s1) 1, (.. - xh s2) 1, rstd * .. 1                       =  D + 4
#   on |xh_e| mean|g xh|:   s2's sum D + 4 (terms g * xh: g 1, xh = (r - mean) * rstd 2, product 1), xh_e 2, xh_e * s2 1,
#                           (.. - xh s2) 1, rstd * .. 1                                                                  =  D + 9
# the largest coefficient bounds all three: K_DR = D + 9 = 29.
LN_D_ROW = 20
K_DR = LN_D_ROW + 9
# dgamma / dbeta, per column, against sum_rows |dy xh| resp. sum_rows |dy|.  Depth of the column sum for M <= 16385 (the tables above):
# 2 steps of a lane (M just past one grid pass) + 16 partials of a workgroup in sequence (4 R <= 16) + hftt_ln_bwd_reduce: chains of
# ceil(1024 / 128) = 8, a tail of <= 7 on chain 0, 3 tree levels, 16 in sequence = 52.  Terms: dy * xh carries xh 2 + product 1.
LN_D_COL = 2 + 16 + 8 + 7 + 3 + 16
K_DG = LN_D_COL + 3
K_DB = LN_D_COL


def ln_bwd_check(got, ref, dr_bf=False, drop=None, mask=None, p=0.0):
    bad = []
    b = K_DR * U32 * ref['dr_scale']
    bad += violations('dr', got['dr'], ref['dr'], b * (1 + UBF) + UBF * ref['dr'].abs() if dr_bf else b)        # + one bf16 rounding of the result
    bad += violations('dgamma', got['dg'], ref['dg'], K_DG * U32 * ref['dg_scale'])
    bad += violations('dbeta', got['db'], ref['db'], K_DB * U32 * ref['db_scale'])
    if drop is not None and mask is not None:
        m = mask.to(ref['dr'].device)
        bd = (b * util.keep_scale(p) + U32 * ref['drd'].abs()) * m.double()                                       # dr * (256 / thr): one more rounding
        bad += violations('dr_drop', got['drd'], ref['drd'], bd * (1 + UBF) + UBF * ref['drd'].abs() if drop == 'bf16' else bd)
        dropped_nonzero = int(((got['drd'].to(m.device) != 0) & ~m).sum())
        if dropped_nonzero:
            bad.append(('dr_drop: non-zero where the mask is 0', -1, float('nan'), 0.0, dropped_nonzero))
    return bad


def ln_old_passes(got, ref, dr_bf=False, drop=None):
    """the first-generation assertion (tests/test_kernels_gpu.py): max |a - b| / max |b| over the tensor, 1e-5 (6e-3 for bf16 storage)"""
    ok = util.rel_err(got['dr'], ref['dr']) < (6e-3 if dr_bf else 1e-5)
    ok = ok and util.rel_err(got['dg'], ref['dg']) < 2e-5 and util.rel_err(got['db'], ref['db']) < 2e-5
    if 'drd' in got and 'drd' in ref:
        ok = ok and util.rel_err(got['drd'], ref['drd']) < (6e-3 if drop == 'bf16' else 1e-5)
    return bool(ok)


# hftt_ln_bwd_reduce on its own: out[c] = beta * out[c] + sum_w ws[w][c].  Depth: chains of ceil(n_wg / 128) <= 8 and a tail of <= 7 on
# chain 0, 3 tree levels, 16 in sequence = 34; then beta * out + s: 2 roundings on the result.
LN_RED_N_WG = (1, 15, 16, 17, 127, 128, 129, 1024)
K_RED = 8 + 7 + 3 + 16


def ln_reduce_bound(ws64, dst64, beta):
    s = ws64.sum(0)
    ref = beta * dst64 + s
    return ref, U32 * (K_RED * ws64.abs().sum(0) + 2 * ((beta * dst64).abs() + s.abs()))


# ================================================================================================ Adam
ADAM_N = (1, 2, 3, 5, 1027, 2097152 + 6)          # n < 4, n % 4 in {1, 2, 3}, and past one grid pass (2048 * 256 * 4 elements)
ADAM_GRAD_SCALE = (1.0, 0.5, 1.0 / 3.0)
ADAM_EPS = (1e-8, 1e-6)
ADAM_START = (1, 1000)
ADAM_STEPS = 20
ADAM_LR, ADAM_B1, ADAM_B2 = 1e-3, 0.9, 0.999


def adam_cases():
    small = [(n, gs, eps, s0) for n in ADAM_N[:-1] for gs in ADAM_GRAD_SCALE for eps in ADAM_EPS for s0 in ADAM_START]
    big = [(ADAM_N[-1], 1.0 / 3.0, 1e-8, 1), (ADAM_N[-1], 0.5, 1e-6, 1000)]
    return small + big


def _log_uniform(n, lo, hi, g):
    mag = 10.0 ** (lo + (hi - lo) * torch.rand(n, generator=g, dtype=torch.float64))
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0).double()
    return (mag * sign).float()


def adam_idle(n):
    """the elements that carry g = 0 and zero state throughout: their p must not change by a bit"""
    return torch.arange(n) % 7 == 3


def adam_state(n, seed):
    """p: a third exact zeros (there p = -update exactly: the update is seen in ITS ulps), a third log-uniform, a third N(0, 1);
    m, v non-zero: the moments of an earlier gradient stream of the same kind"""
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g)
    k = torch.arange(n) % 3
    p = torch.where(k == 0, torch.zeros(n), torch.where(k == 1, _log_uniform(n, -8, 0, g), p))
    m = 0.3 * _log_uniform(n, -12, -1, g)
    v = (_log_uniform(n, -12, -1, g) ** 2) * 0.5
    idle = adam_idle(n)
    m[idle] = 0.0; v[idle] = 0.0
    return p, m, v


def adam_grad(n, seed, step):
    """log-uniform in magnitude over 1e-12 .. 1e-1, random sign, exact zeros (the idle elements, and one in 16 of the others)"""
    g = torch.Generator().manual_seed(seed * 7919 + step)
    gr = _log_uniform(n, -12, -1, g)
    gr[torch.rand(n, generator=g) < 1.0 / 16] = 0.0
    gr[adam_idle(n)] = 0.0
    return gr


def adam_emul(p, g, m, v, step, lr=ADAM_LR, beta1=ADAM_B1, beta2=ADAM_B2, eps=1e-8, grad_scale=1.0, defect=None):
    """hftt_adam_step + adam_kernel: the host forms 1 - beta and the bias corrections in double and rounds once; the kernel is fp32"""
    assert defect is None or defect in DEFECTS['adam']
    s = step - 1 if defect == 'bias_correction_step_minus_1' else step
    bc1 = 1.0 - beta1 ** s; bc2 = 1.0 - beta2 ** s
    lr_c = f32(lr / bc1) if bc1 != 0 else float('inf')
    isb2 = f32(1.0 / math.sqrt(bc2)) if bc2 != 0 else float('inf')
    omb1 = f32(1.0 - beta1)
    omb2 = f32(1.0 - beta2) if defect != 'one_minus_beta2_in_fp32' else float(np.float32(1.0) - np.float32(beta2))
    gr = g * f32(grad_scale)
    m = f32(beta1) * m + omb1 * gr
    gv = g if defect == 'grad_scale_not_in_v' else gr
    v = f32(beta2) * v + omb2 * gv * gv
    if defect == 'eps_inside_bias_correction':
        den = (v.sqrt() + f32(eps)) * isb2
    else:
        den = v.sqrt() * isb2 + f32(eps)
    return p - lr_c * m / den, m, v


def adam_ref(p, g, m, v, step, lr=ADAM_LR, beta1=ADAM_B1, beta2=ADAM_B2, eps=1e-8, grad_scale=1.0):
    """one fp64 Adam step (torch.optim.Adam's definition) from the given fp32 state, with the bounds of m, v and p.  In U32:
      gr = g * gs:                          gs's rounding 1 + product 1                                                  = 2
      m = b1 m0 + (1 - b1) gr:              on |b1 m0|: b1 1, product 1, sum 1 = 3;  on |(1 - b1) gr|: (1 - b1) 1, gr 2, product 1, sum 1 = 5
                                            (the two terms may cancel, so the bound stands on the terms: it is ulps of m when they do not)
      v = b2 v0 + (1 - b2) gr gr:           on b2 v0: 3;  on (1 - b2) gr^2: (1 - b2) 1, gr 2 + 2, two products 2, sum 1 = 8   (no cancellation: <= 8 ulps of v)
      den = sqrt(v) / sqrt(bc2) + eps:      sqrt of v: 8 / 2 + C_SQRT, 1 / sqrt(bc2) 1, product 1, eps 1, sum 1          = 8 + C_SQRT  (all terms positive)
      update = (lr / bc1) m / den:          lr / bc1 1, product 1, den, division C_DIV: (10 + C_SQRT + C_DIV) |update| + (lr / bc1) B_m / den
      p = p0 - update:                      one rounding of p + the update's bound."""
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    bc1 = 1.0 - beta1 ** step; bc2 = 1.0 - beta2 ** step
    gr = g * grad_scale
    t1, t2 = beta1 * m, (1.0 - beta1) * gr
    m1 = t1 + t2
    b_m = U32 * (3 * t1.abs() + 5 * t2.abs())
    v1 = beta2 * v + (1.0 - beta2) * gr * gr
    b_v = U32 * (3 * beta2 * v + 8 * (1.0 - beta2) * gr * gr)
    den = v1.sqrt() / math.sqrt(bc2) + eps
    upd = (lr / bc1) * m1 / den
    b_u = U32 * (10 + C_SQRT + C_DIV) * upd.abs() + (lr / bc1) * b_m / den
    p1 = p - upd
    return dict(p=p1, m=m1, v=v1, b_p=U32 * p1.abs() + b_u, b_m=b_m, b_v=b_v)


def adam_check(got_p, got_m, got_v, ref):
    return (violations('p', got_p, ref['p'], ref['b_p']) + violations('m', got_m, ref['m'], ref['b_m'])
            + violations('v', got_v, ref['v'], ref['b_v']))


# ================================================================================================ loss
# (kernel, V, n, grad_scale): n chosen for n_wg = ceil(n / 8) (loss_v4_kernel: aligned, V % 4 == 0, V <= 128) resp. ceil(n / 4) (the general
# kernel: V = 128 through views offset by one element, V > 128) in {1, 31, 33, 97, 129, 4096}, and one n past each kernel's first grid pass
LOSS_CASES = (
    [('v4', 128, n, gs) for n, gs in ((8, 1.0), (248, 0.25), (261, 1.0), (775, 0.25), (1027, 1.0), (32768, 0.25), (32768 + 9, 1.0))]
    + [('v4', 4, 5, 0.25), ('v4', 4, 261, 1.0)]
    + [('general_unaligned', 128, n, gs) for n, gs in ((3, 0.25), (123, 1.0), (130, 0.25), (387, 1.0), (514, 0.25), (16384, 1.0), (16384 + 5, 0.25))]
    + [('general', V, n, gs) for V in (129, 255, 256) for n, gs in ((3, 1.0), (130, 0.25), (514, 1.0))]
)
LOSS_W = (f32(0.7), f32(1.3))
# loss_out[1..8] (include/hftt_hip.h, loss_reduce_kernel): the order the trainer and the logs read
LOSS_ORDER = ('onset_A', 'offset_A', 'mpe_A', 'velocity_A', 'onset_B', 'offset_B', 'mpe_B', 'velocity_B')


def loss_inputs(V, n, seed=0):
    """posteriors with saturated entries (exactly 0 and 1 against both kinds of target), velocity logits N(0, 9) with one row of +-80"""
    g = torch.Generator().manual_seed(100000 * seed + 1000 * V + n % 997)
    probs = [torch.rand(n, generator=g) for _ in range(6)]
    k = min(4, n)
    for q in probs:
        q[:k] = torch.tensor([0.0, 1.0, 0.0, 1.0])[:k]
    vel = [torch.randn(n, V, generator=g) * 3 for _ in range(2)]
    for t in vel:
        t[n // 2] = torch.where(torch.arange(V) % 2 == 0, 80.0, -80.0)
    lo, lf = torch.rand(n, generator=g), torch.rand(n, generator=g)
    lo[:k] = torch.tensor([0.0, 1.0, 1.0, 0.0])[:k]; lf[:k] = torch.tensor([1.0, 0.0, 0.0, 1.0])[:k]
    lm = (torch.rand(n, generator=g) < 0.3).float()
    lv = torch.randint(0, V, (n,), generator=g)
    return dict(probs=probs, vel=vel, lo=lo, lf=lf, lm=lm, lv=lv, n=n, V=V)


def _bce_labels(c, i):
    return (c['lo'], c['lf'], c['lm'])[i % 3]


def loss_emul(c, grad_scale=1.0, defect=None):
    """loss_kernel / loss_v4_kernel + loss_reduce_kernel in fp32 (the two kernels share every formula).  Returns out[9], d_prob[6], d_vel[2]."""
    assert defect is None or defect in DEFECTS['loss']
    n, V = c['n'], c['V']
    inv_n = f32(1.0 / np.float32(n))
    gs = f32(grad_scale)
    bce, d_prob, ce, d_vel = [], [], [], []
    for i in range(6):
        p, y = c['probs'][i], _bce_labels(c, i)
        lp = torch.log(p).clamp_min(-100.0)
        l1p = torch.log1p(-p)
        if defect != 'log1p_clamp_missing':
            l1p = l1p.clamp_min(-100.0)
        bce.append((-(y * lp + (1.0 - y) * l1p)).sum() / n)
        w = LOSS_W[0] if i < 3 else LOSS_W[1]
        d_prob.append((p - y) / ((1.0 - p) * p).clamp_min(f32(1e-12)) * f32(np.float32(w) * np.float32(inv_n) * np.float32(gs)))
    onehot = torch.nn.functional.one_hot(c['lv'], V).bool()
    for side in range(2):
        lg = c['vel'][side]
        mx = lg.max(1, keepdim=True).values
        ex = torch.exp(lg - mx)
        s = ex.sum(1, keepdim=True)
        lse = mx + torch.log(s)
        ce.append((lse[:, 0] - lg[onehot]).sum() / n)
        w = float(np.float32(LOSS_W[side]) * np.float32(inv_n))
        if defect == 'ce_grad_mean_over_nV':
            w = float(np.float32(w) / np.float32(V))
        if defect != 'grad_scale_missing_from_d_vel':
            w = float(np.float32(w) * np.float32(gs))
        d_vel.append((ex * (1.0 / s) - onehot.float()) * w)
    t = [bce[0], bce[1], bce[2], ce[0], bce[3], bce[4], bce[5], ce[1]]
    la = ((t[0] + t[1]) + t[2]) + t[3]; lb = ((t[4] + t[5]) + t[6]) + t[7]
    if defect == 'terms_swapped':
        t[3], t[4] = t[4], t[3]                          # velocity_A <-> onset_B in loss_out[1..8]; the total is formed before
    out = torch.stack([LOSS_W[0] * la + LOSS_W[1] * lb] + t)
    return out, d_prob, d_vel


# depth of a term's sum over n in the kernels, for n <= 32768 + 9: 2 steps of a wave + 1 (the two halves) + 3 (four waves) + loss_reduce:
# chains of 4096 / 128 = 32, a tail of <= 3, 2 tree levels, 32 in sequence, and the division by n
LOSS_D = 2 + 1 + 3 + 32 + 3 + 2 + 32 + 1
# softmax denominator s = sum exp(v - mx) >= 1, relative: depth 10 (general kernel: 4 in sequence + 6 lane levels) + expf C_EXP + the rounding
# of v - mx, which moves exp(-t) by t U32 exp(-t) <= U32 / e.
K_SOFT = 10 + C_EXP + 1


def loss_ref(c, grad_scale=1.0):
    """fp64 evaluation (the kernels' clamps included) and the bounds of out[9], d_prob, d_vel.
      BCE term of an element, -(y lp + (1 - y) l1p), both parts <= 0 (no cancellation): log C_LOG, (1 - y) 1, product 1, sum 1: (3 + C_LOG) |term_i|;
      CE term, (mx + log s) - picked: on log s: s's K_SOFT (absolute, d log s = ds / s) + C_LOG |log s|; |lse| for the sum; |term_i| for the difference
        (the difference cancels when the label's logit dominates: the bound stands on |lse|, not on the term);
      a term's mean: + LOSS_D sum|term_i| / n.   total: weights exact (fp32 inputs), 2 products + 7 sums on positive terms: + 9 |total|.
      d_prob, relative: (p - y) 1, (1 - p) p 2, division C_DIV, w / n * gs 3, product 1 = 7 + C_DIV.
      d_vel, per element: softmax_c = ex / s: expf C_EXP + 1, s K_SOFT, 1 / s C_DIV, product 1 on softmax_c; the subtraction and the product with
        w: 2 + 3 (w / n * gs) on |softmax_c - onehot|; exp(v - mx) below F32_TINY underflows (logits of +-80): + w F32_TINY, absolute."""
    n, V = c['n'], c['V']
    dev = c['vel'][0].device
    wA, wB = LOSS_W
    bce, b_bce, d_prob, b_dprob = [], [], [], []
    for i in range(6):
        p, y = c['probs'][i].double(), _bce_labels(c, i).double()
        ti = -(y * torch.log(p).clamp_min(-100.0) + (1.0 - y) * torch.log1p(-p).clamp_min(-100.0))
        bce.append(ti.sum() / n)
        b_bce.append(U32 * (3 + C_LOG + LOSS_D) * ti.abs().sum() / n)
        w = (wA if i < 3 else wB) / n * grad_scale
        gr = (p - y) / ((1.0 - p) * p).clamp_min(f32(1e-12)) * w
        d_prob.append(gr); b_dprob.append(U32 * (7 + C_DIV) * gr.abs())
    onehot = torch.nn.functional.one_hot(c['lv'], V).bool()
    ce, b_ce, d_vel, b_dvel = [], [], [], []
    for side in range(2):
        lg = c['vel'][side].double()
        mx = lg.max(1, keepdim=True).values
        s = torch.exp(lg - mx).sum(1, keepdim=True)
        lse = (mx + torch.log(s))[:, 0]
        ti = lse - lg[onehot]
        ce.append(ti.sum() / n)
        per = K_SOFT + C_LOG * torch.log(s)[:, 0].abs() + lse.abs() + ti.abs()
        b_ce.append(U32 * (per.sum() + LOSS_D * ti.abs().sum()) / n)
        w = (wA, wB)[side] / n * grad_scale
        soft = torch.exp(lg - mx) / s
        d = soft - onehot.double()
        d_vel.append(d * w)
        b_dvel.append(U32 * w * ((C_EXP + 1 + K_SOFT + C_DIV + 1) * soft + 5 * d.abs()) + w * F32_TINY)
    t = [bce[0], bce[1], bce[2], ce[0], bce[3], bce[4], bce[5], ce[1]]
    b = [b_bce[0], b_bce[1], b_bce[2], b_ce[0], b_bce[3], b_bce[4], b_bce[5], b_ce[1]]
    total = wA * sum(t[:4]) + wB * sum(t[4:])
    b_total = wA * sum(b[:4]) + wB * sum(b[4:]) + 9 * U32 * total.abs()
    return dict(out=torch.stack([total] + t).to(dev), b_out=torch.stack([b_total] + b).to(dev),
                d_prob=d_prob, b_dprob=b_dprob, d_vel=d_vel, b_dvel=b_dvel)


def loss_check(out, d_prob, d_vel, ref):
    """out[0..8] IN ORDER (LOSS_ORDER), then every gradient element"""
    bad = []
    for k, name in enumerate(('total',) + LOSS_ORDER):
        bad += violations('loss_out[%d] %s' % (k, name), out[k:k + 1], ref['out'][k:k + 1], ref['b_out'][k:k + 1])
    if d_prob is not None:
        for i in range(6):
            bad += violations('d_prob[%d]' % i, d_prob[i], ref['d_prob'][i], ref['b_dprob'][i])
    if d_vel is not None:
        for i in range(2):
            bad += violations('d_vel[%d]' % i, d_vel[i], ref['d_vel'][i], ref['b_dvel'][i])
    return bad


def loss_old_passes(out, d_prob, d_vel, ref):
    """the first-generation assertion (tests/test_small_kernels_gpu.py): total 2e-5 relative, the eight terms SORTED, d_prob 2e-5 relative
    + 1e-9, d_vel 2e-5 of the tensor maximum"""
    got = out.double().cpu(); r = ref['out'].cpu()
    ok = bool(abs(got[0] - r[0]) < 2e-5 * abs(r[0]))
    ok = ok and bool(np.allclose(sorted(got[1:9].tolist()), sorted(r[1:9].tolist()), rtol=2e-5, atol=1e-6))
    for i in range(6):
        ok = ok and bool(((d_prob[i].double().cpu() - ref['d_prob'][i].cpu()).abs() <= 2e-5 * ref['d_prob'][i].cpu().abs() + 1e-9).all())
    for i in range(2):
        ok = ok and util.rel_err(d_vel[i], ref['d_vel'][i]) < 2e-5
    return ok


# ================================================================================================ column sum
# (rows, n, ld - n, bf16 input, beta): rows below / at / above the 16 splits and the engine's B N = 704; n below one block, one block, ragged,
# and the engine's T d = 32768
COLSUM_CASES = (
    (1, 100, 0, False, 0.0), (15, 256, 8, False, 1.0), (16, 3000, 0, True, 0.0), (17, 100, 8, True, 1.0), (17, 3000, 8, False, 0.0),
    (704, 256, 0, True, 1.0), (704, 32768, 0, True, 1.0), (704, 3000, 8, False, 1.0), (15, 32768, 8, True, 0.0), (1, 256, 8, False, 1.0),
)
CS_SPLITS = 16


def colsum_inputs(rows, n, pad, bf, seed=0):
    """gradient-like columns: scales log-uniform over 1e-6 .. 1; every fourth column cancels to about 1e-6 of its sum |x| (rows >= 2);
    x lives in a [rows, n + pad] buffer (ld > n) whose padding is NaN; out0 is the non-zero destination"""
    g = torch.Generator().manual_seed(31 * rows + n + pad + seed)
    x = torch.randn(rows, n, generator=g) * _log_uniform(n, -6, 0, g).abs()[None]
    if rows >= 2:
        cc = torch.arange(n) % 4 == 1
        col = x[:, cc].double()
        col[-1] = -col[:-1].sum(0) * (1.0 - 1e-6)
        x[:, cc] = col.float()
    if bf:
        x = bf_round(x)
    buf = torch.full((rows, n + pad), float('nan'))
    buf[:, :n] = x
    out0 = torch.randn(n, generator=g) * x.abs().sum(0)
    return dict(buf=buf, x=buf[:, :n], out0=out0, rows=rows, n=n)


def colsum_emul(c, beta=0.0, defect=None):
    """colsum_stage1_kernel (16 splits of ceil(rows / 16) rows) + colsum_stage2_kernel (the 16 partials in sequence, then beta * out + acc)"""
    assert defect is None or defect in DEFECTS['colsum']
    x, rows = c['x'], c['rows']
    per = (rows + CS_SPLITS - 1) // CS_SPLITS
    last = (rows - 1) // per
    acc = torch.zeros(c['n'])
    for sp in range(CS_SPLITS):
        r0, r1 = sp * per, min(sp * per + per, rows)
        part = x[r0:r1].sum(0) if r1 > r0 else torch.zeros(c['n'])
        if defect == 'last_split_dropped' and rows % CS_SPLITS != 0 and sp == last:
            part = torch.zeros(c['n'])
        if defect == 'beta_on_partials':
            part = part * f32(beta)
        acc = acc + part
    if defect == 'beta_on_partials':
        return c['out0'] + acc
    return c['out0'] * f32(beta) + acc if beta != 0.0 else acc


def colsum_ref(c, beta=0.0):
    """per column against sum|x|: depth ceil(rows / 16) (a split, in sequence) + 16 (the partials, in sequence); beta * out + acc: 2 roundings"""
    x = c['x'].double(); out0 = c['out0'].double()
    s = x.sum(0)
    ref = beta * out0 + s
    depth = (c['rows'] + CS_SPLITS - 1) // CS_SPLITS + CS_SPLITS
    return ref, U32 * (depth * x.abs().sum(0) + 2 * ((beta * out0).abs() + s.abs()))


def colsum_old_passes(got, ref):
    return util.max_err(got, ref) < 1e-3              # tests/test_kernels_gpu.py::test_colsum_and_adam, doubled after beta = 1 there


# ================================================================================================ time embedding
TE_SHAPES = ((2, 16, 11, 64), (1, 128, 88, 256))          # (B, T, N, d): the second is the model's own T and N
TE_CASES = [(s, half, p, dym) for s in TE_SHAPES for half in (False, True) for p in (0.0, 0.25) for dym in (True, False)]
TE_DROP = dict(site=9, seed=4321)


def te_inputs(shape, half, seed=0):
    B, T, N, d = shape
    g = torch.Generator().manual_seed(d + T + seed + half)
    dy = torch.randn(B * N, T, d, generator=g) * _log_uniform(B * N, -6, 0, g).abs()[:, None, None]
    dx0 = torch.randn(B * T, N, d, generator=g) * 0.01
    if half:
        dy, dx0 = bf_round(dy), bf_round(dx0)
    return dict(dy=dy, dx0=dx0, shape=shape, scale=math.sqrt(d))


def _te_to_input_rows(t, shape):
    B, T, N, d = shape
    return t.view(B, N, T, d).permute(0, 2, 1, 3).reshape(B * T, N, d)


def te_bwd_emul(c, mask=None, p=0.0, half=False, defect=None):
    """time_embed_bwd_kernel with accumulate = 1: v = keep ? dy * (256 / thr) : 0; dym = v; dx += v * scale (rows (b, n, t) -> (b, t, n))"""
    assert defect is None or defect in DEFECTS['time_embed_bwd']
    v = c['dy']
    if mask is not None:
        v = torch.where(mask, v * f32(util.keep_scale(p)), torch.zeros_like(v))
    sc = f32(c['scale'])
    dym = v * sc if defect == 'scale_on_dym' else v
    o = _te_to_input_rows(v * sc, c['shape'])
    if defect != 'accumulate_overwrites':
        o = o + c['dx0']
    return (bf_round(o), bf_round(dym)) if half else (o, dym)


def te_bwd_ref(c, mask=None, p=0.0, half=False):
    """dym: the keep scale's product, 1 rounding; dx = old + v * scale: that one, the product, the sum: 3 on (|v scale| + |old|); + a bf16
    rounding of each stored result when the stream is bf16"""
    v = c['dy'].double()
    if mask is not None:
        v = v * mask.to(v.device).double() * util.keep_scale(p)
    add = _te_to_input_rows(v * f32(c['scale']), c['shape'])
    dx = add + c['dx0'].double()
    b_dym = U32 * v.abs(); b_dx = 3 * U32 * (add.abs() + c['dx0'].double().abs())
    if half:
        b_dym = b_dym * (1 + UBF) + UBF * v.abs(); b_dx = b_dx * (1 + UBF) + UBF * dx.abs()
    return dict(dx=dx, dym=v, b_dx=b_dx, b_dym=b_dym)


def te_bwd_check(dx, dym, ref):
    bad = violations('dx', dx, ref['dx'], ref['b_dx'])
    if dym is not None:
        bad += violations('dym', dym, ref['dym'], ref['b_dym'])
    return bad


def te_old_passes(dx, dym, ref, half):
    tol = 6e-3 if half else 2e-6
    return util.rel_err(dx, ref['dx']) < tol and (dym is None or util.rel_err(dym, ref['dym']) < tol)
