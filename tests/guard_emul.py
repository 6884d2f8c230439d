"""fp64 references, restatements and rounding-model criteria of the guarded optimizer step (csrc/guard.hip): hftt_grad_norm (the global L2
norm of the flat gradient, its clip factor and the apply / skip verdict) and hftt_adam_step_guarded (adam_kernel's update behind that verdict,
with the clip factor and decoupled weight decay).  Same three things per kernel as tests/elementwise_emul.py, in torch and device-agnostic:

  *_ref    fp64 evaluation on the same fp32 inputs, with the bounds;
  *_emul   the kernel's arithmetic restated (the norm in fp64 as the kernel sums it, the update in fp32 in the kernel's operation order);
           defect=<name> selects one deliberately wrong variant (DEFECTS);
  *_check  the list of violations (empty = pass).

tests/test_guard_emul_bound.py shows on the CPU that every criterion passes the restatement and fails every defect, and records which input
family sees which defect; tests/test_guard_gpu.py holds the kernels to the criteria.
"""
import functools
import math

import numpy as np
import torch

import elementwise_emul as E
from elementwise_emul import U32, C_SQRT, C_DIV, f32, violations

F32_MAX = float(np.finfo(np.float32).max)

DEFECTS = {
    'gnorm': ('squares_summed_in_fp32', 'tail_dropped', 'norm_of_unscaled_gradient', 'clip_eps_missing'),
    'adam': ('clip_not_in_v', 'skip_still_updates_v', 'decay_after_update', 'decay_coupled_into_gradient'),
}

# both new kernels run min(ceil((n / 4 + 1) / 256), 2048) workgroups of 256 lanes, four elements per lane and pass: the first grid pass ends
# at 2048 * 256 * 4 elements.  The last n lies one quad and one tail element behind it (n % 4 == 1).
GRID_PASS = 2048 * 256 * 4
GUARD_N = (1, 3, 4, 5, 1023, 1025, GRID_PASS + 5)
GRAD_SCALES = (1.0, 0.25)
MAX_NORMS = (math.inf, 1e-3, 1.0)
WEIGHT_DECAYS = (0.0, 0.01)
FINITE_FAMILIES = ('log_uniform', 'zeros', 'huge', 'tiny')
PLANT_VALUES = {'+inf': math.inf, '-inf': -math.inf, 'nan': math.nan}
PLANT_POSITIONS = ('first', 'tail', 'last_quad')
PLANTED_FAMILIES = tuple('%s@%s' % (v, p) for v in PLANT_VALUES for p in PLANT_POSITIONS)
FAMILIES = FINITE_FAMILIES + PLANTED_FAMILIES


def plant_index(n, pos):
    """element 0; the last element (the last tail element when n % 4 != 0); the last element of the last full quad (None when n < 4)"""
    if pos == 'first':
        return 0
    if pos == 'tail':
        return n - 1
    return 4 * (n // 4) - 1 if n >= 4 else None


@functools.lru_cache(maxsize=None)
def _log_uniform_grad(n, seed):
    return E.adam_grad(n, seed + n % 1000, 0)          # computed once per (n, seed); callers get clones


def guard_grad(n, family, seed=0):
    """the flat gradient of one case, fp32 on the CPU (None: the family does not exist at this n).  log_uniform is adam_grad's stream
    (1e-12 .. 1e-1 in magnitude, random sign, exact zeros); huge / tiny are +-1e30 / +-1e-30 everywhere: their squares leave fp32 on either
    side; a planted family is log_uniform with one element replaced"""
    if family == 'log_uniform':
        return _log_uniform_grad(n, seed).clone()
    if family == 'zeros':
        return torch.zeros(n)
    if family in ('huge', 'tiny'):
        sign = torch.where(torch.arange(n) % 3 == 1, -1.0, 1.0)
        return sign * (1e30 if family == 'huge' else 1e-30)
    value, pos = family.split('@')
    i = plant_index(n, pos)
    if i is None:
        return None
    g = _log_uniform_grad(n, seed).clone()
    g[i] = PLANT_VALUES[value]
    return g


# ================================================================================================ the norm
def gnorm_ref(g, grad_scale=1.0, max_norm=math.inf):
    """fp64: norm = |grad_scale| sqrt(sum g^2), apply = isfinite(norm), coef = min(1, max_norm / (norm + 1e-6)) (0 when skipped).  The kernel
    forms both in fp64 (products of fp32 values are exact there, and the sum of n <= 2^22 non-negative terms is good to n 2^-53 << U32) and
    rounds each ONCE to fp32: the bound is 2 U32 relative -- that rounding, plus one unit of margin for the fp64 sum and the square root.
    `clipped` is the expected increment of the counter: 1 / 0, or None where coef is within the bound of 1 (either is right)."""
    g64 = g.double()
    norm = abs(grad_scale) * math.sqrt(float((g64 * g64).sum()))
    apply = math.isfinite(norm)
    coef = min(1.0, max_norm / (norm + 1e-6)) if apply else 0.0
    raw = max_norm / (norm + 1e-6) if apply else 0.0
    clipped = 0 if not apply or raw >= 1.0 + 2 * U32 else (1 if raw < 1.0 - 2 * U32 else None)
    return dict(norm=norm, coef=coef, apply=int(apply), skipped=int(not apply), clipped=clipped, b_norm=2 * U32 * norm if apply else 0.0, b_coef=2 * U32 * coef)


def gnorm_emul(g, grad_scale=1.0, max_norm=math.inf, defect=None):
    """grad_sqsum_kernel + grad_norm_finalize_kernel: squares and their sum in fp64, norm64 and coef formed in double, each rounded once.
    Returns what the record holds: (norm fp32, coef fp32, apply)."""
    assert defect is None or defect in DEFECTS['gnorm']
    n = g.numel()
    if defect == 'tail_dropped':
        g = g[:4 * (n // 4)]
    if defect == 'squares_summed_in_fp32':
        s = float((g * g).sum())
    else:
        g64 = g.double()
        s = float((g64 * g64).sum())
    scale = 1.0 if defect == 'norm_of_unscaled_gradient' else abs(grad_scale)
    norm = scale * math.sqrt(s) if s == s else math.nan
    apply = math.isfinite(norm)
    coef = 0.0
    if apply:
        den = norm + (0.0 if defect == 'clip_eps_missing' else 1e-6)
        coef = min(1.0, max_norm / den) if den > 0.0 else 1.0          # (x / 0 is +inf in the kernel's arithmetic)
    with np.errstate(over='ignore'):
        return float(np.float32(norm)), float(np.float32(coef)), int(apply)


def gnorm_check(norm, coef, apply, ref):
    """norm, coef (python floats read from the record), apply against gnorm_ref"""
    bad = []
    if apply != ref['apply']:
        bad.append(('apply', 0, float(apply), float(ref['apply']), 1))
    if not ref['apply']:
        if math.isfinite(norm):
            bad.append(('norm of a skipped step is finite', 0, norm, math.inf, 1))
        if coef != 0.0:
            bad.append(('coef of a skipped step', 0, coef, 0.0, 1))
        return bad
    if ref['norm'] > F32_MAX:                   # finite in fp64, beyond fp32: the record holds +inf and the step is applied
        if norm != math.inf:
            bad.append(('norm beyond fp32', 0, norm, math.inf, 1))
    elif not abs(norm - ref['norm']) <= ref['b_norm']:
        bad.append(('norm', 0, abs(norm - ref['norm']), ref['b_norm'], 1))
    if not abs(coef - ref['coef']) <= ref['b_coef'] or coef > 1.0:
        bad.append(('coef', 0, abs(coef - ref['coef']), ref['b_coef'], 1))
    if max(ref['coef'], 0.0) == 1.0 and ref['clipped'] == 0 and coef != 1.0:
        bad.append(('coef must be exactly 1 when nothing is clipped', 0, coef, 1.0, 1))
    return bad


def counters_check(d_skipped, d_clipped, coef, ref):
    """increments of the two cumulative counters over one call; `coef` as read back (it decides where the reference is within its bound of 1)"""
    bad = []
    if d_skipped != ref['skipped']:
        bad.append(('skipped', 0, float(d_skipped), float(ref['skipped']), 1))
    want = ref['clipped'] if ref['clipped'] is not None else int(coef < 1.0)
    if d_clipped != want:
        bad.append(('clipped', 0, float(d_clipped), float(want), 1))
    return bad


# ================================================================================================ the guarded Adam step
def guarded_adam_ref(p, g, m, v, step, coef, lr=E.ADAM_LR, beta1=E.ADAM_B1, beta2=E.ADAM_B2, eps=1e-8, grad_scale=1.0, weight_decay=0.0):
    """one fp64 AdamW step (torch.optim.AdamW's definition: p *= 1 - lr wd, then Adam's update) on gr = g * grad_scale * coef, from the given
    fp32 state, with `coef` AS READ BACK from the record (an exact fp32 value: the bounds do not carry the norm's error).  adam_ref's model
    with the roundings this kernel adds, in U32:
      gr = g * (gs * coef):        gs's rounding 1, the product gs * coef 1, the product with g 1                                   = 3   (adam_ref: 2)
      m = b1 m0 + (1 - b1) gr:     on |b1 m0| 3;  on |(1 - b1) gr|: (1 - b1) 1, gr 3, product 1, sum 1                              = 6
      v = b2 v0 + (1 - b2) gr gr:  on b2 v0 3;  on (1 - b2) gr^2: (1 - b2) 1, gr 3 + 3, two products 2, sum 1                       = 10
      den = sqrt(v) / sqrt(bc2) + eps:   10 / 2 + C_SQRT, 1 / sqrt(bc2) 1, product 1, eps 1, sum 1                                 = 9 + C_SQRT
      update = (lr / bc1) m / den: lr / bc1 1, product 1, den, division C_DIV: (11 + C_SQRT + C_DIV) |update| + (lr / bc1) B_m / den
      pd = p0 d, d = 1 - lr wd:    d's rounding 1, the product 1 = 2 on |pd|; nothing when wd == 0 (d == 1 and p0 * 1 are exact)
      p = pd - update:             one rounding of p + pd's bound + the update's bound."""
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    bc1 = 1.0 - beta1 ** step; bc2 = 1.0 - beta2 ** step
    gr = g * (grad_scale * coef)
    t1, t2 = beta1 * m, (1.0 - beta1) * gr
    m1 = t1 + t2
    b_m = U32 * (3 * t1.abs() + 6 * t2.abs())
    v1 = beta2 * v + (1.0 - beta2) * gr * gr
    b_v = U32 * (3 * beta2 * v + 10 * (1.0 - beta2) * gr * gr)
    den = v1.sqrt() / math.sqrt(bc2) + eps
    upd = (lr / bc1) * m1 / den
    b_u = U32 * (11 + C_SQRT + C_DIV) * upd.abs() + (lr / bc1) * b_m / den
    pd = p * (1.0 - lr * weight_decay)
    b_pd = 2 * U32 * pd.abs() if weight_decay != 0 else torch.zeros_like(pd)
    p1 = pd - upd
    return dict(p=p1, m=m1, v=v1, b_p=U32 * p1.abs() + b_pd + b_u, b_m=b_m, b_v=b_v)


def guarded_adam_emul(p, g, m, v, step, coef, apply, lr=E.ADAM_LR, beta1=E.ADAM_B1, beta2=E.ADAM_B2, eps=1e-8, grad_scale=1.0, weight_decay=0.0,
                      defect=None):
    """hftt_adam_step_guarded + adam_guarded_kernel in fp32; coef / apply: the record's words (gnorm_emul's)"""
    assert defect is None or defect in DEFECTS['adam']
    omb2 = f32(1.0 - beta2)
    if not apply:
        if defect == 'skip_still_updates_v':
            gr = g * f32(grad_scale)
            return p, m, f32(beta2) * v + omb2 * gr * gr
        return p, m, v
    bc1 = 1.0 - beta1 ** step; bc2 = 1.0 - beta2 ** step
    lr_c = f32(lr / bc1); isb2 = f32(1.0 / math.sqrt(bc2))
    s = float(np.float32(grad_scale) * np.float32(coef))
    d = f32(1.0 - lr * weight_decay)
    gr = g * s
    if defect == 'decay_coupled_into_gradient':                 # the L2 form: decay joins the gradient and so the moments
        gr = gr + f32(weight_decay) * p
    elif defect != 'decay_after_update':
        p = p * d
    m = f32(beta1) * m + f32(1.0 - beta1) * gr
    gv = g * f32(grad_scale) if defect == 'clip_not_in_v' else gr
    v = f32(beta2) * v + omb2 * gv * gv
    p = p - lr_c * m / (v.sqrt() * isb2 + f32(eps))
    if defect == 'decay_after_update':
        p = p * d
    return p, m, v


def guarded_adam_check(got_p, got_m, got_v, ref):
    return E.adam_check(got_p, got_m, got_v, ref)


def skip_check(before, after):
    """a skipped step writes nothing: p, m, v keep their BITS (compared as integers: a NaN that was there stays equal to itself)"""
    bad = []
    for name, a, b in zip('pmv', before, after):
        changed = int((a.contiguous().view(torch.int32) != b.contiguous().view(torch.int32).to(a.device)).sum())
        if changed:
            bad.append(('%s changed by a skipped step' % name, -1, float('nan'), 0.0, changed))
    return bad
