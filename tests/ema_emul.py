"""fp64 reference, restatement and rounding-model criteria of the averaged weights carried inside the Adam step (csrc/guard.hip:
hftt_adam_step_ema / adam_ema_kernel): behind adam_update, on the NEW parameters,

    y = omd * (p - e) - c;   t = e + y;   c = (t - e) - y;   e = t;          omd = (float)(1 - beta)

the exponential moving average e = beta e + (1 - beta) p of torch.optim.swa_utils.get_ema_multi_avg_fn(beta) as a compensated (Kahan) fp32
sum.  Same three things as tests/guard_emul.py, in torch and device-agnostic:

  ema_ref    the recurrence in fp64 on the same fp32 p sequence, with the bounds;
  ema_emul   the kernel's arithmetic restated in fp32, one rounding per operation; defect=<name> selects one deliberately wrong variant (DEFECTS);
  ema_check  the list of violations (empty = pass);  bits_check: what a skipped step and a frozen quad must leave alone.

tests/test_ema_emul_bound.py shows on the CPU that the restatement passes every criterion and every defect fails one, and records which
input family sees which defect; tests/test_ema_gpu.py holds the kernel and FusedAdam(ema_decay=...) to the criteria.
"""
import functools

import numpy as np
import torch

import elementwise_emul as E
from elementwise_emul import U32, F32_TINY, f32, violations
from guard_emul import GRID_PASS

DEFECTS = ('uncompensated', 'averages_old_p', 'skip_still_averages', 'frozen_quad_written', 'decay_rounded_before_subtraction')

# adam_ema_kernel runs the grid of the other Adam kernels over quads (n % 4 == 0 is the entry point's rule): one quad, two, one workgroup
# less a quad, one workgroup and a quad, and two quads behind the first grid pass
EMA_N = (4, 8, 1020, 1028, GRID_PASS + 8)
EMA_DECAYS = (0.9, 0.9999)
SENTINEL = 0x4B3C614E                    # 12345678.0f, far from every parameter: an average towards p moves it (a NaN would propagate unchanged)

# the stagnation family: Adam leaves p fixed (g = 0, m = v = 0), p sits 2e-4 |e0| away from the average's start and beta = 0.9999.  One call
# wants to add (1 - beta)(p - e) = 2e-8 |e|, below half an ulp of e (2^-25 |e| = 2.98e-8 |e| at the least): the plain fp32 sum never moves,
# while the fp64 average moves by (1 - beta^K) 2e-4 |e0| = 3.6e-5 |e0| over K = 2000 calls -- about 300 ulp.
STAG_BETA, STAG_REL, STAG_K, STAG_N = 0.9999, 2e-4, 2000, 1028


def warmup_decay(decay, t):
    """the decay of call t (0-based) under FusedAdam(ema_warmup=True): min(decay, (1 + t) / (10 + t))"""
    return min(float(decay), (1.0 + t) / (10.0 + t))


@functools.lru_cache(maxsize=None)
def _start(n, seed):
    return E.adam_state(n, seed + n % 1000)


def ema_start(n, seed=0):
    """random family: (p, m, v) of adam_state and an average e0 that is ANOTHER draw of adam_state's p (exact zeros, 1e-8 .. 1 log-uniform,
    N(0, 1): |e| above, below and far from |p|, so the compensated sum sees both magnitude orders); the gradients are adam_grad's stream"""
    p, m, v = (t.clone() for t in _start(n, seed))
    return p, m, v, _start(n, seed + 5)[0].clone()


def stagnation_start(n=STAG_N, seed=0):
    """(p, e0): e0 = N(0, 1) pushed away from zero, p = fl(e0 (1 + 2e-4))"""
    g = torch.Generator().manual_seed(4242 + seed)
    e0 = torch.randn(n, generator=g)
    e0 = torch.where(e0.abs() < 0.05, torch.full_like(e0, 0.7), e0)
    return (e0.double() * (1.0 + STAG_REL)).float(), e0


def frozen_elements(quad_group, frozen):
    """per-element bool mask from the per-quad group map (uint8 [n / 4]) and one flag per group"""
    fq = torch.as_tensor(list(frozen), dtype=torch.bool)[quad_group.long().cpu()]
    return fq.repeat_interleave(4)


# ================================================================================================ reference
def ema_ref(e0, ps, betas, c0=None):
    """E_k = E_{k-1} + (1 - beta_k)(p_k - E_{k-1}) in fp64 over the fp32 sequence ps (a list of tensors, the parameters AFTER each step),
    from A_0 = e0 - c0 (c0 None: zeros).  Returns dict(e = E_K, b_e, b_a): bounds for the kernel's e and for the value it represents,
    a = e - c (Kahan: c is what the last sum added beyond y, so e - c is the sum without its last rounding).

    The model, per call, in U32 (first order; beta, p, e, c of that call; E stands for e in the bounds, the difference is second order):
      d = p - e                  one rounding                                                                    1 on |p - e|
      q = omd * d                omd = (float)(1 - beta) rounded once 1, the product 1                           2 on (1 - beta)|p - e|
      y = q - c;  t = e + y;  c' = (t - e) - y      the compensated sum: each addend enters perturbed by at most 2 U32 whatever the
                                 order of |e| and |y| (Goldberg 1991, Theorem 8); with |e| >= |y| the pair (t, c') holds e + y exactly and
                                 one of the two is spare                                                         2 on (1 - beta)|p - e|
      so a' = e + y = a + (1 - beta)(p - e) + r,  |r| <= 5 U32 (1 - beta)|p - e|,  and p - e = p - a - c:
      D' = a' - E' = beta D - (1 - beta) c + r        the FEEDBACK: the kernel subtracts e, not e - c, and |c| <= U32 |e| (c is the
                                 rounding error of a sum that came out as e; the given c0 at the first call)
      b_a' = beta b_a + (1 - beta)|c| + 5 U32 (1 - beta)|p - e| + 4 F32_TINY        (four results that may be flushed below the normal range)
    The geometric weights sum to at most 1, so over ANY number of calls b_a <= U32 max|e| + 5 U32 max|p - e|: it does not grow with K.
      b_e = b_a + U32 |E_K|      the kernel's e carries the last sum's rounding, which a has not: |e - a| = |c| <= U32 |e|."""
    a = e0.double() - (0.0 if c0 is None else c0.double())
    cmag = torch.zeros_like(a) if c0 is None else c0.double().abs()
    b = torch.zeros_like(a)
    for p, beta in zip(ps, betas):
        omd = 1.0 - beta
        diff = p.double() - a
        b = beta * b + omd * cmag + 5 * U32 * omd * diff.abs() + 4 * F32_TINY
        a = a + omd * diff
        cmag = U32 * a.abs()
    return dict(e=a, b_a=b, b_e=b + U32 * a.abs())


# ================================================================================================ restatement
def ema_emul(e, c, p_new, beta, p_old=None, apply=True, frozen=None, defect=None):
    """one call of adam_ema_kernel's average in fp32 on the CPU: (e, c) -> (e', c').  p_new: the parameters after adam_update; p_old: before
    it (the averages_old_p defect); apply: the guard record's word (False: the launch returns without a store); frozen: per-ELEMENT bool mask
    of the frozen quads (neither loaded nor stored), or None."""
    assert defect is None or defect in DEFECTS
    if not apply and defect != 'skip_still_averages':
        return e, c
    omd = float(np.float32(1.0) - np.float32(beta)) if defect == 'decay_rounded_before_subtraction' else f32(1.0 - beta)
    p = p_old if defect == 'averages_old_p' else p_new
    d = p - e
    q = omd * d
    if defect == 'uncompensated':
        t, c1 = e + q, c
    else:
        y = q - c
        t = e + y
        c1 = (t - e) - y
    if frozen is not None and defect != 'frozen_quad_written':
        t, c1 = torch.where(frozen, e, t), torch.where(frozen, c, c1)
    return t, c1


# ================================================================================================ criteria
def ema_check(got_e, got_c, ref, keep=None):
    """e against the fp64 average within b_e, and e - c (formed in fp64) within b_a; keep: bool mask of the elements to judge (the unfrozen)"""
    ge, gc = got_e.detach().cpu().double().reshape(-1), got_c.detach().cpu().double().reshape(-1)
    re, ba, be = ref['e'].reshape(-1), ref['b_a'].reshape(-1), ref['b_e'].reshape(-1)
    if keep is not None:
        k = keep.reshape(-1).cpu()
        ge, gc, re, ba, be = ge[k], gc[k], re[k], ba[k], be[k]
    return violations('e', ge, re, be) + violations('e - c', ge - gc, re, ba)


def bits_check(name, before, after, where=None):
    """`after` keeps the BITS of `before` (compared as integers: a NaN stays equal to itself), everywhere or on the bool mask `where`"""
    a, b = before.detach().cpu().contiguous().view(torch.int32), after.detach().cpu().contiguous().view(torch.int32)
    diff = a != b
    if where is not None:
        diff = diff & where.reshape(-1).cpu()
    changed = int(diff.sum())
    return [('%s changed' % name, int(diff.nonzero()[0]), float('nan'), 0.0, changed)] if changed else []
