"""Peaked softmax rows for the x3 and parity attention kernels: inputs, a derived fp64 bound, CPU stand-ins and planted defects (test
infrastructure, CPU; no GPU import).

What the suite did not hold.  The attention checks before this module compare max-normalised tensors inside bands calibrated on `randn` scores
(largest |score| 5.379), or judge dq / dk against a product of operand maxima where the rows are one-hot (tests/test_x3_gpu.py, qk_scale 40:
restated in tests/test_attn_peaked_emul_bound.py).  The first encoder and the first time layer run on rows with two to four live keys an O(1)
gap apart that sit on scores of 10^2 .. 10^5 (DESIGN.md sections 2, 3); there the fp16-pair split of Q.K^T, the raw-maximum subtraction,
delta = rowsum(dO * O) and the bf16-pair gradient products decide the result.

Inputs (every value exact in fp32; the magnitude reached is MEASURED: magnitude()):
  near_dup     keys in groups of 2 .. 4 within eps of a common base of norm r, r^2 = L sqrt(dh); a query near a base; eps = 1.5 sqrt(dh) / r,
               so the score gaps inside a group are O(1).  dq = sum_j dS_j k_j cancels to the eps scale (sum_j dS_j = 0): harsh for dk, dv,
               out and the map.
  solved_ties  unrelated keys; every query is the minimum-norm solution of k_j . q = (L - gap_j) sqrt(dh) on a live set of 2 .. 4 keys with
               gaps drawn in [0, 4] (one of them 0); a key outside the set that would come within 8 of the top is pinned 12 below it by one
               more equation.  dq does not cancel.
v is plain randn or the common-part-plus-small form of test_attention_backward_where_dp_and_delta_nearly_cancel; dO is gradient-sized (1e-3).

The derived bound (bound(): fp64, element by element, from the operands alone).  Unit roundoffs: fp32 U32 = 2^-24, fp16 2^-11, bf16 2^-8.
  * an fp32 sum of K products carries (K + 16) U32 of the sum of their magnitudes (the term bf16_plan_emul.score_terms uses): acc(K);
  * an fp16 pair hi + lo represents x to 2^-22 |x|, or to 2^-25 (half an fp16 subnormal step) once lo is subnormal; three passes
    hi.hi + hi.lo + lo.hi drop lo.lo <= 2^-22 |a b|: the split unit of a forward product is 3 * 2^-22 of the abs-sum, plus 2^-25 per
    operand element against the other operand (csrc/x3_common.h: x3_split2, x3_mma; x3_emul._split);
  * a bf16 pair in the same way: 3 * 2^-16 of the abs-sum (fp32's exponent range: no subnormal term above the format floor); on planes the
    pair is formed from the stored fp16 pair hi + lo instead of the fp32 value: 2^-22 more, and 2^-25 ABSOLUTE per stored element of q, k, v
    against the other factor (lo is subnormal for |x| < 2^-3) -- no relative unit covers an operand element near zero, and the planes
    backward was 2.4 x a bound without this term on dk (solved_ties, magnitude 45, 88 x 256) where the fp32-operand kernel sat at 0.009;
  * parity (npass 3) has no split term; its scores are scaled before the maximum is taken: two more U32.
  score j of a row:  delta_j = (u_s A_j + floor terms) / sqrt(dh) + the same at the row maximum,  A_j = sum_c |q_c k_jc|
  dP_j   <= P_j (e^delta_j - 1 + sum_l P_l (e^delta_l - 1) + tail),  tail = (3 arg + C_EXP + 2 LSE_INV_ULPS + C_DIV + 1) U32 as score_terms
  dO     through |v| of the kept keys, + the P.V product's own unit, + 2^-25 |v_j| per key (p <= 1 below 6e-5 is an fp16 subnormal)
  dDelta through |dO| dO_err + acc(dh) sum |dO O|
  d(dP)  = u_b(dh) |dO| . |v|;   d(dS) <= dP |dP' - Delta| + P (keep d(dP) + dDelta) + 4 U32 P (|dP'| + |Delta|)
  dQ, dK, dV sum those through |k|, |q|, |dO| and add their own product's unit.
With dropout the exact keep mask and keep scale multiply P in P.V, dV and dP (where the kernels apply them); the map is pre-dropout.
Floor: FLOOR = 2^-126, the smallest normal fp32 number (a result below it may be flushed to zero on the device), added to P, dS and every
figure -- a floor of the FORMAT, not of the data: a key no query looks at has a gradient of 1e-290 in fp64 and of exactly 0 on the device.

Criterion, two layers, both must hold (check()):
  (a) every element of out, map, row maximum, 1/sum, dq, dk, dv inside the derived bound;
  (b) per tensor e_dev <= 3 (e32 + e_x3) + 1e-6, max-normalised (the rule of test_attention_backward_where_dp_and_delta_nearly_cancel):
      e32 of the plain fp32 evaluation, e_x3 of the fp64 model of the mode's roundings (0 for parity).
(a) alone is 10 .. 1,000 x loose on dq of near_dup (an honest bound does not cancel); (b) alone is blind to single rows.

Planted defects (chain(defect=...); each fails the criterion on the fp32 stand-in at the figure, family and magnitude DEFECTS names):
  qk_hi_only, dp_drop_lohi, zero_peaked_rows, delta_from_bf16_o, p_fp16, keep_scale_twice, inv_of_neighbour, dk_without_scale, and
  scale_then_subtract -- which CANNOT be seen: s c - max c rounds each score to U32 |s|, (dh + 16) x below the score term of any honest
  bound, and the fp32 evaluation behind e32 performs the same rounding; what it breaks (a whole row underflowing at |score| 1e9) is held on
  exactly representable inputs by test_attention_with_scores_of_1e9.  The nearest visible defect is planted instead: max_from_hi, the row
  maximum taken from the hi.hi pass alone (2^-11 of A on the stored maximum, e^shift on 1/sum).
"""
import math

import torch

import util
from elementwise_emul import U32, C_EXP, C_DIV
from bf16_emul import LSE_INV_ULPS
from x3_emul import _split, x3mm

F64, F32 = torch.float64, torch.float32
FLOOR = 2.0 ** -126
U_F16PAIR = 3.0 * 2.0 ** -22
U_BF16PAIR = 3.0 * 2.0 ** -16
SUB16 = 2.0 ** -25

MAGS = (5.0, 45.0, 1500.0, 1.0e5)
FAMILIES = ('near_dup', 'solved_ties')
V_FORMS = ('randn', 'common')
GEOMS = [(2, 2, 48, 48, 32), (2, 2, 12, 48, 32), (2, 4, 88, 88, 64), (2, 4, 88, 256, 64), (2, 4, 256, 256, 64), (2, 4, 72, 100, 64), (2, 1, 100, 70, 64)]
FIGURES = ('out', 'map', 'mx', 'inv', 'dq', 'dk', 'dv')
LIVE_P2, LIVE_ROW = 1e-2, 1e-2          # conditions on the inputs: second-largest probability, row size against the tensor's maximum
LIVE_SHARE = 0.9
LOOKED_P = 0.1


def acc(K):
    return (K + 16) * U32


def heads(t, H):
    n, L, d = t.shape
    return t.reshape(n, L, H, d // H).transpose(1, 2)


def unheads(t):
    n, H, L, dh = t.shape
    return t.transpose(1, 2).reshape(n, L, H * dh)


# ---------------------------------------------------------------------------------------------------------------------------- inputs
def _values(n, Lk, d, form, g):
    if form == 'common':
        return torch.randn(1, 1, d, generator=g, dtype=F64) * 3.0 + torch.randn(n, Lk, d, generator=g, dtype=F64) * 0.01
    return torch.randn(n, Lk, d, generator=g, dtype=F64)


def _group_ids(Lk):
    sizes, left, i = [], Lk, 0
    while left > 0:
        s = (4, 3, 2)[i % 3]
        if left - s < 2:
            s = left
        sizes.append(s); left -= s; i += 1
    return torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes)), len(sizes)


def near_dup(n, H, Lq, Lk, dh, L, seed, v_form='randn', shared=False):
    """(q, k, v, do) as fp32.  shared: one query block and one set of bases for all sequences (q is returned as [1, Lq, d])"""
    g = torch.Generator().manual_seed(seed)
    r = math.sqrt(L * math.sqrt(dh))
    eps = 1.5 * math.sqrt(dh) / r
    gid, G = _group_ids(Lk)
    nb = 1 if shared else n
    base = torch.randn(nb, H, G, dh, generator=g, dtype=F64)
    base = base / base.norm(dim=-1, keepdim=True) * r
    kh = base[:, :, gid].expand(n, H, Lk, dh) + eps * torch.randn(n, H, Lk, dh, generator=g, dtype=F64)
    pick = torch.randint(0, G, (nb, H, Lq), generator=g)
    qh = torch.gather(base, 2, pick.unsqueeze(-1).expand(nb, H, Lq, dh)) + eps * torch.randn(nb, H, Lq, dh, generator=g, dtype=F64)
    v = _values(n, Lk, H * dh, v_form, g)
    do = torch.randn(n, Lq, H * dh, generator=g, dtype=F64) * 1e-3
    return tuple(t.float() for t in (unheads(qh), unheads(kh), v, do))


def solved_ties(n, H, Lq, Lk, dh, L, seed, v_form='randn', shared=False):
    g = torch.Generator().manual_seed(seed)
    rk = math.sqrt(1.7 * L * math.sqrt(dh))
    kh = torch.randn(n, H, Lk, dh, generator=g, dtype=F64) * (rk / math.sqrt(dh))
    kh = kh.float().double()
    nb = 1 if shared else n
    if shared:                                     # one query for all sequences: every sequence holds the first one's keys in an order of its own
        kh = torch.stack([kh[0]] + [kh[0][:, torch.randperm(Lk, generator=g)] for _ in range(n - 1)])
    J0, extra = 4, 6 if L >= 20.0 else 0
    m = torch.randint(2, 5, (nb, H, Lq), generator=g)
    idx = torch.stack([torch.randperm(Lk, generator=g)[:J0] for _ in range(nb * H * Lq)]).view(nb, H, Lq, J0)
    gap = torch.rand(nb, H, Lq, J0, generator=g, dtype=F64) * 4.0
    gap[..., 0] = 0.0
    w = (torch.arange(J0).view(1, 1, 1, J0) < m.unsqueeze(-1)).double()
    t = (L - gap) * math.sqrt(dh)
    kq = kh[:nb]                                   # shared: the query is solved on the first sequence's keys
    for it in range(extra + 1):
        J = idx.shape[-1]
        Ka = torch.gather(kq.unsqueeze(2).expand(nb, H, Lq, Lk, dh), 3, idx.unsqueeze(-1).expand(nb, H, Lq, J, dh))
        Gm = (Ka @ Ka.transpose(-1, -2)) * (w.unsqueeze(-1) * w.unsqueeze(-2)) + torch.diag_embed(1.0 - w)
        al = torch.linalg.solve(Gm, (t * w).unsqueeze(-1)).squeeze(-1) * w
        qh = (al.unsqueeze(-2) @ Ka).squeeze(-2)
        if it == extra:
            break
        s = (qh @ kq.transpose(-1, -2)) / math.sqrt(dh)
        s = torch.where(torch.zeros_like(s).scatter_add(-1, idx, w) > 0, torch.full_like(s, -1e300), s)     # keys already in the system do not count
        top, at = s.max(-1)
        viol = (top > L - 8.0).double()
        idx = torch.cat([idx, at.unsqueeze(-1)], -1)
        w = torch.cat([w, viol.unsqueeze(-1)], -1)
        t = torch.cat([t, torch.full_like(top, (L - 12.0) * math.sqrt(dh)).unsqueeze(-1)], -1)
    v = _values(n, Lk, H * dh, v_form, g)
    do = torch.randn(n, Lq, H * dh, generator=g, dtype=F64) * 1e-3
    return tuple(x.float() for x in (unheads(qh), unheads(kh), v, do))


def make(family, geom, L, v_form='randn', shared=False, seed=None):
    n, H, Lq, Lk, dh = geom
    seed = seed if seed is not None else 1000 * Lq + Lk + dh + int(L) % 977
    return (near_dup if family == 'near_dup' else solved_ties)(n, H, Lq, Lk, dh, L, seed, v_form, shared)


def magnitude(q, k, H):
    """largest |score| / sqrt(dh), fp64"""
    qh, kh = heads(q.double(), H), heads(k.double(), H)
    return ((qh @ kh.transpose(-1, -2)).abs().max() / math.sqrt(qh.shape[-1])).item()


# ---------------------------------------------------------------------------------------------------------------------------- the chain
DEFECTS = {
    # name: (family, magnitude, v form, dropout, the figure that must fail)
    'qk_hi_only': ('near_dup', 45.0, 'randn', 0.0, 'out'),
    'dp_drop_lohi': ('near_dup', 45.0, 'common', 0.0, 'dq'),
    'zero_peaked_rows': ('solved_ties', 1500.0, 'randn', 0.0, 'dq'),
    'max_from_hi': ('near_dup', 1500.0, 'randn', 0.0, 'mx'),
    'delta_from_bf16_o': ('solved_ties', 45.0, 'common', 0.0, 'dq'),
    'p_fp16': ('near_dup', 5.0, 'randn', 0.0, 'out'),
    'keep_scale_twice': ('solved_ties', 45.0, 'randn', 0.1, 'dk'),
    'inv_of_neighbour': ('near_dup', 45.0, 'randn', 0.0, 'map'),
    'dk_without_scale': ('solved_ties', 1500.0, 'randn', 0.0, 'dk'),
}
INVISIBLE = ('scale_then_subtract',)


def chain(q, k, v, do, H, dtype, mode, mask=None, keep_sc=1.0, defect=None, planes=False):
    """One attention, forward and backward, written out: {out, map, mx, inv, dq, dk, dv} as fp64.
    mode 'plain': the products as they stand in `dtype` (fp64: the reference; fp32: the fp32 evaluation), scores scaled before the maximum;
    mode 'x3': the x3 mode's operand splits (fp16 pairs forward, bf16 pairs backward), raw maximum subtracted before the scale,
    delta = rowsum(dO * O).  mx is the raw maximum for 'x3' and the scaled one for 'plain' (what the kernels store).  q may be [1, Lq, d].
    planes ('x3'): q, k, v are stored as f16-pair planes -- the forward reads the same halves either way, the backward forms its bf16 pairs
    from hi + lo instead of the fp32 value."""
    n = k.shape[0]
    qh, kh, vh, doh = (heads(t.to(dtype), H) for t in (q.expand(n, -1, -1), k, v, do))
    dh = qh.shape[-1]
    c = torch.tensor(1.0 / math.sqrt(dh), dtype=dtype)
    mk = None if mask is None else mask.to(dtype) * keep_sc
    x3 = mode == 'x3'
    mm_f = (lambda a, b, **kw: x3mm(a, b, 'f16', **kw)) if x3 else (lambda a, b, **kw: torch.matmul(a, b))
    mm_b = (lambda a, b, **kw: x3mm(a, b, 'bf16', **kw)) if x3 else (lambda a, b, **kw: torch.matmul(a, b))
    kT = kh.transpose(-1, -2)
    if defect == 'qk_hi_only':
        s = torch.matmul(_split(qh, 'f16')[0], _split(kT, 'f16')[0])
    else:
        s = mm_f(qh, kT)
    if x3:
        mx = s.amax(-1, keepdim=True)
        if defect == 'max_from_hi':
            mx = torch.matmul(_split(qh, 'f16')[0], _split(kT, 'f16')[0]).amax(-1, keepdim=True)
        z = (s * c).float().to(dtype) - (mx * c).float().to(dtype) if defect == 'scale_then_subtract' else (s - mx) * c
    else:
        s = s * c
        mx = s.amax(-1, keepdim=True)
        z = s - mx
    e = torch.exp(z)
    inv = 1.0 / e.sum(-1, keepdim=True)
    if defect == 'inv_of_neighbour':
        inv = torch.roll(inv, 1, dims=-2)
    P = e * inv
    Pd = P if mk is None else P * mk
    pv = Pd.half().to(dtype) if defect == 'p_fp16' else Pd
    O = mm_f(pv, vh)
    if x3 and planes:
        qh, kh, vh = (sum(_split(t, 'f16')) for t in (qh, kh, vh))
    dP = mm_b(doh, vh.transpose(-1, -2), drop_lohi=(defect == 'dp_drop_lohi'))
    if mk is not None:
        dP = dP * mk * (keep_sc if defect == 'keep_scale_twice' else 1.0)
    Od = O.bfloat16().to(dtype) if defect == 'delta_from_bf16_o' else O
    delta = (doh * Od).sum(-1, keepdim=True)
    dS = P * (dP - delta)
    if defect == 'zero_peaked_rows':
        dS = torch.where(P.amax(-1, keepdim=True) > 0.9, torch.zeros_like(dS), dS)
    dq = mm_b(dS, kh) * c
    dk = mm_b(dS.transpose(-1, -2), qh) * (1.0 if defect == 'dk_without_scale' else c)
    dv = mm_b(Pd.transpose(-1, -2), doh)
    return dict(out=unheads(O).double(), map=P.double(), mx=mx.squeeze(-1).double(), inv=inv.squeeze(-1).double(),
                dq=unheads(dq).double(), dk=unheads(dk).double(), dv=unheads(dv).double())


# ---------------------------------------------------------------------------------------------------------------------------- the bound
def bound(q, k, v, do, H, mode, mask=None, keep_sc=1.0, planes=False):
    """{figure: per-element bound} in fp64, from the operands alone (module docstring).  mode 'x3' or 'parity'."""
    n = k.shape[0]
    qh, kh, vh, doh = (heads(t.double(), H) for t in (q.expand(n, -1, -1), k, v, do))
    Lq, Lk, dh = qh.shape[-2], kh.shape[-2], qh.shape[-1]
    c = 1.0 / math.sqrt(dh)
    x3 = mode == 'x3'
    mk = torch.ones(n, H, Lq, Lk, dtype=F64) if mask is None else mask.double() * keep_sc
    s = qh @ kh.transpose(-1, -2)
    A = qh.abs() @ kh.abs().transpose(-1, -2)
    if x3:
        ds = (acc(dh) + U_F16PAIR) * A + SUB16 * (qh.abs().sum(-1, keepdim=True) + kh.abs().sum(-1).unsqueeze(-2))
        uf, ub = U_F16PAIR, U_BF16PAIR + (2.0 ** -22 if planes else 0.0)
    else:
        ds = (acc(dh) + 2 * U32) * A
        uf = ub = 0.0
    top = s.argmax(-1, keepdim=True)
    dl = c * (ds + ds.gather(-1, top))
    P = torch.softmax(s * c, -1)
    ex = torch.expm1(dl)
    inv_rel = (P * ex).sum(-1, keepdim=True)
    arg = (s.gather(-1, top) - s) * c
    relP = ex + inv_rel + (3.0 * arg + C_EXP + 2 * LSE_INV_ULPS + C_DIV + 1) * U32
    bP = P * relP + FLOOR
    b_mx = ds.amax(-1) * (1.0 if x3 else c) + FLOOR
    inv = 1.0 / torch.exp((s - s.gather(-1, top)) * c).sum(-1)
    b_inv = inv * (inv_rel.squeeze(-1) + (2 * LSE_INV_ULPS + C_DIV + 1) * U32) + FLOOR
    Pd = P * mk
    va = vh.abs()
    bO = (bP * mk) @ va + (acc(Lk) + uf) * (Pd @ va) + FLOOR
    if x3:
        bO = bO + SUB16 * (mk @ va + Pd.sum(-1, keepdim=True))
    O = Pd @ vh
    doa = doh.abs()
    dP = (doh @ vh.transpose(-1, -2)) * mk
    sub = SUB16 if (x3 and planes) else 0.0          # a stored f16 pair is off by up to 2^-25 ABSOLUTE where its lo half is subnormal (|x| < 2^-3)
    b_dP = ((acc(dh) + ub) * (doa @ va.transpose(-1, -2)) + sub * doa.sum(-1, keepdim=True)) * mk
    Dl = (doh * O).sum(-1, keepdim=True)
    b_Dl = (doa * bO).sum(-1, keepdim=True) + acc(dh) * (doh * O).abs().sum(-1, keepdim=True)
    dS = P * (dP - Dl)
    b_dS = bP * (dP - Dl).abs() + P * (b_dP + b_Dl) + 4 * U32 * P * (dP.abs() + Dl.abs()) + FLOOR
    b_dq = c * (b_dS @ kh.abs() + (acc(Lk) + ub) * (dS.abs() @ kh.abs()) + sub * dS.abs().sum(-1, keepdim=True)) + FLOOR
    b_dk = c * (b_dS.transpose(-1, -2) @ qh.abs() + (acc(Lq) + ub) * (dS.abs().transpose(-1, -2) @ qh.abs()) + sub * dS.abs().sum(-2).unsqueeze(-1)) + FLOOR
    b_dv = (bP * mk).transpose(-1, -2) @ doa + (acc(Lq) + ub) * (Pd.transpose(-1, -2) @ doa) + FLOOR
    return dict(out=unheads(bO), map=bP, mx=b_mx, inv=b_inv, dq=unheads(b_dq), dk=unheads(b_dk), dv=unheads(b_dv))


# ---------------------------------------------------------------------------------------------------------------------------- the criterion
def rel(a, r):
    return ((a.double() - r).abs().max() / r.abs().max()).item()


class Case:
    """One input set with everything that depends on it alone: fp64 reference, fp32 evaluation, fp64 x3 model, both bounds.  Computed once
    and shared by the checks of all kernel forms on these inputs."""

    def __init__(self, q, k, v, do, H, mask=None, keep_sc=1.0):
        self.q, self.k, self.v, self.do, self.H, self.mask, self.keep_sc = q, k, v, do, H, mask, keep_sc
        a = (q, k, v, do, H)
        self.ref = chain(*a, F64, 'plain', mask, keep_sc)
        self.e32 = chain(*a, F32, 'plain', mask, keep_sc)
        self.x3 = chain(*a, F64, 'x3', mask, keep_sc)
        self._b, self._x3p = {}, None

    def model(self, mode, planes=False):
        """the fp64 model of the mode's roundings (None for parity: e_x3 = 0)"""
        if mode != 'x3':
            return None
        if not planes:
            return self.x3
        if self._x3p is None:
            self._x3p = chain(self.q, self.k, self.v, self.do, self.H, F64, 'x3', self.mask, self.keep_sc, planes=True)
        return self._x3p

    def bound(self, mode, planes=False):
        key = (mode, planes)
        if key not in self._b:
            self._b[key] = bound(self.q, self.k, self.v, self.do, self.H, mode, self.mask, self.keep_sc, planes)
        return self._b[key]

    def reference(self, fig, mode):
        """the fp64 value of a figure as `mode` stores it: the x3 kernels keep the RAW row maximum"""
        if fig == 'mx' and mode == 'x3':
            return self.ref['mx'] * math.sqrt(self.q.shape[-1] // self.H)
        return self.ref[fig]

    def conditions(self):
        """(share of query rows with a second-largest probability >= LIVE_P2, share of dq rows and of looked-at dk rows above LIVE_ROW of
        their tensor's maximum) from the fp64 reference"""
        P = self.ref['map']
        p2 = (P.topk(2, -1).values[..., 1] >= LIVE_P2).double().mean().item()
        dqr = self.ref['dq'].abs().amax(-1)
        dq_share = (dqr >= LIVE_ROW * dqr.max()).double().mean().item()
        # dk per (head, key).  Looked at: some query gives the key a probability of LOOKED_P = 0.1 or more -- a key seen with 1e-2 has a
        # dk row of about 1e-2 of a key seen with 1, which the row condition would then be asking of it by construction; from 0.1 the
        # condition leaves a factor of ten for |dP - delta| and for the number of queries that look
        looked = P.amax(-2) >= LOOKED_P                                  # [n, H, Lk]
        dkr = heads(self.ref['dk'], self.H).abs().amax(-1)
        dk_share = (dkr[looked] >= LIVE_ROW * dkr.max()).double().mean().item()
        return p2, dq_share, dk_share

    def assert_conditions(self, tag=''):
        p2, dq_share, dk_share = self.conditions()
        assert p2 >= LIVE_SHARE and dq_share >= LIVE_SHARE and dk_share >= LIVE_SHARE, (tag, p2, dq_share, dk_share)


def check(case, got, mode, planes=False, figures=FIGURES):
    """got: {figure: tensor}.  Returns ({figure: (worst measured / bound, e_dev, 3 (e32 + e_x3) + 1e-6)}, [failures as text])"""
    b = case.bound(mode, planes)
    model = case.model(mode, planes)
    figs, bad = {}, []
    for f in figures:
        if f not in got or got[f] is None:
            continue
        r = case.reference(f, mode)
        a = got[f].detach().double().cpu().reshape(r.shape)
        if not bool(torch.isfinite(a).all()):
            bad.append('%s: non-finite values' % f)
            continue
        ratio = ((a - r).abs() / b[f]).max().item()
        e_dev = rel(a, r)
        if f == 'mx':
            allow = float('inf')                      # (b) is a rule for tensors judged against their maximum; the row maximum has layer (a) only
        else:
            allow = 3.0 * (rel(case.e32[f], case.ref[f]) + (rel(model[f], case.ref[f]) if model is not None else 0.0)) + 1e-6
        figs[f] = (ratio, e_dev, allow)
        if not ratio <= 1.0:
            bad.append('%s: (a) an element is %.3g x its derived bound' % (f, ratio))
        if not e_dev <= allow:
            bad.append('%s: (b) e_dev %.3g > 3 (e32 + e_x3) + 1e-6 = %.3g' % (f, e_dev, allow))
    return figs, bad


def check_plan_launch(rec, got, forward):
    """An attention launch of an engine plan under the criterion, on the device's own operands.  rec: the launch record of
    fwd_plan_emul / bwd_plan_emul.make_record (q [n or 1, Lq, d], k, v (, dout) decoded from planes where the plan stores planes; H, drop_p,
    site, seed, planes, mode, shape); got: the fetched outputs.  -> (figures, failures, largest |score| / sqrt(dh))"""
    n, H, Lq, Lk = rec['shape']
    p = rec.get('drop_p', 0.0)
    q, k, v = (rec[x].float() for x in ('q', 'k', 'v'))
    mask, ks = (util.keep_mask_t(rec['seed'], rec['site'], (n, H, Lq, Lk), p), util.keep_scale(p)) if p > 0.0 else (None, 1.0)
    do = rec['dout'].float() if not forward else torch.zeros(n, Lq, q.shape[-1])
    case = Case(q, k, v, do, H, mask, ks)
    if forward:
        lse = got['lse'].reshape(n, H, Lq, 2)
        dev = dict(out=got['out'].reshape(n, Lq, -1), mx=lse[..., 0], inv=lse[..., 1], map=got['probs'].reshape(n, H, Lq, Lk) if 'probs' in got else None)
        figures = ('out', 'map', 'mx', 'inv')
    else:
        dev = dict(dq=got['dq'].reshape(n, Lq, -1), dk=got['dk'].reshape(n, Lk, -1), dv=got['dv'].reshape(n, Lk, -1))
        figures = ('dq', 'dk', 'dv')
    figs, bad = check(case, dev, rec['mode'], rec['planes'], figures)
    return figs, bad, magnitude(q, k, H)


def dropout_mask(geom, p, site, seed):
    n, H, Lq, Lk, _ = geom
    return util.keep_mask_t(seed, site, (n, H, Lq, Lk), p), util.keep_scale(p)
