"""The non-MFMA kernels of csrc/ln_bwd.hip, guard.hip, loss.hip and glue.hip against fp64, in the forms hftt_hip/engine.py launches them, under the rounding-model
criteria of tests/elementwise_emul.py (derivations there; tests/test_elementwise_emul_bound.py shows on the CPU what they resolve).

LayerNorm backward over every branch of the hftt_ln_bwd dispatcher (the unaligned fallbacks through views offset by one element) x three
input families x ragged M and one M past the first grid pass; hftt_ln_bwd_reduce on a synthetic workspace with beta; Adam with grad_scale,
non-zero state, log-uniform gradients and n past one grid pass; both loss kernels with their grid-stride loops, grad_scale, null gradient
pointers and the ORDER of loss_out; the column sum in the engine's call shape (bf16 input, beta, ld > n); the time-embedding backward with
accumulate = 1 and a null dym; the heads split at saturating logits.  The fp64 references are evaluated on the device, from the same
rounded inputs the kernel reads."""
import ctypes as C

import pytest
import torch

import util
import elementwise_emul as E

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


def _lib():
    from hftt_hip import _capi
    return _capi, _capi.lib()


def _st(dev):
    return torch.cuda.current_stream(dev).cuda_stream


GUARD = -8192.0            # (exact in bf16 too)


def _guarded(dev, numel, dtype, off, fill=None):
    """a flat buffer with one guard element after (and `off` before) the view the kernel gets: off = 1 makes the view's address odd in
    elements (not 16-byte aligned).  Returns (buffer, view)."""
    buf = torch.full((numel + off + 1,), GUARD, device=dev, dtype=dtype)
    view = buf[off:off + numel]
    if fill is not None:
        view.copy_(fill.reshape(-1).to(dtype))
    return buf, view


def _guards_intact(buf, off):
    return float(buf[-1]) == GUARD and (off == 0 or float(buf[0]) == GUARD)


# ================================================================================================ LayerNorm backward
@pytest.mark.parametrize('family', E.LN_FAMILIES)
@pytest.mark.parametrize('branch', list(E.LN_BRANCHES))
def test_ln_bwd_branch_against_fp64(dev, branch, family):
    capi, L = _lib()
    spec = E.LN_BRANCHES[branch]
    N, off = spec['N'], spec['off']
    for M in spec['Ms']:
        c = E.ln_inputs(branch, family, M)
        p = E.LN_DROP['p'] if spec['drop'] else 0.0
        mask = E.ln_mask(M, N, p, E.LN_DROP['site'], E.LN_DROP['seed']) if spec['drop'] else None
        cd = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in c.items()}
        ref = E.ln_bwd_ref(cd, mask, p)
        dt = lambda bf: BF16 if bf else torch.float32      # noqa: E731
        dyb, dyv = _guarded(dev, M * N, dt(spec['dy_bf']), off, c['dy'])
        rb, rv = _guarded(dev, M * N, dt(spec['r_bf']), off, c['r'])
        drb, drv = _guarded(dev, M * N, dt(spec['dr_bf']), off)
        ddb, ddv = _guarded(dev, M * N, dt(spec['drop'] == 'bf16'), off)
        n_wg = L.hftt_ln_bwd_wgs(M)
        ws = torch.full((n_wg * 2 * N + 1,), GUARD, device=dev)
        d = capi.LnBwdDesc()
        d.M, d.N = M, N
        d.dy, d.r, d.mean, d.rstd, d.gamma = dyv.data_ptr(), rv.data_ptr(), cd['mean'].data_ptr(), cd['rstd'].data_ptr(), cd['gamma'].data_ptr()
        d.dr, d.dr_drop = drv.data_ptr(), (ddv.data_ptr() if spec['drop'] else 0)
        d.drop_p, d.drop_site, d.drop_seed = p, E.LN_DROP['site'], E.LN_DROP['seed']
        d.ws, d.drop_bf16 = ws.data_ptr(), 1 if spec['drop'] == 'bf16' else 0
        d.io_flags = (1 if spec['dy_bf'] else 0) | (2 if spec['dr_bf'] else 0) | (4 if spec['r_bf'] else 0)
        assert (dyv.data_ptr() % 16 != 0) == bool(off)
        capi.check(L.hftt_ln_bwd(C.byref(d), _st(dev)), 'ln_bwd')
        dg = torch.empty(N, device=dev); db = torch.empty(N, device=dev)
        capi.check(L.hftt_ln_bwd_reduce(ws.data_ptr(), n_wg, N, dg.data_ptr(), db.data_ptr(), 0.0, _st(dev)), 'ln_bwd_reduce')
        got = dict(dr=drv.view(M, N), dg=dg, db=db)
        if spec['drop']:
            got['drd'] = ddv.view(M, N)
        bad = E.ln_bwd_check(got, ref, dr_bf=spec['dr_bf'], drop=spec['drop'], mask=mask, p=p)
        assert not bad, (branch, family, M, bad)
        assert _guards_intact(drb, off) and _guards_intact(ddb, off) and float(ws[-1]) == GUARD, (branch, family, M)
        assert _guards_intact(dyb, off) and _guards_intact(rb, off)


@pytest.mark.parametrize('N', [64, 256])
def test_ln_bwd_reduce_on_a_synthetic_workspace(dev, N):
    capi, L = _lib()
    g = torch.Generator().manual_seed(N)
    for n_wg in E.LN_RED_N_WG:
        ws = (torch.randn(n_wg, 2 * N, generator=g) * (10.0 ** (-6 * torch.rand(2 * N, generator=g)))[None]).to(dev)
        for beta in (0.0, 1.0):
            dst = torch.randn(2 * N, generator=g).to(dev)
            ref, bound = E.ln_reduce_bound(ws.double(), dst.double(), beta)
            dgam, dbet = dst[:N].clone(), dst[N:].clone()
            capi.check(L.hftt_ln_bwd_reduce(ws.data_ptr(), n_wg, N, dgam.data_ptr(), dbet.data_ptr(), beta, _st(dev)), 'ln_bwd_reduce')
            bad = E.violations('reduce', torch.cat([dgam, dbet]), ref, bound)
            assert not bad, (N, n_wg, beta, bad)


# ================================================================================================ Adam
@pytest.mark.parametrize('n', E.ADAM_N)
def test_adam_step_against_fp64(dev, n):
    """twenty steps per case; every step is held to the fp64 step from the device's own previous state (m, v, and p: where p starts at 0,
    p is the update itself), and the elements with g = 0 and zero state keep p to the bit"""
    from hftt_hip import ops
    for (n_, gs, eps, s0) in [c for c in E.adam_cases() if c[0] == n]:
        seed = n % 1000 + int(gs * 12) + s0
        p, m, v = (t.to(dev) for t in E.adam_state(n, seed))
        p0, idle = p.clone(), E.adam_idle(n).to(dev)
        for k in range(E.ADAM_STEPS):
            g = E.adam_grad(n, seed, k).to(dev)
            ref = E.adam_ref(p, g, m, v, s0 + k, eps=eps, grad_scale=gs)
            ops.adam_step(p, g, m, v, s0 + k, lr=E.ADAM_LR, beta1=E.ADAM_B1, beta2=E.ADAM_B2, eps=eps, grad_scale=gs)
            bad = E.adam_check(p, m, v, ref)
            assert not bad, (n, gs, eps, s0 + k, bad)
        assert torch.equal(p[idle], p0[idle]) and float(m[idle].abs().sum()) == 0.0 and float(v[idle].abs().sum()) == 0.0


# ================================================================================================ loss
def _loss_launch(dev, capi, L, c, kernel, gs, grads=True):
    """returns out[9], d_prob[6], d_vel[2] (None without grads) and the buffers whose guards the caller checks"""
    n, V = c['n'], c['V']
    off = 1 if kernel == 'general_unaligned' else 0
    d = capi.LossDesc()
    d.n, d.V = n, V
    keep = []
    dp = [q.to(dev).contiguous() for q in c['probs']]
    gp = [torch.full((n,), float('nan'), device=dev) for _ in range(6)]
    vel = [_guarded(dev, n * V, torch.float32, off, t) for t in c['vel']]
    gv = [_guarded(dev, n * V, torch.float32, off) for _ in range(2)]
    for i in range(6):
        d.prob[i], d.d_prob[i] = dp[i].data_ptr(), (gp[i].data_ptr() if grads else None)
    for i in range(2):
        d.vel[i], d.d_vel[i] = vel[i][1].data_ptr(), (gv[i][1].data_ptr() if grads else None)
    labs = (c['lo'].to(dev), c['lf'].to(dev), c['lm'].to(dev), c['lv'].to(dev))
    d.label_onset, d.label_offset, d.label_mpe, d.label_velocity = (t.data_ptr() for t in labs)
    d.weight_A, d.weight_B, d.grad_scale = E.LOSS_W[0], E.LOSS_W[1], gs
    out = torch.zeros(16, device=dev)
    ws = torch.empty(L.hftt_loss_ws_bytes(n) // 4 + 16, device=dev)
    d.loss_out, d.ws = out.data_ptr(), ws.data_ptr()
    keep += [dp, labs, ws]
    capi.check(L.hftt_loss(C.byref(d), _st(dev)), 'loss')
    torch.cuda.synchronize(dev)
    return out[:9].clone(), gp, [b[1].view(n, V) for b in gv], [b[0] for b in gv], off


@pytest.mark.parametrize('kernel,V,n,gs', E.LOSS_CASES)
def test_loss_kernels_against_fp64(dev, kernel, V, n, gs):
    capi, L = _lib()
    c = E.loss_inputs(V, n)
    cd = dict(c, probs=[t.to(dev) for t in c['probs']], vel=[t.to(dev) for t in c['vel']], lo=c['lo'].to(dev), lf=c['lf'].to(dev),
              lm=c['lm'].to(dev), lv=c['lv'].to(dev))
    ref = E.loss_ref(cd, gs)
    out, gp, gv, gv_bufs, off = _loss_launch(dev, capi, L, c, kernel, gs)
    assert (gv[0].data_ptr() % 16 != 0) == (kernel == 'general_unaligned')
    bad = E.loss_check(out, gp, gv, ref)
    assert not bad, (kernel, V, n, gs, bad)
    assert all(_guards_intact(b, off) for b in gv_bufs)
    assert all(bool(torch.isfinite(t).all()) for t in gp + gv)


@pytest.mark.parametrize('kernel,V,n', [('v4', 128, 261), ('general_unaligned', 128, 130), ('general', 255, 130)])
def test_loss_with_null_gradient_pointers(dev, kernel, V, n):
    """the validation loss: every d_* NULL.  The nine values are those of the run with gradients, bit for bit, and nothing is written into
    gradient buffers that were not passed"""
    capi, L = _lib()
    c = E.loss_inputs(V, n)
    full, _, _, _, _ = _loss_launch(dev, capi, L, c, kernel, 0.25)
    out, gp, gv, gv_bufs, off = _loss_launch(dev, capi, L, c, kernel, 0.25, grads=False)
    assert torch.equal(out, full)
    assert all(bool(torch.isnan(t).all()) for t in gp)
    assert all(bool((b == GUARD).all()) for b in gv_bufs)


# ================================================================================================ column sum
@pytest.mark.parametrize('rows,n,pad,bf,beta', E.COLSUM_CASES)
def test_colsum_against_fp64(dev, rows, n, pad, bf, beta):
    from hftt_hip import ops
    c = E.colsum_inputs(rows, n, pad, bf)
    buf = c['buf'].to(dev).to(BF16 if bf else torch.float32)
    x = buf[:, :n]
    assert x.stride(0) == n + pad
    cd = dict(c, x=x.float(), out0=c['out0'].to(dev))
    ref, bound = E.colsum_ref(cd, beta)
    outb, out = _guarded(dev, n, torch.float32, 0, c['out0'])
    ops.colsum(x, beta=beta, out=out)
    bad = E.violations('colsum', out, ref, bound)
    assert not bad, (rows, n, pad, bf, beta, bad)
    assert _guards_intact(outb, 0)


# ================================================================================================ time embedding
@pytest.mark.parametrize('shape,half,p,with_dym', E.TE_CASES)
def test_time_embed_bwd_accumulates(dev, shape, half, p, with_dym):
    """the engine's call: accumulate = 1 onto a non-zero dx (fp32, and the all-bf16 stream with TE_M_BF16), dym NULL when dropout is off"""
    capi, L = _lib()
    B, T, N, d = shape
    c = E.te_inputs(shape, half)
    mask = util.keep_mask_t(E.TE_DROP['seed'], E.TE_DROP['site'], (B * N, T, d), p) if p > 0 else None
    cd = dict(c, dy=c['dy'].to(dev), dx0=c['dx0'].to(dev))
    ref = E.te_bwd_ref(cd, mask, p, half)
    dt = BF16 if half else torch.float32
    dy = c['dy'].to(dev).to(dt)
    dxb, dx = _guarded(dev, B * T * N * d, dt, 0, c['dx0'])
    dymb, dym = _guarded(dev, B * T * N * d, dt, 0)
    fl = (capi.TE_X_BF16 | capi.TE_Y_BF16 | capi.TE_M_BF16) if half else 0
    capi.check(L.hftt_time_embed_bwd(dy.data_ptr(), dx.data_ptr(), dym.data_ptr() if with_dym else None, B, T, N, d, c['scale'], p,
                                     E.TE_DROP['site'], E.TE_DROP['seed'], 1, fl, _st(dev)), 'te_bwd')
    bad = E.te_bwd_check(dx.view(B * T, N, d), dym.view(B * N, T, d) if with_dym else None, ref)
    assert not bad, (shape, half, p, with_dym, bad)
    assert _guards_intact(dxb, 0) and _guards_intact(dymb, 0)
    if not with_dym:
        assert bool((dymb == GUARD).all())
    elif mask is not None:
        assert bool(((dym.view(B * N, T, d) == 0) | mask.to(dev)).all())


@pytest.mark.parametrize('half', [False, True])
@pytest.mark.parametrize('p', [0.0, 0.25])
def test_time_embed_forward_at_the_model_shape(dev, p, half):
    """y[(b,n),t,:] = keep * (x[(b,t),n,:] * sqrt(d) + pos[t]) * (256 / thr) at T = 128, N = 88, d = 256: the product, the sum and the keep
    scale are 3 roundings on (|x| sqrt(d) + |pos|) * (256 / thr), + one bf16 rounding of the stored result"""
    capi, L = _lib()
    B, T, N, d = E.TE_SHAPES[1]
    g = torch.Generator().manual_seed(int(p * 100) + half)
    dt = BF16 if half else torch.float32
    x = torch.randn(B * T, N, d, generator=g).to(dt).to(dev)
    pos = torch.randn(T, d, generator=g).to(dev)
    scale = E.f32(d ** 0.5)
    yb, y = _guarded(dev, B * N * T * d, dt, 0)
    fl = (capi.TE_X_BF16 | capi.TE_Y_BF16) if half else 0
    capi.check(L.hftt_time_embed_fwd(x.data_ptr(), pos.data_ptr(), y.data_ptr(), B, T, N, d, scale, p, E.TE_DROP['site'], E.TE_DROP['seed'], fl,
                                     _st(dev)), 'te_fwd')
    xs = x.double().view(B, T, N, d).permute(0, 2, 1, 3).reshape(B * N, T, d) * scale
    mask = (util.keep_mask_t(E.TE_DROP['seed'], E.TE_DROP['site'], (B * N, T, d), p).to(dev).double() if p > 0
            else torch.ones(B * N, T, d, dtype=torch.float64, device=dev))
    ks = util.keep_scale(p)
    ref = (xs + pos.double()[None]) * mask * ks
    bound = 3 * E.U32 * (xs.abs() + pos.double().abs()[None]) * mask * ks
    if half:
        bound = bound * (1 + E.UBF) + E.UBF * ref.abs()
    bad = E.violations('y', y, ref, bound)
    assert not bad, (p, half, bad)
    assert _guards_intact(yb, 0)


# ================================================================================================ heads split
def test_heads_split_at_saturating_logits_feeds_a_finite_loss(dev):
    """logits of +-100 and +-20 in the three sigmoid columns: the posteriors are exactly 0 / 1 or finite, never NaN, and hftt_loss turns them
    into finite values and gradients"""
    capi, L = _lib()
    B, T, N, V = 1, 4, 3, 128
    ldl = 192
    S = B * T * N
    g = torch.Generator().manual_seed(7)
    logits = torch.randn(S, ldl, generator=g) * 2
    sat = torch.tensor([100.0, -100.0, 20.0, -20.0])
    for k in range(3):
        logits[:, V + k] = sat[(torch.arange(S) + k) % 4]
    dl = logits.to(dev)
    o = [torch.full((S,), float('nan'), device=dev) for _ in range(3)] + [torch.full((S, V), float('nan'), device=dev)]
    capi.check(L.hftt_heads_split(dl.data_ptr(), ldl, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), B, T, N, V, 0, _st(dev)), 'heads')
    for k in range(3):
        got = o[k].double().cpu()
        ref = torch.sigmoid(logits[:, V + k].double())
        assert bool(torch.isfinite(got).all()) and bool(((got >= 0) & (got <= 1)).all())
        # 1 / (1 + expf(-x)): expf E.C_EXP, the sum 1, the division E.C_DIV, on a result whose expf argument is exact
        assert not E.violations('sigmoid', got, ref, (E.C_EXP + 1 + E.C_DIV) * E.U32 * ref + E.F32_TINY)
        assert bool((got[logits[:, V + k] == 100.0] == 1.0).all()) and bool((got[logits[:, V + k] == -100.0] == 0.0).all())
    assert torch.equal(o[3].cpu(), logits[:, :V])
    c = E.loss_inputs(V, S)
    c['probs'] = [o[0].cpu(), o[1].cpu(), o[2].cpu()] * 2
    c['vel'] = [o[3].cpu(), o[3].cpu()]
    out, gp, gv, _, _ = _loss_launch(dev, capi, L, c, 'v4', 1.0)
    assert bool(torch.isfinite(out).all()) and all(bool(torch.isfinite(t).all()) for t in gp + gv)
    cd = dict(c, probs=[t.to(dev) for t in c['probs']], vel=[t.to(dev) for t in c['vel']], lo=c['lo'].to(dev), lf=c['lf'].to(dev),
              lm=c['lm'].to(dev), lv=c['lv'].to(dev))
    assert not E.loss_check(out, gp, gv, E.loss_ref(cd, 1.0))
