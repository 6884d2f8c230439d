"""The MFMA kernels in the layouts hftt_hip/plan.py launches them in (test infrastructure for tests/test_engine_layouts_gpu.py).

Three pieces:

  * `Plane`: the arena.  Every operand and result of a case is a strided view into a flat device buffer of (rows + 2) x ld elements: one
    guard row in front, one behind, and the gap columns of every row.  Output planes are filled with SENT (-8192.0, exact in bf16 too); after
    the launch every element outside the views handed out must still be SENT to the bit and every element inside must differ from it.  Input
    planes are filled with NaN: a NaN in a result means a value outside the operand's footprint took part in arithmetic.  In-place and
    accumulating forms: the pre-fill of the view is data and the reference starts from a copy of it.
  * the case tables (`TN_CASES`, `NT_CASES`, `SL_CASES`, `FFN_CASES`, `OFFN_CASES`, `ATTN_CASES`) and one `build_*` / `run` pair per entry point.
    `build_*` allocates the planes and fills the `_capi` descriptor exactly as the plan builder does (leading dimensions, column offsets,
    segments, aliasing, flags); with dry=True it launches nothing at all (no weight packing either) -- that is what the coverage pin uses.
    twin=True builds the SAME product on contiguous, non-aliased operands: a layout must not change the arithmetic.
  * `signature`: a descriptor reduced to its layout -- entry point, precision / storage flags, which leading dimensions exceed their width,
    which output aliases an input, segment structure, K_out < K, beta / res_mod / add_mod, a zero sequence stride.  A descriptor with no such
    feature is PLAIN: the layout hftt_hip/ops.py hard-codes, which the wrappers' own tests hold (tests/test_x3_gpu.py, test_kernels_gpu.py,
    test_strip_gpu.py, test_bf16_ulp_gpu.py).

Bounds: none is new.  Each case is held to the bound its kernel and mode carry in those files; the table below each runner names the line."""
import ctypes as C
import math

import torch

import util                                   # noqa: F401  (puts the package on sys.path)
from util import keep_mask_t, keep_scale

SENT = -8192.0            # (exact in bf16 too: the sentinel of tests/test_elementwise_fp64_gpu.py)
NAN = float('nan')
BF = torch.bfloat16
F32 = torch.float32
F64 = torch.float64

TOL_X3 = {2: 4e-6, 4: 6e-5}          # tests/test_x3_gpu.py TOL
TOL_K = {3: 3e-6, 1: 2e-2}           # tests/test_kernels_gpu.py TOL


def _capi():
    from hftt_hip import _capi
    return _capi


def _ops():
    from hftt_hip import ops
    return ops


def stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


class Plane:
    """(rows + 2) x ld elements: guard row, the rows, guard row.  block() hands out a view and adds it to the footprint."""

    def __init__(self, dev, rows, ld, dtype=F32, fill=SENT):
        self.rows, self.ld, self.fill = rows, ld, fill
        self.buf = torch.full((rows + 2, ld), fill, dtype=dtype, device=dev)
        self.foot = torch.zeros(rows + 2, ld, dtype=torch.bool, device=dev)

    def block(self, col0, width, data=None, rows=None):
        r = self.rows if rows is None else rows
        assert col0 + width <= self.ld and r <= self.rows
        v = self.buf[1:1 + r, col0:col0 + width]
        self.foot[1:1 + r, col0:col0 + width] = True
        if data is not None:
            v.copy_(data.reshape(r, width).to(v.dtype))
        return v

    def guards_intact(self):
        return bool((self.buf[~self.foot] == self.fill).all())

    def written(self):
        return bool((self.buf[self.foot] != self.fill).all())


def out_plane(dev, rows, width, ld=None, dtype=F32, col0=0, data=None):
    p = Plane(dev, rows, ld or width, dtype, SENT)
    return p, p.block(col0, width, data)


def in_plane(dev, data, ld=None, col0=0, dtype=None):
    rows, width = data.shape
    p = Plane(dev, rows, ld or width, dtype or data.dtype, NAN)
    return p, p.block(col0, width, data)


def vec_plane(dev, n, dtype=F32, data=None):
    """a vector result with a guard vector in front and behind"""
    return out_plane(dev, 1, n, dtype=dtype, data=data)


def check_planes(ctx):
    """the three layout assertions of every case: guards intact, footprint written, no NaN from a gap"""
    for name, p in ctx['out_planes'].items():
        assert p.guards_intact(), '%s: an element outside the documented footprint was overwritten' % name
        assert p.written(), '%s: an element of the footprint was not written' % name
    for name, t in ctx['results'].items():
        assert bool(torch.isfinite(t.float()).all()), '%s: a NaN / Inf -- a value from a gap or a guard row reached the result' % name


def rel_err(a, b):
    a, b = a.double(), b.double()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def max_err(a, b):
    return (a.double() - b.double()).abs().max().item()


def bf16_check(name, dev_out, ref, absref, excess, ident=None, row_ident=None):
    """the criterion of tests/test_bf16_ulp_gpu.py::_check, figures returned for the report"""
    import bf16_emul as E
    dev_out, ref, absref = dev_out.cpu(), ref.cpu(), absref.cpu()
    exc = E.excess(dev_out, ref, absref)
    _, frac = E.ulp_stats(dev_out, ref)
    row = E.row_ident_min(dev_out, ref)
    print('%-40s identical %.5f  worst row %.4f  excess %.1f (<= %d)' % (name, frac, row, exc, excess))
    assert frac >= (E.IDENT_STREAM if ident is None else ident), (name, frac)
    assert row >= (E.ROW_IDENT_STREAM if row_ident is None else row_ident), (name, row)
    assert exc <= excess, (name, exc)


def _report(name, what, err, bound):
    print('%-44s %-8s %.3e  (bound %.3e)' % (name, what, err, bound))
    return err < bound


# ============================================================================================================ TN GEMM
# modes: npass and how dY / X are stored there.  'x3': npass 4, fp32 operands, gradient-sized dY (test_x3_gpu.py::test_gemm_tn: max error over
# sqrt(M) max|dY| below 3 TOL[4], bias 1e-5, out_scale 0.5).  'parity': npass 3 (test_kernels_gpu.py::test_gemm_tn: the same with TOL[3]).
# 'bf16': npass 1 with the operands the bf16 strip plans store as bf16 (test_kernels_gpu.py::test_gemm_tn_bf16_storage: bf16-exact values, error
# over sqrt(M) below 1e-4, bias 1e-5, out_scale 1).
TN_M = 1000
_HEAD_SEGS = [(0, 16), (16, 1), (17, 1), (18, 1)]            # V = 16 velocity rows, onset, offset, mpe; rows 19 .. 63 of N = NHp in no segment
TN_CASES = {
    # name: N, K, segments (row0, rows), K_out, beta, {mode: (dY bf16, X bf16)}
    'qkv_3seg': dict(N=768, K=256, segs=[(0, 256), (256, 256), (512, 256)], modes={'x3': (0, 0), 'parity': (0, 0), 'bf16': (1, 1)}),
    'cross_kv_2seg': dict(N=512, K=256, segs=[(0, 256), (256, 256)], modes={'x3': (0, 0), 'parity': (0, 0), 'bf16': (1, 1)}),
    'cross_kv_6seg': dict(N=1536, K=256, segs=[(i * 256, 256) for i in range(6)], modes={'x3': (0, 0)}),
    'qkv_3seg_d64': dict(N=192, K=64, segs=[(0, 64), (64, 64), (128, 64)], modes={'x3': (0, 0), 'parity': (0, 0), 'bf16': (1, 1)}),
    'cross_kv_2seg_d64': dict(N=128, K=64, segs=[(0, 64), (64, 64)], modes={'x3': (0, 0), 'parity': (0, 0), 'bf16': (1, 1)}),
    'heads': dict(N=64, K=256, segs=_HEAD_SEGS, modes={'x3': (0, 0), 'parity': (0, 0), 'bf16': (0, 1)}),
    'heads_d64': dict(N=64, K=64, segs=_HEAD_SEGS, modes={'x3': (0, 0), 'parity': (0, 0), 'bf16': (0, 1)}),
    'embed_fold_k_out': dict(N=256, K=96, K_out=65, segs=[(0, 256)], modes={'x3': (0, 0), 'parity': (0, 0), 'bf16': (1, 0)}),
    'embed_fold_k_out_d64': dict(N=64, K=96, K_out=65, segs=[(0, 64)], modes={'x3': (0, 0), 'parity': (0, 0), 'bf16': (1, 0)}),
    # no plan passes beta today; the header documents it (accumulate into up to 8 segments), so one case holds it on random prior contents
    'qkv_3seg_beta1': dict(N=768, K=256, segs=[(0, 256), (256, 256), (512, 256)], beta=1.0, modes={'x3': (0, 0)}),
}
TN_NPASS = {'x3': 4, 'parity': 3, 'bf16': 1}


def build_tn(dev, case, mode, twin=False, dry=False):
    capi = _capi()
    c = TN_CASES[case]
    M, N, K = TN_M, c['N'], c['K']
    dy_bf, x_bf = c['modes'][mode]
    K_out = K if twin else c.get('K_out', K)
    beta = 0.0 if twin else c.get('beta', 0.0)
    segs = [(0, N)] if twin else c['segs']
    out_scale = 1.0 if mode == 'bf16' else 0.5
    g = torch.Generator().manual_seed(N * 7 + K + len(c['segs']))
    dY = torch.randn(M, N, generator=g) * (1e-6 if mode == 'x3' else 1.0)
    X = torch.randn(M, K, generator=g)
    if mode == 'bf16':
        dY, X = dY.to(BF).float(), X.to(BF).float()
    dY, X = dY.to(dev), X.to(dev)
    pdy, vdy = in_plane(dev, dY, dtype=BF if dy_bf else F32)
    px, vx = in_plane(dev, X, dtype=BF if x_bf else F32)
    mag = out_scale * math.sqrt(M) * float(dY.abs().max())
    d = capi.GemmTnDesc()
    d.M, d.N, d.K, d.npass = M, N, K, TN_NPASS[mode]
    d.dY, d.lddy, d.X, d.ldx = vdy.data_ptr(), N, vx.data_ptr(), K
    d.out_scale, d.beta, d.n_seg, d.K_out = out_scale, beta, len(segs), K_out
    d.io_flags = (1 if dy_bf else 0) | (2 if x_bf else 0)
    planes, dws, dbs, priors = {}, [], [], []
    # the destinations are the caller's: here in reverse order of the segments, each between its own guards
    for i, (r0, rows) in reversed(list(enumerate(segs))):
        pw = torch.randn(rows, K_out, generator=g).to(dev) * mag if beta else None
        pb = torch.randn(rows, generator=g).to(dev) * mag if beta else None
        planes['dw%d' % i], vw = out_plane(dev, rows, K_out, data=pw)
        planes['db%d' % i], vb = vec_plane(dev, rows, data=pb)
        d.seg_row0[i], d.seg_rows[i], d.seg_dw[i], d.seg_db[i] = r0, rows, vw.data_ptr(), vb.data_ptr()
        dws.insert(0, vw); dbs.insert(0, vb); priors.insert(0, (pw, pb))
    ws = None
    if not dry:
        wsb = capi.lib().hftt_gemm_tn_ws_bytes(M, N, K)
        ws = torch.empty(wsb // 4 + 16, device=dev)
        d.ws, d.ws_bytes = ws.data_ptr(), ws.numel() * 4
    results = {'dw%d' % i: v for i, v in enumerate(dws)}
    results.update({'db%d' % i: v[0] for i, v in enumerate(dbs)})
    return dict(kind='gemm_tn', desc=d, descs=[('gemm_tn', d)], keep=(ws, pdy, px), out_planes=planes, results=results, dws=dws, dbs=dbs,
                priors=priors, segs=segs, dY=vdy, X=vx, mag=mag, mode=mode, case=case, K_out=K_out, out_scale=out_scale, beta=beta)


def launch_tn(dev, ctx):
    capi = _capi()
    capi.check(capi.lib().hftt_gemm_tn(C.byref(ctx['desc']), stream(dev)), 'gemm_tn')


def check_tn(ctx, figures):
    mode, name = ctx['mode'], 'tn %s/%s' % (ctx['case'], ctx['mode'])
    dY, X = ctx['dY'].double(), ctx['X'].double()
    ref = ctx['out_scale'] * dY.T @ X
    refb = ctx['out_scale'] * dY.sum(0)
    # the inherited tests' scale: sqrt(M) max|dY| for the gradient-sized dY of the x3 test, sqrt(M) for the unit-variance dY of the other two
    scale = ctx['mag'] / ctx['out_scale'] if mode == 'x3' else math.sqrt(TN_M)
    wb = {'x3': 3 * TOL_X3[4], 'parity': 3 * TOL_K[3], 'bf16': 1e-4}[mode]
    ok, ew, eb = True, 0.0, 0.0
    for (r0, rows), vw, vb, (pw, pb) in zip(ctx['segs'], ctx['dws'], ctx['dbs'], ctx['priors']):
        rw, rb = ref[r0:r0 + rows, :ctx['K_out']], refb[r0:r0 + rows]
        if ctx['beta']:
            rw, rb = rw + ctx['beta'] * pw.double(), rb + ctx['beta'] * pb.double()
        ew, eb = max(ew, max_err(vw, rw) / scale), max(eb, max_err(vb[0], rb) / scale)
    ok &= _report(name, 'dW', ew, wb)
    ok &= _report(name, 'db', eb, 1e-5)
    figures[name] = [('dW', ew, wb), ('db', eb, 1e-5)]
    assert ok, name


def twin_equal_tn(ctx, tw):
    full_w, full_b = tw['dws'][0], tw['dbs'][0][0]
    for (r0, rows), vw, vb, (pw, pb) in zip(ctx['segs'], ctx['dws'], ctx['dbs'], ctx['priors']):
        ew, eb = full_w[r0:r0 + rows, :ctx['K_out']], full_b[r0:r0 + rows]
        if ctx['beta']:                            # dst * 1 + v: one rounding, the fp32 sum
            ew, eb = pw + ew, pb + eb
        assert torch.equal(vw, ew) and torch.equal(vb[0], eb), 'tn %s: the segment layout changed the arithmetic' % ctx['case']


# ============================================================================================================ block NT GEMM
# modes: 'x3f' npass 2 (forward products), 'x3b' npass 4 (products with a gradient), 'parity' npass 3, 'bf16' npass 1 with the storage flags of
# the bf16 plans.  Bounds: rel_err below TOL (test_x3_gpu.py::test_gemm_nt_plain / _epilogues, test_kernels_gpu.py the same); LayerNorm form:
# pre-LN sum below TOL, output / mean / rstd below 1e-4; bf16 (test_gemm_nt_bf16_storage, bf16-exact inputs): fp32 C 1e-5, bf16 C 5e-3.
NT_NPASS = {'x3f': 2, 'x3b': 4, 'parity': 3, 'bf16': 1}
NT_CASES = {
    # io per mode: (A bf16, C bf16)
    'heads_ldc': dict(M=300, N=131, K=256, ldc=192, bias=1, modes={'x3f': (0, 0), 'parity': (0, 0), 'bf16': (1, 0)}),
    'heads_ldc_d64': dict(M=300, N=19, K=64, ldc=64, bias=1, modes={'x3f': (0, 0), 'parity': (0, 0), 'bf16': (1, 0)}),
    'gpos_in_place': dict(M=88, N=256, K=256, inplace=1, modes={'x3b': (0, 0), 'parity': (0, 0), 'bf16': (0, 0)}),
    'gpos_in_place_d64': dict(M=88, N=64, K=64, inplace=1, modes={'x3b': (0, 0), 'parity': (0, 0), 'bf16': (0, 0)}),
    'embed_add_table': dict(M=300, N=256, K=96, bias=1, out_scale=16.0, add_mod=32, drop=0.1, modes={'x3f': (0, 0), 'parity': (0, 0), 'bf16': (0, 1)}),
    'embed_add_table_d64': dict(M=300, N=64, K=96, bias=1, out_scale=8.0, add_mod=32, drop=0.1, modes={'x3f': (0, 0), 'parity': (0, 0), 'bf16': (0, 1)}),
    'cross0_res_mod_ln': dict(M=300, N=256, K=256, bias=1, res_mod=88, ln=1, drop=0.1, modes={'x3f': (0, 0), 'parity': (0, 0)}),
    'cross0_res_mod_ln_d64': dict(M=300, N=64, K=64, bias=1, res_mod=88, ln=1, drop=0.1, modes={'x3f': (0, 0), 'parity': (0, 0)}),
    'kv_t_in_place': dict(M=300, N=256, K=512, inplace=1, modes={'x3b': (0, 0), 'parity': (0, 0)}),
    'kv_t_in_place_d64': dict(M=300, N=64, K=128, inplace=1, modes={'x3b': (0, 0), 'parity': (0, 0)}),
    'ffn_gate_ldg': dict(M=300, N=512, K=256, gate=1, gate_scale=1.25, modes={'x3b': (0, 0), 'parity': (0, 0)}),
}
NT_SITE, NT_SEED = 5, 77


def build_nt(dev, case, mode, twin=False, dry=False):
    capi, c = _capi(), NT_CASES[case]
    M, N, K = c['M'], c['N'], c['K']
    a_bf, c_bf = c['modes'][mode]
    npass = NT_NPASS[mode]
    ldc = N if twin else c.get('ldc', N)
    g = torch.Generator().manual_seed(M + N + K)
    rnd = lambda *s: torch.randn(*s, generator=g)                       # noqa: E731
    A, W = rnd(M, K), rnd(N, K) / math.sqrt(K)
    bias = rnd(N) if c.get('bias') else None
    table = rnd(c['add_mod'], N) if c.get('add_mod') else None
    res = rnd(c.get('res_mod') or M, N) if (c.get('res_mod') or c.get('inplace')) else None
    gate = rnd(M, N) if c.get('gate') else None
    gam, bet = (rnd(N), rnd(N)) if c.get('ln') else (None, None)
    if mode == 'bf16':
        A = A.to(BF).float()
    A = A.to(dev)
    pa, va = in_plane(dev, A, dtype=BF if a_bf else F32)
    planes = {}
    d = capi.GemmNtDesc()
    d.M, d.N, d.K, d.npass = M, N, K, npass
    d.A, d.lda = va.data_ptr(), K
    d.io_flags = (1 if a_bf else 0) | (2 if c_bf else 0)
    keep = [pa]
    if bias is not None:
        bias = bias.to(dev); d.bias = bias.data_ptr()
    d.act, d.out_scale = 0, c.get('out_scale', 1.0)
    if table is not None:
        pt, table_v = in_plane(dev, table.to(dev)); keep.append(pt)
        d.add_table, d.add_mod = table_v.data_ptr(), c['add_mod']
    if gate is not None:
        pg, gate_v = in_plane(dev, gate.to(dev)); keep.append(pg)
        d.gate, d.ldg, d.gate_scale = gate_v.data_ptr(), N, c['gate_scale']
    p = c.get('drop', 0.0)
    d.drop_p, d.drop_site, d.drop_seed = p, NT_SITE, NT_SEED
    in_place = bool(c.get('inplace')) and not twin
    res_d = res.to(dev) if res is not None else None
    planes['C'], vc = out_plane(dev, M, N, ld=ldc, dtype=BF if c_bf else F32, data=res_d if in_place else None)
    d.C, d.ldc = vc.data_ptr(), ldc
    if res is not None:
        if in_place:
            d.residual = vc.data_ptr()
        else:
            pr, vr = in_plane(dev, res_d); keep.append(pr)
            d.residual = vr.data_ptr()
        d.ldr, d.res_mod = N, (c.get('res_mod') or M)
    results = {'C': vc}
    if gam is not None:
        gam, bet = gam.to(dev), bet.to(dev)
        planes['pre'], vpre = out_plane(dev, M, N)
        planes['mean'], vm = vec_plane(dev, M)
        planes['rstd'], vs = vec_plane(dev, M)
        d.ln_gamma, d.ln_beta, d.pre_ln_out, d.ln_mean, d.ln_rstd = gam.data_ptr(), bet.data_ptr(), vpre.data_ptr(), vm.data_ptr(), vs.data_ptr()
        results.update(pre=vpre, mean=vm[0], rstd=vs[0])
    Wd = W.to(dev)
    if not dry:
        wp = _ops().prepare_weight(Wd, npass)
        d.W = wp.data_ptr()
        if npass in (2, 4):
            d.W_lo = wp[1].data_ptr()
        keep.append(wp)
    return dict(kind='gemm_nt', desc=d, descs=[('gemm_nt', d)], keep=keep, out_planes=planes, results=results, case=case, mode=mode, c=c, A=va, W=Wd, bias=bias,
                table=table.to(dev) if table is not None else None, gate=gate.to(dev) if gate is not None else None, res=res_d, gam=gam, bet=bet, c_bf=c_bf)


def launch_nt(dev, ctx):
    capi = _capi()
    capi.check(capi.lib().hftt_gemm_nt(C.byref(ctx['desc']), stream(dev)), 'gemm_nt')


def _epilogue_ref(lin, c, M, N, table, gate, res, site, seed, dev):
    rows = torch.arange(M, device=dev)
    v = lin * c.get('out_scale', 1.0)
    if table is not None:
        v = v + table.double()[rows % c['add_mod']]
    if gate is not None:
        v = torch.where(gate.double() > 0, v * c['gate_scale'], torch.zeros((), dtype=F64, device=dev))
    if c.get('drop'):
        v = v * keep_mask_t(seed, site, (M, N), c['drop']).to(dev).double() * keep_scale(c['drop'])
    if res is not None:
        v = v + res.double()[rows % (c.get('res_mod') or M)]
    return v


def _ln_ref(r, gam, bet):
    return (torch.nn.functional.layer_norm(r, (r.shape[1],), gam.double(), bet.double(), 1e-5), r.mean(1),
            1.0 / torch.sqrt(r.var(1, unbiased=False) + 1e-5))


def check_nt(ctx, figures):
    c, mode, name = ctx['c'], ctx['mode'], 'nt %s/%s' % (ctx['case'], ctx['mode'])
    M, N = c['M'], c['N']
    dev = ctx['A'].device
    W = ctx['W'].to(BF).double() if mode == 'bf16' else ctx['W'].double()
    lin = ctx['A'].double() @ W.T
    if ctx['bias'] is not None:
        lin = lin + ctx['bias'].double()
    r = _epilogue_ref(lin, c, M, N, ctx['table'], ctx['gate'], ctx['res'], NT_SITE, NT_SEED, dev)
    tol = (5e-3 if ctx['c_bf'] else 1e-5) if mode == 'bf16' else (TOL_X3[NT_NPASS[mode]] if mode.startswith('x3') else TOL_K[3])
    res = ctx['results']
    figs = []
    if c.get('ln'):
        y, mean, rstd = _ln_ref(r, ctx['gam'], ctx['bet'])
        figs = [('pre', rel_err(res['pre'], r), tol), ('C', rel_err(res['C'], y), 1e-4), ('mean', rel_err(res['mean'], mean), 1e-4),
                ('rstd', rel_err(res['rstd'], rstd), 1e-4)]
    else:
        figs = [('C', rel_err(res['C'], r), tol)]
    figures[name] = figs
    assert all([_report(name, *f) for f in figs]), name


def twin_equal(ctx, tw):
    for k, v in ctx['results'].items():
        assert torch.equal(v, tw['results'][k]), '%s %s: %s differs from the launch on contiguous, non-aliased operands' % (ctx['kind'], ctx['case'], k)


# ============================================================================================================ strip linear
# families: 'x3' (csrc/x3_strip.hip, fp32 tensors; forward products fp16 halves, backward bf16 halves), 'x3s' (d = 64, small_strip.h),
# 'bf16' (strip_gemm2.hip / strip_gemm.hip, all-bf16 storage), 'bs' (bs_strip.hip, d = 64).  Bounds: x3 / x3s rel_err below TOL[2] forward and
# TOL[4] backward (test_x3_gpu.py::test_strip_linear, test_small_strip_linear); LayerNorm form: the bf16 pre-LN sum 4e-3, output / mean / rstd
# 1e-4 (test_strip_linear_layernorm); planes: the decoded pair below TOL[2]; bf16 / bs: the rounding model of test_bf16_ulp_gpu.py, excess
# K + 16 (LayerNorm output K + N + 16).
SL_MS = (160, 416)              # one and three 128-token blocks, plus one 32-token strip
SL_CASES = {
    # the merged cross-attention K / V backward: the two K = 768 halves of the [Se, 6d] gradient, the second one in place onto the first
    'kv_all_t0_ldx': dict(N=1, K=3, ldx=6, xcol=0, bwd=1, fams=('x3',)),
    'kv_all_t1_ldx_in_place': dict(N=1, K=3, ldx=6, xcol=3, bwd=1, inplace=1, fams=('x3',)),
    'kv_t_in_place': dict(N=1, K=2, bwd=1, inplace=1, fams=('x3', 'x3s', 'bf16', 'bs')),
    'fc_o_res_mod_ln': dict(N=1, K=1, bias=1, drop=0.1, res_mod=88, ln=1, fams=('x3', 'x3s', 'bf16', 'bs')),
    'kv_all_planes': dict(N=6, K=1, bias=1, planes=1, fams=('x3',)),
    'fc_o_x_drop': dict(N=1, K=1, bwd=1, x_drop=0.1, fams=('x3',)),
}
SL_SITE, SL_SEED = 3, 4242


def planes_decode(t):
    """fp32 slots holding f16-pair planes -> the values (hi + lo) in fp64"""
    h = t.contiguous().view(torch.float16).reshape(t.shape[0], t.shape[1] // 32, 64)
    return (h[..., :32].double() + h[..., 32:].double()).reshape(t.shape)


def build_sl(dev, case, fam, M, twin=False, dry=False):
    capi, ops, c = _capi(), _ops(), SL_CASES[case]
    dm = 64 if fam in ('x3s', 'bs') else 256
    N, K = c['N'] * dm, c['K'] * dm
    x3 = fam in ('x3', 'x3s')
    elem = 4 if c.get('bwd') else 2
    dt = F32 if x3 else BF
    ldx = K if twin else c.get('ldx', c['K']) * dm
    xcol = 0 if twin else c.get('xcol', 0) * dm
    g = torch.Generator().manual_seed(M + N + K)
    rnd = lambda *s: torch.randn(*s, generator=g)                       # noqa: E731
    x, W = rnd(M, K), rnd(N, K) / math.sqrt(K)
    bias = rnd(N).to(dev) if c.get('bias') else None
    res = rnd(c.get('res_mod') or M, N) * (3.0 if c.get('ln') else 1.0) if (c.get('res_mod') or c.get('inplace')) else None
    gam, bet = (rnd(N).to(dev), rnd(N).to(dev)) if c.get('ln') else (None, None)
    if not x3:
        x = x.to(BF).float()
        res = res.to(BF).float() if res is not None else None
    x = x.to(dev)
    px, vx = in_plane(dev, x, ld=ldx, col0=xcol, dtype=dt)
    keep, planes = [px], {}
    d = capi.StripDesc()
    d.M, d.N, d.K = M, N, K
    if x3:
        d.flags = (capi.SL_X3_BF16 if c.get('bwd') else capi.SL_X3_F16) | (capi.SL_PRE_BF16 if c.get('ln') else 0) \
            | (capi.SL_C_F16PAIR if c.get('planes') else 0) | (capi.SL_X_DROP if c.get('x_drop') else 0)
    else:
        d.flags = capi.SL_X_BF16 | capi.SL_C_BF16 | (capi.SL_RES_BF16 if res is not None else 0)
    d.x, d.ldx = vx.data_ptr(), ldx
    d.bias = bias.data_ptr() if bias is not None else 0
    d.out_scale, d.gate_scale = 1.0, 1.0
    p = c.get('x_drop') or c.get('drop', 0.0)
    d.drop_p, d.drop_site, d.drop_seed = p, SL_SITE, SL_SEED
    in_place = bool(c.get('inplace')) and not twin
    res_d = res.to(dev) if res is not None else None
    planes['C'], vc = out_plane(dev, M, N, dtype=dt, data=res_d if in_place else None)
    d.C, d.ldc = vc.data_ptr(), N
    if res is not None:
        if in_place:
            d.residual = vc.data_ptr()
        else:
            pr, vr = in_plane(dev, res_d, dtype=dt); keep.append(pr)
            d.residual = vr.data_ptr()
        d.ldr, d.res_mod = N, c.get('res_mod', 0)
    results = {'C': vc}
    if gam is not None:
        planes['pre'], vpre = out_plane(dev, M, N, dtype=BF)
        planes['mean'], vm = vec_plane(dev, M)
        planes['rstd'], vs = vec_plane(dev, M)
        d.ln_gamma, d.ln_beta, d.pre_ln_out, d.ln_mean, d.ln_rstd = gam.data_ptr(), bet.data_ptr(), vpre.data_ptr(), vm.data_ptr(), vs.data_ptr()
        results.update(pre=vpre, mean=vm[0], rstd=vs[0])
    Wd = W.to(dev)
    if not dry:
        if fam == 'x3':
            wp = ops.x3_strip_pack(Wd, elem, order=1 if (K == 256 and not c.get('ln')) else 0)
        elif fam == 'x3s':
            wp = ops.x3s_pack(Wd, elem)
        elif fam == 'bf16':
            wp = ops.strip_pack(Wd)
        else:
            wp = ops.x3s_pack(Wd, 4)
        d.w = wp.data_ptr(); keep.append(wp)
    return dict(kind='strip_linear', desc=d, descs=[('strip_linear', d)], keep=keep, out_planes=planes, results=results, case=case, mode=fam, c=c, M=M, N=N, K=K,
                x=vx, W=Wd, bias=bias, res=res_d, gam=gam, bet=bet, x3=x3, elem=elem)


def launch_sl(dev, ctx):
    capi = _capi()
    capi.check(capi.lib().hftt_strip_linear(C.byref(ctx['desc']), stream(dev)), 'strip_linear')


def check_sl(ctx, figures):
    c, M, N, K = ctx['c'], ctx['M'], ctx['N'], ctx['K']
    name = 'sl %s/%s/M%d' % (ctx['case'], ctx['mode'], M)
    dev = ctx['x'].device
    res = ctx['results']
    x = ctx['x'].double()
    W = ctx['W'].double() if ctx['x3'] else ctx['W'].to(BF).double()
    if c.get('x_drop'):
        x = x * keep_mask_t(SL_SEED, SL_SITE, (M, K), c['x_drop']).to(dev).double() * keep_scale(c['x_drop'])
    lin = x @ W.T
    ab = x.abs() @ W.abs().T
    if ctx['bias'] is not None:
        lin, ab = lin + ctx['bias'].double(), ab + ctx['bias'].double().abs()
    m = keep_mask_t(SL_SEED, SL_SITE, (M, N), c['drop']).to(dev).double() * keep_scale(c['drop']) if c.get('drop') else 1.0
    r, ab = lin * m, ab * m
    if ctx['res'] is not None:
        rr = ctx['res'].double()[torch.arange(M, device=dev) % (c.get('res_mod') or M)]
        r, ab = r + rr, ab + rr.abs()
    if ctx['x3']:
        tol = TOL_X3[ctx['elem']]
        if c.get('ln'):
            y, mean, rstd = _ln_ref(r, ctx['gam'], ctx['bet'])
            figs = [('pre', rel_err(res['pre'].float(), r), 4e-3), ('C', rel_err(res['C'], y), 1e-4), ('mean', rel_err(res['mean'], mean), 1e-4),
                    ('rstd', rel_err(res['rstd'], rstd), 1e-4)]
        elif c.get('planes'):
            figs = [('C', rel_err(planes_decode(res['C']), r), tol)]
        else:
            figs = [('C', rel_err(res['C'], r), tol)]
        figures[name] = figs
        assert all([_report(name, *f) for f in figs]), name
        return
    if c.get('ln'):
        bf16_check(name + ' pre', res['pre'], r, ab, excess=K + 16)
        mu = r.mean(1, keepdim=True)
        rstd = 1.0 / torch.sqrt(r.var(1, unbiased=False, keepdim=True) + 1e-5)
        y = (r - mu) * rstd * ctx['gam'].double() + ctx['bet'].double()
        absy = rstd * ctx['gam'].double().abs() * (r.abs() + mu.abs() + ab) + ctx['bet'].double().abs()
        bf16_check(name + ' C', res['C'], y, absy, excess=K + N + 16)
        figures[name] = [('rounding model', 0.0, float(K + N + 16))]
    else:
        bf16_check(name + ' C', res['C'], r, ab, excess=K + 16)
        figures[name] = [('rounding model', 0.0, float(K + 16))]


# ============================================================================================================ fused FFN dX
# hftt_ffn_bwd_dx in the x3 strip plans: dy masked on load with the output dropout's site (d = 256, masked-in-consumers), the stored hidden
# (bf16) as gate, dh out (bf16), the LayerNorm backward's dr as residual.  Bounds: test_x3_gpu.py::test_fused_ffn_forward_and_dx (dh 4e-3: a
# bf16 store; dx 6e-5) and test_small_fused_ffn_forward_and_dx.
# bf16 strip plans (strip_gemm2.hip / bs_strip.hip, every tensor bf16, no mask on load): test_strip_gpu.py::test_fused_ffn_backward_dx (dh 6e-3,
# dx 1e-2 from the rounded dh) and test_bf16_small_fused_ffn_forward_and_dx (dh 6e-3, dx 6e-3 from the device's dh).
FFN_CASES = {'ffn_bwd_dx_masked_dy': dict(d=256, p=512, drop=0.1, fam='x3'), 'ffn_bwd_dx_d64': dict(d=64, p=128, drop=0.0, fam='x3s'),
             'ffn_bwd_dx_bf16': dict(d=256, p=512, drop=0.0, fam='bf16'), 'ffn_bwd_dx_bf16_d64': dict(d=64, p=128, drop=0.0, fam='bs')}
FFN_SITE, FFN_SEED = 9, 4711


def build_ffn(dev, case, M, twin=False, dry=False):
    capi, ops, c = _capi(), _ops(), FFN_CASES[case]
    dm, pf = c['d'], c['p']
    g = torch.Generator().manual_seed(M + dm)
    rnd = lambda *s: torch.randn(*s, generator=g)                       # noqa: E731
    x3 = c['fam'] in ('x3', 'x3s')
    gs = 1.0 if c['fam'] == 'bf16' else 1e-5                       # (the magnitudes of the inherited tests)
    dt = F32 if x3 else BF
    dy, hid = rnd(M, dm) * gs, rnd(M, pf).to(BF)
    W1, W2 = rnd(pf, dm) / math.sqrt(dm), rnd(dm, pf) / math.sqrt(pf)
    res = rnd(M, dm) * gs
    pdy, vdy = in_plane(dev, dy.to(dev), dtype=dt)
    ph, vh = in_plane(dev, hid.to(dev))
    pr, vr = in_plane(dev, res.to(dev), dtype=dt)
    planes = {}
    planes['dx'], vdx = out_plane(dev, M, dm, dtype=dt)
    planes['dh'], vdh = out_plane(dev, M, pf, dtype=BF)
    d = capi.FfnDesc()
    d.M, d.d, d.p, d.mode = M, dm, pf, 1
    d.flags = (capi.SL_X3_BF16 | capi.SL_H_BF16 | capi.SL_PRE_BF16) if x3 else (capi.SL_X_BF16 | capi.SL_C_BF16 | capi.SL_RES_BF16)
    d.x, d.ldx = vdy.data_ptr(), dm
    d.h_out, d.ldh = vdh.data_ptr(), pf
    d.gate, d.ldg, d.gate_scale = vh.data_ptr(), pf, 1.25
    d.drop_p, d.site_o, d.drop_seed = c['drop'], (FFN_SITE if c['drop'] else 0), FFN_SEED
    d.residual, d.ldr = vr.data_ptr(), dm
    d.y, d.ldy = vdx.data_ptr(), dm
    keep = [pdy, ph, pr]
    W1d, W2d = W1.to(dev), W2.to(dev)
    if not dry:
        wp = {'x3': ops.x3_ffn_pack, 'x3s': ops.x3s_ffn_pack, 'bf16': ops.ffn_pack, 'bs': ops.x3s_ffn_pack}[c['fam']](W1d, W2d, backward=True)
        d.w = wp.data_ptr(); keep.append(wp)
    return dict(kind='ffn_bwd_dx', desc=d, descs=[('ffn_bwd_dx', d)], keep=keep, out_planes=planes, results={'dx': vdx, 'dh': vdh}, case=case, mode=c['fam'], c=c, M=M,
                dy=vdy, hid=vh, res=vr, W1=W1d, W2=W2d)


def launch_ffn(dev, ctx):
    capi = _capi()
    capi.check(capi.lib().hftt_ffn_bwd_dx(C.byref(ctx['desc']), stream(dev)), 'ffn_bwd_dx')


def check_ffn(ctx, figures):
    c, M = ctx['c'], ctx['M']
    name = 'ffn %s/M%d' % (ctx['case'], M)
    dev = ctx['dy'].device
    dy = ctx['dy'].double()
    if c['drop']:
        dy = dy * keep_mask_t(FFN_SEED, FFN_SITE, (M, c['d']), c['drop']).to(dev).double() * keep_scale(c['drop'])
    fam = c['fam']
    W1, W2 = (ctx['W1'].double(), ctx['W2'].double()) if fam in ('x3', 'x3s') else (ctx['W1'].to(BF).double(), ctx['W2'].to(BF).double())
    dh = torch.where(ctx['hid'].double() > 0, (dy @ W2) * 1.25, torch.zeros((), dtype=F64, device=dev))
    got_dh, got_dx = ctx['results']['dh'].float(), ctx['results']['dx'].float()
    if fam in ('x3', 'x3s'):
        figs = [('dh', rel_err(got_dh, dh), 4e-3), ('dx', rel_err(got_dx, dh @ W1 + ctx['res'].double()), 6e-5)]
    elif fam == 'bf16':
        figs = [('dh', rel_err(got_dh, dh), 6e-3), ('dx', rel_err(got_dx, dh.float().to(BF).double() @ W1 + ctx['res'].double()), 1e-2)]
    else:
        figs = [('dh', rel_err(got_dh, dh), 6e-3), ('dx', rel_err(got_dx, got_dh.double() @ W1 + ctx['res'].double()), 6e-3)]
    figures[name] = figs
    assert all([_report(name, *f) for f in figs]), name


# ============================================================================================================ fc_o + LayerNorm + FFN as one launch
# hftt_attn_out_ffn_fwd in the x3 strip plans at d = 256: the fc_o descriptor with the broadcast residual of the decoder's layer zero
# (res_mod = N_notes) and the FFN descriptor, every saved tensor between guards; the inference plan's form (o.C NULL, nothing saved) must give
# the same y to the bit.  Bounds: test_strip_linear_layernorm (bf16 pre-LN sum 4e-3, output / mean / rstd 1e-4) and
# test_fused_ffn_forward_and_dx with the bf16 hidden (hidden 4e-3, pre-LN sum 4e-3, y 1e-4, mean 1e-4).
OFFN_CASES = {'fc_o_res_mod_ln_ffn': dict(res_mod=88, drop=0.1)}
OFFN_SITES, OFFN_SEED = (20, 21, 22), 777


def build_offn(dev, case, M, twin=False, dry=False):
    """twin: the inference form -- nothing but y is written"""
    capi, ops, c = _capi(), _ops(), OFFN_CASES[case]
    dm, pf, save = 256, 512, not twin
    g = torch.Generator().manual_seed(M + 7)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)                       # noqa: E731
    ctx_, Wo, bo, res = rnd(M, dm), rnd(dm, dm) / 16.0, rnd(dm) * 0.3, rnd(c['res_mod'], dm)
    W1, W2, b1, b2 = rnd(pf, dm) / 16.0, rnd(dm, pf) / 22.0, rnd(pf) * 0.3, rnd(dm) * 0.3
    g1, be1, g2, be2 = rnd(dm), rnd(dm), rnd(dm), rnd(dm)
    pc, vctx = in_plane(dev, ctx_)
    pr, vres = in_plane(dev, res)
    planes, results = {}, {}
    planes['y'], vy = out_plane(dev, M, dm); results['y'] = vy
    for nm in ('mean1', 'rstd1', 'mean2', 'rstd2'):
        planes[nm], v = vec_plane(dev, M); results[nm] = v[0]
    if save:
        planes['x1'], results['x1'] = out_plane(dev, M, dm)
        planes['pre1'], results['pre1'] = out_plane(dev, M, dm, dtype=BF)
        planes['pre2'], results['pre2'] = out_plane(dev, M, dm, dtype=BF)
        planes['hid'], results['hid'] = out_plane(dev, M, pf, dtype=BF)
    else:                                              # the plan leaves f.x at the x1 buffer, which this form must not touch
        planes['x1_never_written'] = Plane(dev, M, dm)
    ptr = lambda k: results[k].data_ptr() if k in results else 0             # noqa: E731
    o = capi.StripDesc()
    o.M, o.N, o.K = M, dm, dm
    o.flags = capi.SL_X3_F16 | capi.SL_PRE_BF16
    o.x, o.ldx, o.bias = vctx.data_ptr(), dm, bo.data_ptr()
    o.C, o.ldc, o.out_scale, o.gate_scale = ptr('x1'), dm, 1.0, 1.0
    o.drop_p, o.drop_site, o.drop_seed = c['drop'], OFFN_SITES[0], OFFN_SEED
    o.residual, o.ldr, o.res_mod = vres.data_ptr(), dm, c['res_mod']
    o.ln_gamma, o.ln_beta, o.pre_ln_out, o.ln_mean, o.ln_rstd = g1.data_ptr(), be1.data_ptr(), ptr('pre1'), ptr('mean1'), ptr('rstd1')
    f = capi.FfnDesc()
    f.M, f.d, f.p, f.mode = M, dm, pf, 0
    f.flags = capi.SL_X3_F16 | capi.SL_H_BF16 | capi.SL_PRE_BF16
    f.x, f.ldx = (ptr('x1') if save else planes['x1_never_written'].buf[1:].data_ptr()), dm
    f.b1, f.b2 = b1.data_ptr(), b2.data_ptr()
    f.h_out, f.ldh = ptr('hid'), pf
    f.drop_p, f.site_h, f.site_o, f.drop_seed = c['drop'], OFFN_SITES[1], OFFN_SITES[2], OFFN_SEED
    f.ldr = dm
    f.ln_gamma, f.ln_beta, f.pre_ln_out, f.ln_mean, f.ln_rstd = g2.data_ptr(), be2.data_ptr(), ptr('pre2'), ptr('mean2'), ptr('rstd2')
    f.y, f.ldy = vy.data_ptr(), dm
    keep = [pc, pr, bo, b1, b2, g1, be1, g2, be2]
    if not dry:
        wp = ops.x3_attn_out_ffn_pack(Wo, W1, W2)
        o.w, f.w = wp.data_ptr(), wp.data_ptr() + 2 * (2 * dm * dm)
        keep.append(wp)
    return dict(kind='attn_out_ffn_fwd', descs=[('strip_linear', o), ('ffn_fwd', f)], o=o, f=f, keep=keep, out_planes=planes, results=results, case=case, mode='x3',
                c=c, M=M, t=dict(ctx=vctx, Wo=Wo, bo=bo, res=vres, W1=W1, W2=W2, b1=b1, b2=b2, g1=g1, be1=be1, g2=g2, be2=be2))


def launch_offn(dev, ctx):
    capi = _capi()
    capi.check(capi.lib().hftt_attn_out_ffn_fwd(C.byref(ctx['o']), C.byref(ctx['f']), stream(dev)), 'attn_out_ffn_fwd')


def check_offn(ctx, figures):
    c, M, t, r = ctx['c'], ctx['M'], {k: v.double() for k, v in ctx['t'].items()}, ctx['results']
    name = 'offn %s/M%d' % (ctx['case'], M)
    dev = ctx['t']['ctx'].device
    p, ks = c['drop'], keep_scale(c['drop'])
    mask = lambda site, n: keep_mask_t(OFFN_SEED, site, (M, n), p).to(dev).double() * ks             # noqa: E731
    r1 = (t['ctx'] @ t['Wo'].T + t['bo']) * mask(OFFN_SITES[0], 256) + t['res'][torch.arange(M, device=dev) % c['res_mod']]
    x1, m1, s1 = _ln_ref(r1, t['g1'], t['be1'])
    h = torch.relu(x1 @ t['W1'].T + t['b1']) * mask(OFFN_SITES[1], 512)
    r2 = x1 + (h @ t['W2'].T + t['b2']) * mask(OFFN_SITES[2], 256)
    y, m2, s2 = _ln_ref(r2, t['g2'], t['be2'])
    figs = [('pre1', rel_err(r['pre1'].float(), r1), 4e-3), ('x1', rel_err(r['x1'], x1), 1e-4), ('mean1', rel_err(r['mean1'], m1), 1e-4),
            ('rstd1', rel_err(r['rstd1'], s1), 1e-4), ('hid', rel_err(r['hid'].float(), h), 4e-3), ('pre2', rel_err(r['pre2'].float(), r2), 4e-3),
            ('y', rel_err(r['y'], y), 1e-4), ('mean2', rel_err(r['mean2'], m2), 1e-4)]
    figures[name] = figs
    assert all([_report(name, *f) for f in figs]), name


def twin_equal_offn(ctx, tw):
    for k in ('y', 'mean1', 'rstd1', 'mean2', 'rstd2'):
        assert torch.equal(ctx['results'][k], tw['results'][k]), 'attn_out_ffn_fwd: %s of the inference form differs from the training form' % k


# ============================================================================================================ attention
# layouts: 'self' -- q / k / v the column blocks of one [n L, 3d] projection, dq / dk / dv the column blocks of one [n L, 3d] gradient;
# 'cross' -- q [n Lq, d] contiguous, K / V at column block 1 of a three-layer stack [n Lk, 6d], dk / dv into the same block of a
# [n Lk, 6d] gradient; 'shared' -- cross with ONE query block for all sequences (sequence stride 0) and a per-sequence dq.
# modes: 'parity' npass 3; 'x3' npass 2 on fp32 operands; 'x3p' npass 2 on f16-pair planes (dh 64); 'bf16' npass 1, every tensor bf16 (dq of
# the shared query fp32, as the plan keeps it).
# Bounds.  Without dropout: test_kernels_gpu.py::test_attention_fwd_bwd (parity: map 2e-6, out 2 TOL[3], gradients 4 TOL[3]) and
# test_x3_gpu.py::test_attention_fwd_bwd (ptol = 4e-6 + 4e-7 lmax: map ptol, out 2 ptol, gradients gtol = 2e-4 + 3 ptol).  With dropout: the
# two test_attention_shared_query_and_dropout (parity: out 1e-4, gradients 2e-4; x3: out 1e-4, gradients 3e-4).  Planes: the forward is the
# fp32-operand forward's to the bit, the backward agrees with it to 4e-5 (test_attention_on_planes_equals_attention_on_fp32_operands): held
# to the x3 bound + 4e-5.  bf16: test_bf16_stream_attention_with_dropout (map 2e-2, out 2e-2, gradients 3e-2).
ATTN_N = 3
ATTN_CASES = {
    # H, Lq, Lk, dh, layout, dropout, map out, modes
    'self_88': dict(H=4, Lq=88, Lk=88, dh=64, lay='self', p=0.0, modes=('parity', 'x3', 'x3p', 'bf16')),
    'self_256_drop': dict(H=4, Lq=256, Lk=256, dh=64, lay='self', p=0.1, modes=('parity', 'x3', 'x3p', 'bf16')),
    'cross_88_256_map': dict(H=4, Lq=88, Lk=256, dh=64, lay='cross', p=0.0, probs=1, modes=('parity', 'x3', 'x3p', 'bf16')),
    'cross_88_256_drop': dict(H=4, Lq=88, Lk=256, dh=64, lay='cross', p=0.1, modes=('parity', 'x3', 'x3p', 'bf16')),
    'shared_88_256_drop': dict(H=4, Lq=88, Lk=256, dh=64, lay='shared', p=0.1, modes=('parity', 'x3', 'x3p', 'bf16')),
    'self_48_dh32_drop': dict(H=2, Lq=48, Lk=48, dh=32, lay='self', p=0.1, modes=('parity', 'x3', 'bf16')),
    'cross_12_48_dh32_map': dict(H=2, Lq=12, Lk=48, dh=32, lay='cross', p=0.0, probs=1, modes=('parity', 'x3', 'bf16')),
    'shared_12_48_dh32_drop': dict(H=2, Lq=12, Lk=48, dh=32, lay='shared', p=0.1, modes=('parity', 'x3', 'bf16')),
}
ATTN_SITE, ATTN_SEED = 9, 12345
ATTN_NPASS = {'parity': 3, 'x3': 2, 'x3p': 2, 'bf16': 1}


def build_attn(dev, case, mode, twin=False, dry=False):
    capi, c = _capi(), ATTN_CASES[case]
    n, H, Lq, Lk, dh, lay = ATTN_N, c['H'], c['Lq'], c['Lk'], c['dh'], c['lay']
    d = H * dh
    bf, pl = mode == 'bf16', mode == 'x3p'
    dt = BF if bf else F32
    g = torch.Generator().manual_seed(Lq * 1000 + Lk + dh)
    rnd = lambda *s: torch.randn(*s, generator=g)                       # noqa: E731
    nq = 1 if lay == 'shared' else n
    q, k, v = rnd(nq * Lq, d), rnd(n * Lk, d), rnd(n * Lk, d)
    do = rnd(n * Lq, d) * (1e-5 if mode in ('x3', 'x3p') else 1.0)
    if bf:
        q, k, v, do = (t.to(BF).float() for t in (q, k, v, do))
    q, k, v, do = (t.to(dev) for t in (q, k, v, do))
    keep, planes = [], {}
    if lay == 'self' and not twin:
        pin = Plane(dev, n * Lq, 3 * d, dt, NAN)
        vq, vk, vv = pin.block(0, d, q), pin.block(d, d, k), pin.block(2 * d, d, v)
        pg = planes['dqkv'] = Plane(dev, n * Lq, 3 * d, dt, SENT)
        dq, dk, dv = pg.block(0, d), pg.block(d, d), pg.block(2 * d, d)
        keep.append(pin)
    elif lay != 'self' and not twin:
        pq, vq = in_plane(dev, q, dtype=dt)
        pin = Plane(dev, n * Lk, 6 * d, dt, NAN)
        vk, vv = pin.block(2 * d, d, k), pin.block(3 * d, d, v)
        planes['dq'], dq = out_plane(dev, n * Lq, d, dtype=F32 if (bf and lay == 'shared') else dt)
        pg = planes['dkv'] = Plane(dev, n * Lk, 6 * d, dt, SENT)
        dk, dv = pg.block(2 * d, d), pg.block(3 * d, d)
        keep += [pq, pin]
    else:
        (pq, vq), (pk, vk), (pv, vv) = in_plane(dev, q, dtype=dt), in_plane(dev, k, dtype=dt), in_plane(dev, v, dtype=dt)
        planes['dq'], dq = out_plane(dev, n * Lq, d, dtype=F32 if (bf and lay == 'shared') else dt)
        planes['dk'], dk = out_plane(dev, n * Lk, d, dtype=dt)
        planes['dv'], dv = out_plane(dev, n * Lk, d, dtype=dt)
        keep += [pq, pk, pv]
    if pl and not dry:                                 # the operands as f16-pair planes, written in place by hftt_x3_to_planes (gaps stay NaN)
        L = capi.lib()
        for t in (vq, vk, vv):
            src = t.clone(memory_format=torch.contiguous_format)          # (the conversion is not an in-place operation)
            capi.check(L.hftt_x3_to_planes(src.data_ptr(), d, t.data_ptr(), t.stride(0), t.shape[0], d, stream(dev)), 'x3_to_planes')
    planes['out'], vo = out_plane(dev, n * Lq, d, dtype=dt)
    planes['lse'], vl = vec_plane(dev, n * H * Lq * 2)
    pdo, vdo = in_plane(dev, do, dtype=dt); keep.append(pdo)
    a = capi.AttnDesc()
    a.n_seq, a.n_heads, a.Lq, a.Lk, a.dh, a.npass = n, H, Lq, Lk, dh, ATTN_NPASS[mode]
    a.q, a.q_seq_stride, a.ldq = vq.data_ptr(), (0 if lay == 'shared' else Lq * vq.stride(0)), vq.stride(0)
    a.k, a.k_seq_stride, a.ldk = vk.data_ptr(), Lk * vk.stride(0), vk.stride(0)
    a.v, a.v_seq_stride, a.ldv = vv.data_ptr(), Lk * vv.stride(0), vv.stride(0)
    a.out, a.o_seq_stride, a.ldo = vo.data_ptr(), Lq * d, d
    a.lse = vl.data_ptr()
    results = {'out': vo, 'lse': vl[0], 'dq': dq, 'dk': dk, 'dv': dv}
    if c.get('probs'):
        planes['probs'], vp = vec_plane(dev, n * H * Lq * Lk)
        a.probs = vp.data_ptr()
        results['probs'] = vp[0]
    a.drop_p, a.drop_site, a.drop_seed = c['p'], ATTN_SITE, ATTN_SEED
    a.io_flags = ((1 | 2 | 4) if bf else 0) | ((capi.ATTN_Q_F16PAIR | capi.ATTN_KV_F16PAIR) if pl else 0)
    b = capi.AttnDesc()
    C.memmove(C.byref(b), C.byref(a), C.sizeof(a))
    b.probs = 0
    b.dout = vdo.data_ptr()
    b.dq, b.dq_seq_stride, b.lddq = dq.data_ptr(), Lq * dq.stride(0), dq.stride(0)
    b.dk, b.dk_seq_stride, b.lddk = dk.data_ptr(), Lk * dk.stride(0), dk.stride(0)
    b.dv, b.dv_seq_stride, b.lddv = dv.data_ptr(), Lk * dv.stride(0), dv.stride(0)
    if bf:
        b.io_flags |= 16 | (0 if lay == 'shared' else 8)
    return dict(kind='attn', descs=[('attn_fwd', a), ('attn_bwd', b)], fwd=a, bwd=b, keep=keep, out_planes=planes, results=results, case=case, mode=mode, c=c,
                q=vq, k=vk, v=vv, do=vdo, d=d)


def launch_attn(dev, ctx):
    capi = _capi()
    capi.check(capi.lib().hftt_attn_fwd(C.byref(ctx['fwd']), stream(dev)), 'attn_fwd')
    capi.check(capi.lib().hftt_attn_bwd(C.byref(ctx['bwd']), stream(dev)), 'attn_bwd')


def check_attn(ctx, figures):
    c, mode = ctx['c'], ctx['mode']
    name = 'attn %s/%s' % (ctx['case'], mode)
    n, H, Lq, Lk, dh, d, p = ATTN_N, c['H'], c['Lq'], c['Lk'], c['dh'], ctx['d'], c['p']
    dev = ctx['do'].device
    dec = planes_decode if mode == 'x3p' else (lambda t: t.double())
    q, k, v = dec(ctx['q']), dec(ctx['k']), dec(ctx['v'])
    if c['lay'] == 'shared':
        q = q.repeat(n, 1)                              # a leaf per sequence: the per-sequence dq
    q, k, v = (t.clone().requires_grad_(True) for t in (q, k, v))
    qh = q.view(n, Lq, H, dh).transpose(1, 2); kh = k.view(n, Lk, H, dh).transpose(1, 2); vh = v.view(n, Lk, H, dh).transpose(1, 2)
    e = qh @ kh.transpose(-1, -2) / math.sqrt(dh)
    pr = torch.softmax(e, -1)
    pd = pr * keep_mask_t(ATTN_SEED, ATTN_SITE, (n, H, Lq, Lk), p).to(dev).double() * keep_scale(p) if p > 0 else pr
    o = (pd @ vh).transpose(1, 2).reshape(n * Lq, d)
    (o * ctx['do'].double()).sum().backward()
    lmax = float(e.detach().abs().max())
    ptol = 4e-6 + 4e-7 * lmax
    if mode == 'parity':
        bp, bo, bg = (2e-6, 2 * TOL_K[3], 4 * TOL_K[3]) if p == 0 else (2e-5, 1e-4, 2e-4)
    elif mode == 'bf16':
        bp, bo, bg = 2e-2, 2e-2, 3e-2
    else:
        bp, bo, bg = (ptol, 2 * ptol, 2e-4 + 3 * ptol) if p == 0 else (2e-5, 1e-4, 3e-4)
        if mode == 'x3p':
            bg += 4e-5
    r = ctx['results']
    figs = [('out', rel_err(r['out'].float(), o.detach()), bo), ('dq', rel_err(r['dq'].float(), q.grad), bg), ('dk', rel_err(r['dk'].float(), k.grad), bg),
            ('dv', rel_err(r['dv'].float(), v.grad), bg)]
    if 'probs' in r:
        figs.append(('map', max_err(r['probs'], pr.detach().reshape(-1)), bp))
    figures[name] = figs
    assert all([_report(name, *f) for f in figs]), name


# ============================================================================================================ layout signatures
def _ptr(v):
    return int(v or 0)


def signature(entry, d):
    """(entry point, precision / storage word, sorted layout features) of one descriptor; no feature = the PLAIN layout of hftt_hip/ops.py"""
    f = set()
    if entry == 'gemm_nt':
        mode = (d.npass, d.io_flags)
        if d.lda > d.K: f.add('lda>K')
        if d.ldc > d.N: f.add('ldc>N')
        if _ptr(d.residual):
            if d.ldr > d.N: f.add('ldr>N')
            if _ptr(d.residual) == _ptr(d.C): f.add('C==residual')
            if 0 < d.res_mod < d.M: f.add('res_mod')
        if _ptr(d.gate) and d.ldg > d.N: f.add('ldg>N')
        if _ptr(d.add_table): f.add('add_mod')
    elif entry == 'gemm_tn':
        mode = (d.npass, d.io_flags & 7)             # (HFTT_TN_DY_DROP: a loader form on the plain layout, test_x3_gpu.py holds it)
        if d.lddy > d.N: f.add('lddy>N')
        if d.ldx > d.K: f.add('ldx>K')
        if d.n_seg > 1: f.add('n_seg=%d' % d.n_seg)
        covered = set()
        for s in range(d.n_seg):
            covered.update(range(d.seg_row0[s], d.seg_row0[s] + d.seg_rows[s]))
            if d.seg_rows[s] == 1: f.add('one-row segment')
        if len(covered) < d.N: f.add('rows in no segment')
        if d.K_out < d.K: f.add('K_out<K')
        if d.beta != 0.0: f.add('beta')
    elif entry == 'strip_linear':
        mode = (d.flags & ~8, 'small' if (d.K <= 192 and d.N <= 192) else 'wide')       # (ReLU is no layout)
        if d.ldx > d.K: f.add('ldx>K')
        if d.ldc > d.N: f.add('ldc>N')
        if _ptr(d.residual):
            if d.ldr > d.N: f.add('ldr>N')
            if _ptr(d.residual) == _ptr(d.C): f.add('C==residual')
            if d.res_mod > 0: f.add('res_mod')
    elif entry in ('ffn_fwd', 'ffn_bwd_dx'):
        mode = (d.flags, d.d)
        if d.ldx > d.d: f.add('ldx>d')
        if d.ldy > d.d: f.add('ldy>d')
        if _ptr(d.h_out) and d.ldh > d.p: f.add('ldh>p')
        if _ptr(d.gate) and d.ldg > d.p: f.add('ldg>p')
        if _ptr(d.residual) and d.ldr > d.d: f.add('ldr>d')
        if _ptr(d.y) in (_ptr(d.x), _ptr(d.residual)): f.add('y aliases an input')
    elif entry in ('attn_fwd', 'attn_bwd'):
        w = d.n_heads * d.dh
        mode = (d.npass, d.io_flags, d.dh)
        if d.ldq > w: f.add('ldq>d')
        if d.ldk > w: f.add('ldk>d')
        if d.ldv > w: f.add('ldv>d')
        if d.ldo > w: f.add('ldo>d')
        if d.q_seq_stride == 0: f.add('q_seq_stride=0')
        if entry == 'attn_bwd':
            if d.lddq > w: f.add('lddq>d')
            if d.lddk > w: f.add('lddk>d')
            if d.lddv > w: f.add('lddv>d')
    else:
        raise ValueError(entry)
    return (entry, mode, tuple(sorted(f)))


def is_plain(sig):
    return not sig[2]


def table_builds(dev):
    """every case of the table, built dry (descriptors only): (case id, ctx)"""
    for case, c in TN_CASES.items():
        for mode in c['modes']:
            yield 'tn-%s-%s' % (case, mode), build_tn(dev, case, mode, dry=True)
    for case, c in NT_CASES.items():
        for mode in c['modes']:
            yield 'nt-%s-%s' % (case, mode), build_nt(dev, case, mode, dry=True)
    for case, c in SL_CASES.items():
        for fam in c['fams']:
            yield 'sl-%s-%s' % (case, fam), build_sl(dev, case, fam, SL_MS[0], dry=True)
    for case in FFN_CASES:
        yield 'ffn-%s' % case, build_ffn(dev, case, SL_MS[0], dry=True)
    for case in OFFN_CASES:
        yield 'offn-%s' % case, build_offn(dev, case, SL_MS[0], dry=True)
        yield 'offn-%s-inference' % case, build_offn(dev, case, SL_MS[0], twin=True, dry=True)
    for case, c in ATTN_CASES.items():
        for mode in c['modes']:
            yield 'attn-%s-%s' % (case, mode), build_attn(dev, case, mode, dry=True)


def table_signatures(dev, without=()):
    sigs = {}
    for cid, ctx in table_builds(dev):
        if cid in without:
            continue
        for entry, d in ctx['descs']:
            sigs.setdefault(signature(entry, d), cid)
    return sigs


def plan_signatures(ws):
    """every GEMM, strip, FFN and attention launch of the three plans -> {signature: (plan, index, kernel)}"""
    found = {}
    for pname in ('fwd', 'fwd_inf', 'bwd'):
        for i, (fn, args, name, meta) in enumerate(ws.get(pname, ())):
            if isinstance(fn, str) or name not in ('gemm_nt', 'gemm_tn', 'strip_linear', 'ffn_fwd', 'ffn_bwd_dx', 'attn_fwd', 'attn_bwd'):
                continue
            descs = [a._obj for a in args if hasattr(a, '_obj')]
            if name == 'ffn_fwd' and len(descs) == 2:       # hftt_attn_out_ffn_fwd: the fc_o descriptor and the FFN descriptor, each as itself
                entries = [('strip_linear', descs[0]), ('ffn_fwd', descs[1])]
            else:
                entries = [(name, descs[0])]
            for entry, d in entries:
                found.setdefault(signature(entry, d), (pname, i, (meta or {}).get('kernel', '')))
    return found
