"""The split step loop of the x3 weight-gradient product (csrc/gemm_tn.hip: converts, LDS writes and refills inside the MFMA groups, on the
256-wide tiles) against the reference loop of the same library (HFTT_TN_PIPE=0, read by hftt_gemm_tn on every call): dW and db must agree
element for element, torch.equal.  The split loop moves loads, converts and LDS writes, never an MFMA, a column-sum addition or a hash index.
Forms that keep the reference loop by default (narrow tiles, the masked 256 x 256 forms) run the same kernel twice here and stay covered
should they change.

Shapes, worked through tn_plan by hand (tile rows x columns; splits of rows_per_split token rows; 32-row steps per split):
  M =  4100, N = 768, K = 256: 256 x 256, 3 tiles, 65 splits of 64 rows (2 steps), the last with 4 rows (1 step = one real and one zero step);
                                65 is no multiple of 8: seven padding slots per tile leave at once
  M = 12810, N = 768, K = 256: 256 x 256, 67 splits of 192 rows (6 steps), the last with 138 rows (5 steps, the fifth of 10 rows, then a zero step)
  M =  4100, N = 320, K = 320: 256 x 256, 4 tiles each one quarter to one half empty, 43 splits of 96 rows (3 steps + a zero step), the last 68 rows
  M =  4100, N = 256, K = 256: 128 x 256 (TM = 1), 2 tiles, 65 splits of 64 rows, the last with 4 rows
  M = 11990, N = 256, K = 256: 128 x 256, 125 splits of 96 rows (3 steps + a zero step), the last with 86 rows (third step of 22 rows)
  M = 12810, N = 256, K = 256: 128 x 256, 101 splits of 128 rows (4 steps), the last with 10 rows (1 step)
  M =  4100, N = 192, K =  96: 128 x 128 (TM = 1, TN = 2), 2 tiles half / a quarter empty, 65 splits of 64 rows
  M =  4100, N =  64, K =  64: 128 x 64 (TM = 1, TN = 1), half empty, 65 splits of 64 rows
(M = 13,000 at most: N = K = 256 cannot reach five steps there, 128 splits of at most 128 rows.)"""
import ctypes as C
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

DY_BF16, X_BF16, DY_HI, DY_DROP = 1, 2, 4, 8


def _grad_hi_built():
    from hftt_hip import _capi
    return bool(_capi.lib().hftt_build_options() & 1)


def _launch(dY, X, flags, segs, K_out, beta, priors, drop):
    """one hftt_gemm_tn call at npass 4 -> ([dW per segment], [db per segment]); priors = the (dW, db) a beta != 0 launch accumulates onto"""
    from hftt_hip import _capi, ops
    L = _capi.lib()
    M, N = dY.shape
    K = X.shape[1]
    d = _capi.GemmTnDesc()
    d.M, d.N, d.K, d.npass = M, N, K, 4
    d.dY, d.lddy, d.X, d.ldx = dY.data_ptr(), dY.stride(0), X.data_ptr(), X.stride(0)
    d.out_scale, d.beta, d.n_seg, d.K_out, d.io_flags = 0.5, beta, len(segs), K_out, flags
    if flags & DY_DROP:
        d.drop_p, d.drop_site, d.drop_seed = drop
    dws = [pw.clone() for pw, _ in priors]
    dbs = [pb.clone() for _, pb in priors]
    for i, (r0, rows) in enumerate(segs):
        d.seg_row0[i], d.seg_rows[i], d.seg_dw[i], d.seg_db[i] = r0, rows, dws[i].data_ptr(), dbs[i].data_ptr()
    ws = torch.empty(L.hftt_gemm_tn_ws_bytes(M, N, K) // 4 + 16, device=dY.device)
    d.ws, d.ws_bytes = ws.data_ptr(), ws.numel() * 4
    ops.check(L.hftt_gemm_tn(C.byref(d), ops._stream(dY.device)), 'gemm_tn')
    torch.cuda.synchronize()
    return dws, dbs


def _both(dev, M, N, K, flags=0, segs=None, K_out=None, beta=0.0, drop=(0.1, 3, 1234)):
    g = torch.Generator().manual_seed(M + 7 * N + 13 * K + flags)
    dY = (torch.randn(M, N, generator=g) * 1e-3).to(dev)
    X = torch.randn(M, K, generator=g).to(dev)
    if flags & DY_BF16: dY = dY.bfloat16()
    if flags & X_BF16: X = X.bfloat16()
    segs = segs or [(0, N)]
    K_out = K_out or K
    # outputs start from the same finite values on both paths, so that an element one path leaves unwritten differs
    priors = [((torch.randn(rows, K_out, generator=g) * 0.1).to(dev), (torch.randn(rows, generator=g) * 0.1).to(dev)) for _, rows in segs]
    old = os.environ.pop('HFTT_TN_PIPE', None)
    try:
        new = _launch(dY, X, flags, segs, K_out, beta, priors, drop)
        os.environ['HFTT_TN_PIPE'] = '0'
        ref = _launch(dY, X, flags, segs, K_out, beta, priors, drop)
    finally:
        os.environ.pop('HFTT_TN_PIPE', None)
        if old is not None:
            os.environ['HFTT_TN_PIPE'] = old
    for i in range(len(segs)):
        assert bool(torch.isfinite(ref[0][i]).all()) and float(ref[0][i].abs().max()) > 0
        assert torch.equal(new[0][i], ref[0][i]), ('dW', i, int((new[0][i] != ref[0][i]).sum()))
        assert torch.equal(new[1][i], ref[1][i]), ('db', i, int((new[1][i] != ref[1][i]).sum()))
    return new


STORAGE = {'f32_f32': 0, 'dy_bf16': DY_BF16, 'x_bf16': X_BF16, 'drop_x_f32': DY_DROP, 'drop_x_bf16': DY_DROP | X_BF16}


@pytest.mark.parametrize('storage', list(STORAGE))
@pytest.mark.parametrize('M,N,K', [(4100, 768, 256), (12810, 768, 256), (4100, 320, 320), (4100, 256, 256), (11990, 256, 256), (12810, 256, 256)])
def test_pipelined_schedule_is_bit_identical_to_the_reference(dev, M, N, K, storage):
    _both(dev, M, N, K, STORAGE[storage])
    if storage in ('f32_f32', 'x_bf16') and _grad_hi_built():      # HFTT_TN_DY_HI, in a library built with HFTT_BUILD_GRAD_HI=1
        _both(dev, M, N, K, STORAGE[storage] | DY_HI)


@pytest.mark.parametrize('storage', ['f32_f32', 'dy_bf16', 'x_bf16'])
@pytest.mark.parametrize('M,N,K', [(4100, 192, 96), (4100, 64, 64)])
def test_small_tiles_are_bit_identical_to_the_reference(dev, M, N, K, storage):
    """the 128 x 128 and 128 x 64 tiles (the masked form exists for the 256-wide tiles only)"""
    _both(dev, M, N, K, STORAGE[storage])


@pytest.mark.parametrize('M,N,K,K_out', [(4100, 256, 256, 200), (12810, 512, 256, 65)])
def test_k_out_below_k(dev, M, N, K, K_out):
    _both(dev, M, N, K, K_out=K_out)


@pytest.mark.parametrize('M,N,K', [(12810, 768, 256), (4100, 256, 256)])
def test_three_segments_accumulated_onto_a_prior(dev, M, N, K):
    r = N // 4
    new = _both(dev, M, N, K, segs=[(0, r), (r, 2 * r), (3 * r, r)], beta=1.0)
    assert [tuple(w.shape) for w in new[0]] == [(r, K), (2 * r, K), (r, K)]
