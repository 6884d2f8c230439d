"""Tensor-level wrappers of single C-ABI kernels (used by tests, by ``model.amt`` for the log-mel front end and by
tools).  Each wrapper only builds the POD descriptor from torch tensors and enqueues the kernel on torch's
current stream; results are torch tensors.  No arithmetic happens in Python/torch here.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from ._capi import (ADAM_MAX_GROUPS, AdamEmaDesc, AdamGroupsDesc, AttnDesc, ClipLogmelDesc, ClipLogmelMixDesc, ClipLogmelMixWarpDesc, ClipLogmelWarpDesc, ClipMixArgs, ClipRoomDesc, ClipSynthDesc, ClipSynthPartsDesc, ClipWindowsDesc, FfnDesc, GemmNtDesc, GemmTnDesc, HfttError, LabelNote, LabelsDesc, LabelsMixDesc, LabelsWarpDesc, LnBwdDesc, LogmelDesc, LossDesc, NotesDesc, NotesSegDesc, NotesStreamDesc, ResampleDesc, ResampleStreamDesc, PrepEntry, StitchDesc, StripDesc, StripPackEntry, WarpArgs, WaveWarpDesc,
                    WARP_DELAY_MAX, WARP_STEP_MAX, WARP_STEP_MIN, WARP_TABLE_L, WARP_TABLE_LEN, WARP_ZEROS,
                    LABELS_STORE, LABELS_TRAIN, NOTES_CHUNK, ROOM_MAX_TAPS, STITCH_MAX_CLIPS, SYNTH_MAX_PARTIALS,
                    SL_C_BF16, SL_C_F16PAIR, SL_H_BF16, SL_PRE_BF16, SL_RELU, SL_X3_GRAD_HI, SL_RES_BF16, SL_X_BF16, SL_X3_F16, SL_X3_BF16, SL_X_DROP,
                    ATTN_Q_F16PAIR, ATTN_KV_F16PAIR, check, lib)


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _need_cuda(*ts):
    for t in ts:
        if t is not None and t.device.type != 'cuda':
            raise HfttError('hftt ops need ROCm device tensors (got %s); there is no CPU fallback' % t.device)


BF16 = torch.bfloat16
NT_A_BF16, NT_C_BF16, NT_GATE_BF16, NT_RES_BF16, NT_A_HI = 1, 2, 4, 8, 16
TN_DY_BF16, TN_X_BF16, TN_DY_HI, TN_DY_DROP = 1, 2, 4, 8
ATTN_Q_BF16, ATTN_KV_BF16, ATTN_O_BF16, ATTN_DQ_BF16, ATTN_DKV_BF16 = 1, 2, 4, 8, 16


def _align(x, a):
    return (x + a - 1) // a * a


def prepare_weight(w: torch.Tensor, npass=3, transposed=False, n_pad=64):
    """fp32 [rows, cols] -> the GEMM operand [align(rows, n_pad), cols] (or its transpose): bf16 (int16 tensor) for npass 1,
    fp32 for npass 3; npass 2 / 4 (split fp16 / bf16): an int16 tensor [2, rows_pad, cols] holding the hi plane, then the lo plane."""
    _need_cuda(w)
    w = w.contiguous().float()
    rows, cols = w.shape
    if transposed:
        out_r, out_c = _align(cols, n_pad), _align(rows, 32)
    else:
        out_r, out_c = _align(rows, n_pad), cols
    if npass in (2, 4):
        out = torch.zeros(2, out_r, out_c, dtype=torch.int16, device=w.device)
        ent = (PrepEntry * 1)(PrepEntry(0, 0, rows, cols, cols, out_c, 1 if transposed else 0, npass))
        table = torch.frombuffer(bytearray(bytes(ent)), dtype=torch.uint8).to(w.device)
        check(lib().hftt_prep_weights_x3(w.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), 0, table.data_ptr(), 1, _stream(w.device)), 'prep_weights_x3')
        return out
    out = torch.zeros(out_r, out_c, dtype=torch.int16 if npass == 1 else torch.float32, device=w.device)
    ent = (PrepEntry * 1)(PrepEntry(0, 0, rows, cols, cols, out_c, 1 if transposed else 0, 0))
    table = torch.frombuffer(bytearray(bytes(ent)), dtype=torch.uint8).to(w.device)
    check(lib().hftt_prep_weights(w.data_ptr(), out.data_ptr() if npass == 1 else 0, out.data_ptr() if npass == 3 else 0, 0,
                                  table.data_ptr(), 1, _stream(w.device)), 'prep_weights')
    return out


def gemm_nt(A, W, bias=None, npass=3, act=0, out_scale=1.0, add_table=None, add_mod=0, gate=None, gate_scale=1.0,
            drop_p=0.0, drop_site=0, drop_seed=0, residual=None, res_mod=0, ln=None, planes=None, debug=0, out_dtype=torch.float32, grad_hi=False):
    """C = epi(A @ W.T + bias); W fp32 [N, K].  ln = (gamma, beta) -> returns (C, pre_ln, mean, rstd).  grad_hi (npass 4): A enters as
    its bf16 rounding (NT_A_HI)."""
    _need_cuda(A, W)
    M, K = A.shape
    N = W.shape[0]
    Wprep = planes if planes is not None else prepare_weight(W, npass)
    Cout = torch.empty(M, N, device=A.device, dtype=out_dtype)
    d = GemmNtDesc()
    d.M, d.N, d.K, d.npass = M, N, K, npass
    d.A, d.lda = A.data_ptr(), A.stride(0)
    d.W = Wprep.data_ptr()
    if npass in (2, 4):
        d.W_lo = Wprep[1].data_ptr()
    d.debug = debug
    d.io_flags = (NT_A_BF16 if A.dtype == BF16 else 0) | (NT_C_BF16 if out_dtype == BF16 else 0) | (NT_GATE_BF16 if (gate is not None and gate.dtype == BF16) else 0) \
        | (NT_RES_BF16 if (residual is not None and residual.dtype == BF16) else 0) | (NT_A_HI if grad_hi else 0)
    d.bias = bias.data_ptr() if bias is not None else 0
    d.C, d.ldc = Cout.data_ptr(), N
    d.act, d.out_scale = act, out_scale
    if add_table is not None:
        d.add_table, d.add_mod = add_table.data_ptr(), add_mod
    if gate is not None:
        d.gate, d.ldg, d.gate_scale = gate.data_ptr(), gate.stride(0), gate_scale
    d.drop_p, d.drop_site, d.drop_seed = drop_p, drop_site, drop_seed
    if residual is not None:
        d.residual, d.ldr, d.res_mod = residual.data_ptr(), residual.stride(0), (res_mod or M)
    extra = ()
    if ln is not None:
        pre = torch.empty(M, N, device=A.device)
        mean = torch.empty(M, device=A.device)
        rstd = torch.empty(M, device=A.device)
        d.ln_gamma, d.ln_beta = ln[0].data_ptr(), ln[1].data_ptr()
        d.pre_ln_out, d.ln_mean, d.ln_rstd = pre.data_ptr(), mean.data_ptr(), rstd.data_ptr()
        extra = (pre, mean, rstd)
    check(lib().hftt_gemm_nt(C.byref(d), _stream(A.device)), 'gemm_nt')
    return (Cout,) + extra if extra else Cout


# ---------------------------------------------------------------------------------------------------------------------
# strip kernels (bf16 mode): packed weights, token strips
# ---------------------------------------------------------------------------------------------------------------------
def strip_pack_table(entries, device):
    arr = (StripPackEntry * len(entries))(*[StripPackEntry(*e) for e in entries])
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device), len(entries)


def strip_pack(w: torch.Tensor, transpose=False, order=0, out=None, slot_stride=1, slot_offset=0):
    """fp32 [rows, cols] -> strip-packed bf16 stream of the logical matrix Wl = w (or w.T): int16 tensor of Wl.numel() elements
    (or written into `out` at the given slot stride / offset)."""
    _need_cuda(w)
    w = w.contiguous().float()
    rows, cols = w.shape
    K = rows if transpose else cols
    if out is None:
        out = torch.zeros(w.numel() * slot_stride, dtype=torch.int16, device=w.device)
    table, n = strip_pack_table([(0, 0, rows, cols, cols, 1 if transpose else 0, 0, 0, K, order, slot_stride, slot_offset)], w.device)
    check(lib().hftt_strip_pack(w.data_ptr(), out.data_ptr(), table.data_ptr(), n, _stream(w.device)), 'strip_pack')
    return out


def ffn_pack(w1: torch.Tensor, w2: torch.Tensor, backward=False):
    """Interleaved stream of the fused FFN.  forward: slot 2t = tile t of fc_1.weight [p, d] (tile-major), slot 2t+1 = K-slice t
    of fc_2.weight [d, p].  backward (dX): first matrix = fc_2.weight^T [p, d], second = fc_1.weight^T [d, p]."""
    out = torch.zeros(w1.numel() + w2.numel(), dtype=torch.int16, device=w1.device)
    if not backward:
        strip_pack(w1, False, 1, out, 2, 0)
        strip_pack(w2, False, 0, out, 2, 1)
    else:
        strip_pack(w2, True, 1, out, 2, 0)
        strip_pack(w1, True, 0, out, 2, 1)
    return out


def x3_strip_pack(w: torch.Tensor, elem=2, transpose=False, order=0, out=None, slot_stride=2, slot_offset=0):
    """fp32 [rows, cols] -> split-operand strip stream of the logical matrix Wl = w (or w.T): (hi, lo) fragment pairs of fp16 (elem 2)
    or bf16 (elem 4) halves, 2 * Wl.numel() int16 elements (or written into `out` at the given pair stride / offset)."""
    _need_cuda(w)
    w = w.contiguous().float()
    rows, cols = w.shape
    K = rows if transpose else cols
    if out is None:
        out = torch.zeros(2 * w.numel() * (slot_stride // 2), dtype=torch.int16, device=w.device)
    table, n = strip_pack_table([(0, 0, rows, cols, cols, 1 if transpose else 0, 0, 0, K, order, slot_stride, slot_offset)], w.device)
    check(lib().hftt_x3_strip_pack(w.data_ptr(), out.data_ptr(), table.data_ptr(), n, elem, _stream(w.device)), 'x3_strip_pack')
    return out


def x3_ffn_pack(w1: torch.Tensor, w2: torch.Tensor, backward=False):
    """Interleaved split-operand stream of the fused FFN: per hidden tile two slots of the first matrix, then two of the second."""
    out = torch.zeros(2 * (w1.numel() + w2.numel()), dtype=torch.int16, device=w1.device)
    if not backward:
        x3_strip_pack(w1, 2, False, 1, out, 4, 0)
        x3_strip_pack(w2, 2, False, 0, out, 4, 2)
    else:
        x3_strip_pack(w2, 4, True, 1, out, 4, 0)
        x3_strip_pack(w1, 4, True, 0, out, 4, 2)
    return out


def x3s_pack(w: torch.Tensor, elem=2, transpose=False, nt=None, out=None, pair_offset=0):
    """fp32 [rows, cols] -> COMPACT split-operand pack (order 2) of the logical matrix Wl = w (or w.T) for the small-width strip kernels
    (csrc/x3s_strip.h): the (hi, lo) pair of (k chunk c, output tile t) at pair index pair_offset + c * nt + t, 1024 int16 elements per pair."""
    _need_cuda(w)
    w = w.contiguous().float()
    rows, cols = w.shape
    K, N = (rows, cols) if transpose else (cols, rows)
    nt = nt or N // 32
    if out is None:
        out = torch.zeros((pair_offset + (K // 16) * nt) * 1024, dtype=torch.int16, device=w.device)
    table, n = strip_pack_table([(0, 0, rows, cols, cols, 1 if transpose else 0, 0, 0, K, 2, nt, pair_offset)], w.device)
    check(lib().hftt_x3_strip_pack(w.data_ptr(), out.data_ptr(), table.data_ptr(), n, elem, _stream(w.device)), 'x3_strip_pack')
    return out


def x3s_ffn_pack(w1: torch.Tensor, w2: torch.Tensor, backward=False, bf16=False):
    """the fused block's two matrices at d = 64, p = 128: pairs 0 .. 15 the first GEMM's, 16 .. 31 the second's
    (bf16: bf16 halves for the forward matrices too -- the pack of the bf16 small-width family, csrc/bs_strip.hip, which reads the hi fragments)"""
    out = torch.zeros(32 * 1024, dtype=torch.int16, device=w1.device)
    if not backward:
        x3s_pack(w1, 4 if bf16 else 2, False, 4, out, 0)        # fc_1.weight [p, d]
        x3s_pack(w2, 4 if bf16 else 2, False, 2, out, 16)       # fc_2.weight [d, p]
    else:
        x3s_pack(w2, 4, True, 4, out, 0)         # fc_2.weight^T [p, d]
        x3s_pack(w1, 4, True, 2, out, 16)        # fc_1.weight^T [d, p]
    return out


def strip_linear(x, wpack, N, bias=None, relu=False, out_scale=1.0, gate=None, gate_scale=1.0, drop_p=0.0, drop_site=0, drop_seed=0,
                 residual=None, res_mod=0, ln=None, out_dtype=BF16, save_pre=True, x3=0, pre_bf16=False, grad_hi=False, c_planes=False, x_drop=False):
    """C = epi(x @ Wl.T + bias) with Wl given as its strip pack.  ln = (gamma, beta) -> (C, pre_ln, mean, rstd).
    x3 = 2 / 4: the split-operand form (fp32 tensors, wpack from x3_strip_pack with the same element type).
    x_drop (x3 = 4, N == K == 256): HFTT_SL_X_DROP -- x is the gradient of a dropout output; the mask of (drop_p, drop_site, drop_seed) is applied
    to x while it is loaded (no dropout on the result)."""
    _need_cuda(x, wpack)
    M, K = x.shape
    if x3:
        out_dtype = torch.float32
    Cout = torch.empty(M, N, device=x.device, dtype=out_dtype)
    d = StripDesc()
    d.M, d.N, d.K = M, N, K
    d.flags = (SL_X_BF16 if x.dtype == BF16 else 0) | (SL_C_BF16 if out_dtype == BF16 else 0) | (SL_RELU if relu else 0) \
        | (SL_RES_BF16 if (residual is not None and residual.dtype == BF16) else 0) | (SL_X3_F16 if x3 == 2 else 0) | (SL_X3_BF16 if x3 == 4 else 0) \
        | (SL_PRE_BF16 if (x3 and pre_bf16 and ln is not None) else 0) | (SL_X3_GRAD_HI if (x3 == 4 and grad_hi) else 0) | (SL_C_F16PAIR if c_planes else 0) \
        | (SL_X_DROP if x_drop else 0)
    d.x, d.ldx, d.w = x.data_ptr(), x.stride(0), wpack.data_ptr()
    d.bias = bias.data_ptr() if bias is not None else 0
    d.C, d.ldc, d.out_scale, d.gate_scale = Cout.data_ptr(), N, out_scale, gate_scale
    if gate is not None:
        d.gate, d.ldg = gate.data_ptr(), gate.stride(0)
    d.drop_p, d.drop_site, d.drop_seed = drop_p, drop_site, drop_seed
    if residual is not None:
        d.residual, d.ldr, d.res_mod = residual.data_ptr(), residual.stride(0), res_mod
    extra = ()
    if ln is not None:
        pre = torch.empty(M, N, device=x.device, dtype=BF16 if (x3 and pre_bf16) else out_dtype) if save_pre else None
        mean = torch.empty(M, device=x.device)
        rstd = torch.empty(M, device=x.device)
        d.ln_gamma, d.ln_beta = ln[0].data_ptr(), ln[1].data_ptr()
        d.pre_ln_out, d.ln_mean, d.ln_rstd = (pre.data_ptr() if save_pre else 0), mean.data_ptr(), rstd.data_ptr()
        extra = (pre, mean, rstd)
    check(lib().hftt_strip_linear(C.byref(d), _stream(x.device)), 'strip_linear')
    return (Cout,) + extra if extra else Cout


def ffn_res_ln_fwd(x, wpack, p, b1, b2, gamma, beta, drop_p=0.0, site_h=0, site_o=0, seed=0, save_hidden=True, save_pre=True, residual=None, x3=False, hidden_bf16=False, pre_bf16=False):
    """Fused FFN block: y = LN(x + drop(fc_2(drop(relu(fc_1 x))))) -> (y, hidden | None, pre_ln | None, mean, rstd); all bf16
    (x3: all fp32, wpack from x3_ffn_pack; hidden_bf16: the stored hidden as bf16, SL_H_BF16)."""
    _need_cuda(x, wpack)
    M, dm = x.shape
    dt = torch.float32 if x3 else BF16
    y = torch.empty(M, dm, device=x.device, dtype=dt)
    hid = torch.empty(M, p, device=x.device, dtype=BF16 if hidden_bf16 else dt) if save_hidden else None
    pre = torch.empty(M, dm, device=x.device, dtype=BF16 if (x3 and pre_bf16) else dt) if save_pre else None
    mean = torch.empty(M, device=x.device); rstd = torch.empty(M, device=x.device)
    d = FfnDesc()
    d.M, d.d, d.p, d.flags, d.mode = M, dm, p, ((SL_X3_F16 | (SL_H_BF16 if hidden_bf16 else 0) | (SL_PRE_BF16 if pre_bf16 else 0)) if x3 else (SL_X_BF16 | SL_C_BF16 | SL_RES_BF16)), 0
    d.x, d.ldx, d.w = x.data_ptr(), x.stride(0), wpack.data_ptr()
    d.b1, d.b2 = b1.data_ptr(), b2.data_ptr()
    if save_hidden:
        d.h_out, d.ldh = hid.data_ptr(), p
    d.drop_p, d.site_h, d.site_o, d.drop_seed = drop_p, site_h, site_o, seed
    if residual is not None:
        d.residual, d.ldr = residual.data_ptr(), residual.stride(0)
    d.ln_gamma, d.ln_beta = gamma.data_ptr(), beta.data_ptr()
    d.pre_ln_out = pre.data_ptr() if save_pre else 0
    d.ln_mean, d.ln_rstd = mean.data_ptr(), rstd.data_ptr()
    d.y, d.ldy = y.data_ptr(), dm
    check(lib().hftt_ffn_res_ln_fwd(C.byref(d), _stream(x.device)), 'ffn_res_ln_fwd')
    return y, hid, pre, mean, rstd


def x3_attn_out_ffn_pack(wo: torch.Tensor, w1: torch.Tensor, w2: torch.Tensor):
    """The weight stream of hftt_attn_out_ffn_fwd: fc_o's 16 slots (order 0), then the fused FFN's interleaved stream (x3_ffn_pack), fp16 halves."""
    out = torch.zeros(2 * (wo.numel() + w1.numel() + w2.numel()), dtype=torch.int16, device=wo.device)
    x3_strip_pack(wo, 2, False, 0, out[:2 * wo.numel()])
    x3_strip_pack(w1, 2, False, 1, out[2 * wo.numel():], 4, 0)
    x3_strip_pack(w2, 2, False, 0, out[2 * wo.numel():], 4, 2)
    return out


def attn_out_ffn_fwd(ctx, wpack, bo, residual, gamma1, beta1, p, b1, b2, gamma2, beta2, drop_p=0.0, site_a=0, site_h=0, site_o=0, seed=0, res_mod=0,
                     save=True, hidden_bf16=False, pre_bf16=False):
    """hftt_attn_out_ffn_fwd (x3): x1 = LN1(residual + drop(ctx @ Wo.T + bo)); y = LN2(x1 + drop(FFN(x1))) as ONE launch.
    save=True (training plan) -> (y, x1, pre1, mean1, rstd1, hidden, pre2, mean2, rstd2); save=False (inference plan) -> y only, x1 is never written."""
    _need_cuda(ctx, wpack, residual)
    M, dm = ctx.shape
    dev = ctx.device
    y = torch.empty(M, dm, device=dev)
    mean1 = torch.empty(M, device=dev); rstd1 = torch.empty(M, device=dev); mean2 = torch.empty(M, device=dev); rstd2 = torch.empty(M, device=dev)
    x1 = torch.empty(M, dm, device=dev) if save else None
    pre1 = torch.empty(M, dm, device=dev, dtype=BF16 if pre_bf16 else torch.float32) if save else None
    pre2 = torch.empty(M, dm, device=dev, dtype=BF16 if pre_bf16 else torch.float32) if save else None
    hid = torch.empty(M, p, device=dev, dtype=BF16 if hidden_bf16 else torch.float32) if save else None
    o = StripDesc()
    o.M, o.N, o.K = M, dm, dm
    o.flags = SL_X3_F16 | (SL_PRE_BF16 if pre_bf16 else 0)
    o.x, o.ldx, o.w, o.bias = ctx.data_ptr(), ctx.stride(0), wpack.data_ptr(), bo.data_ptr()
    o.C, o.ldc, o.out_scale, o.gate_scale = (x1.data_ptr() if save else 0), dm, 1.0, 1.0
    o.drop_p, o.drop_site, o.drop_seed = drop_p, site_a, seed
    o.residual, o.ldr, o.res_mod = residual.data_ptr(), residual.stride(0), res_mod
    o.ln_gamma, o.ln_beta = gamma1.data_ptr(), beta1.data_ptr()
    o.pre_ln_out, o.ln_mean, o.ln_rstd = (pre1.data_ptr() if save else 0), mean1.data_ptr(), rstd1.data_ptr()
    f = FfnDesc()
    f.M, f.d, f.p, f.flags, f.mode = M, dm, p, SL_X3_F16 | (SL_H_BF16 if hidden_bf16 else 0) | (SL_PRE_BF16 if pre_bf16 else 0), 0
    f.x, f.ldx, f.w = (x1.data_ptr() if save else y.data_ptr()), dm, wpack.data_ptr() + 2 * (2 * dm * dm)      # (f.x is not read: the strip comes from the registers)
    f.b1, f.b2 = b1.data_ptr(), b2.data_ptr()
    if save:
        f.h_out, f.ldh = hid.data_ptr(), p
    f.drop_p, f.site_h, f.site_o, f.drop_seed = drop_p, site_h, site_o, seed
    f.ln_gamma, f.ln_beta = gamma2.data_ptr(), beta2.data_ptr()
    f.pre_ln_out = pre2.data_ptr() if save else 0
    f.ln_mean, f.ln_rstd = mean2.data_ptr(), rstd2.data_ptr()
    f.y, f.ldy = y.data_ptr(), dm
    check(lib().hftt_attn_out_ffn_fwd(C.byref(o), C.byref(f), _stream(dev)), 'attn_out_ffn_fwd')
    return (y, x1, pre1, mean1, rstd1, hid, pre2, mean2, rstd2) if save else y


def ffn_bwd_dx(dy, wpack_bwd, p, hidden, gate_scale=1.0, residual=None, x3=False, grad_hi=False, dy_drop=None):
    """dh = (hidden > 0) * (dy @ fc_2.weight) * gate_scale;  dx = dh @ fc_1.weight (+ residual) -> (dx, dh); all bf16 (x3: all fp32).
    dy_drop = (p, site, seed) (x3): dy is the gradient of the block's OUTPUT dropout and is masked with that site while it is loaded."""
    _need_cuda(dy, wpack_bwd, hidden)
    M, dm = dy.shape
    dt = torch.float32 if x3 else BF16
    dx = torch.empty(M, dm, device=dy.device, dtype=dt)
    hbf = x3 and hidden.dtype == BF16                     # x3 with the hidden stored as bf16: dh leaves as bf16 too (SL_H_BF16)
    dh = torch.empty(M, p, device=dy.device, dtype=BF16 if hbf else dt)
    d = FfnDesc()
    d.M, d.d, d.p, d.flags, d.mode = M, dm, p, ((SL_X3_BF16 | (SL_H_BF16 if hbf else 0) | (SL_X3_GRAD_HI if grad_hi else 0)) if x3 else (SL_X_BF16 | SL_C_BF16 | SL_RES_BF16)), 1
    d.x, d.ldx, d.w = dy.data_ptr(), dy.stride(0), wpack_bwd.data_ptr()
    d.h_out, d.ldh = dh.data_ptr(), p
    d.gate, d.ldg, d.gate_scale = hidden.data_ptr(), hidden.stride(0), gate_scale
    if dy_drop is not None:
        d.drop_p, d.site_o, d.drop_seed = dy_drop
    if residual is not None:
        d.residual, d.ldr = residual.data_ptr(), residual.stride(0)
    d.y, d.ldy = dx.data_ptr(), dm
    check(lib().hftt_ffn_bwd_dx(C.byref(d), _stream(dy.device)), 'ffn_bwd_dx')
    return dx, dh


def gemm_tn(dY, X, npass=3, out_scale=1.0, with_bias=True, grad_hi=False, dy_drop=None):
    """dW[N,K] = out_scale * dY[M,N].T @ X[M,K]; db[N] = colsum(dY).
    dy_drop = (p, site, seed) (npass 4, fp32 dY): HFTT_TN_DY_DROP -- dY is masked with that dropout site while it is loaded."""
    _need_cuda(dY, X)
    M, N = dY.shape
    K = X.shape[1]
    dW = torch.empty(N, K, device=dY.device)
    db = torch.empty(N, device=dY.device)
    L = lib()
    wsb = L.hftt_gemm_tn_ws_bytes(M, N, K)
    ws = torch.empty(wsb // 4 + 16, device=dY.device)
    d = GemmTnDesc()
    d.M, d.N, d.K, d.npass = M, N, K, npass
    d.dY, d.lddy, d.X, d.ldx = dY.data_ptr(), dY.stride(0), X.data_ptr(), X.stride(0)
    d.out_scale, d.beta, d.n_seg = out_scale, 0.0, 1
    d.io_flags = (TN_DY_BF16 if dY.dtype == BF16 else 0) | (TN_X_BF16 if X.dtype == BF16 else 0) | (TN_DY_HI if (grad_hi and dY.dtype != BF16) else 0) \
        | (TN_DY_DROP if dy_drop is not None else 0)
    if dy_drop is not None:
        d.drop_p, d.drop_site, d.drop_seed = dy_drop
    d.seg_row0[0], d.seg_rows[0], d.seg_dw[0], d.seg_db[0] = 0, N, dW.data_ptr(), (db.data_ptr() if with_bias else 0)
    d.K_out = K
    d.ws, d.ws_bytes = ws.data_ptr(), ws.numel() * 4
    check(L.hftt_gemm_tn(C.byref(d), _stream(dY.device)), 'gemm_tn')
    return dW, db


def to_planes(x):
    """fp32 [..., cols] (contiguous, cols % 32 == 0) -> the f16-pair plane form of the same shape (hftt_x3_to_planes): per 32-column group the
    32 fp16 hi halves, then the 32 lo halves, in the group's 128 bytes.  A float32 tensor whose BYTES are the planes."""
    _need_cuda(x)
    assert x.dtype == torch.float32 and x.is_contiguous() and x.shape[-1] % 32 == 0
    out = torch.empty_like(x)
    cols = x.shape[-1]
    check(lib().hftt_x3_to_planes(x.data_ptr(), cols, out.data_ptr(), cols, x.numel() // cols, cols, _stream(x.device)), 'x3_to_planes')
    return out


def _attn_desc(q, k, v, n_heads, npass, drop_p, drop_site, drop_seed, planes=False):
    n_seq, Lq, dm = q.shape
    Lk = k.shape[1]
    d = AttnDesc()
    d.n_seq, d.n_heads, d.Lq, d.Lk, d.dh, d.npass = n_seq, n_heads, Lq, Lk, dm // n_heads, npass
    d.q, d.q_seq_stride, d.ldq = q.data_ptr(), q.stride(0), q.stride(1)
    d.k, d.k_seq_stride, d.ldk = k.data_ptr(), k.stride(0), k.stride(1)
    d.v, d.v_seq_stride, d.ldv = v.data_ptr(), v.stride(0), v.stride(1)
    d.drop_p, d.drop_site, d.drop_seed = drop_p, drop_site, drop_seed
    d.io_flags = (ATTN_Q_BF16 if q.dtype == BF16 else 0) | (ATTN_KV_BF16 if k.dtype == BF16 else 0) | ((ATTN_Q_F16PAIR | ATTN_KV_F16PAIR) if planes else 0)
    assert k.dtype == v.dtype
    return d


def attn_fwd(q, k, v, n_heads, npass=3, want_probs=False, drop_p=0.0, drop_site=0, drop_seed=0, out_dtype=torch.float32, planes=False, outs=None):
    """q [n_seq, Lq, d], k/v [n_seq, Lk, d] (any row/seq strides) -> out [n_seq, Lq, d], row stats [n_seq, H, Lq, 2](, probs).
    planes (npass 2): q, k, v hold f16-pair planes (to_planes / a projection with SL_C_F16PAIR) instead of fp32 values.
    outs = (out, lse, probs): preallocated tensors to write into (out possibly strided; lse and probs contiguous; probs None without want_probs)."""
    _need_cuda(q, k, v)
    n_seq, Lq, dm = q.shape
    Lk = k.shape[1]
    if outs is not None:
        out, lse, probs = outs
        out_dtype = out.dtype
        assert lse.is_contiguous() and lse.dtype == torch.float32 and (not want_probs or (probs.is_contiguous() and probs.dtype == torch.float32))
    else:
        out = torch.empty(n_seq, Lq, dm, device=q.device, dtype=out_dtype)
        lse = torch.empty(n_seq, n_heads, Lq, 2, device=q.device)     # (row max, 1/row sum)
        probs = torch.empty(n_seq, n_heads, Lq, Lk, device=q.device) if want_probs else None
    d = _attn_desc(q, k, v, n_heads, npass, drop_p, drop_site, drop_seed, planes)
    d.out, d.o_seq_stride, d.ldo = out.data_ptr(), out.stride(0), out.stride(1)
    d.lse = lse.data_ptr()
    d.probs = probs.data_ptr() if want_probs else 0
    d.io_flags |= ATTN_O_BF16 if out_dtype == BF16 else 0
    check(lib().hftt_attn_fwd(C.byref(d), _stream(q.device)), 'attn_fwd')
    return (out, lse, probs) if want_probs else (out, lse)


def attn_bwd(q, k, v, out, lse, dout, n_heads, npass=3, drop_p=0.0, drop_site=0, drop_seed=0, dq_dtype=torch.float32, dkv_dtype=torch.float32,
             grads_out=None, planes=False):
    """grads_out = (dq, dk, dv): preallocated (possibly strided, e.g. interleaved [S, 3d]) gradient tensors to write into."""
    _need_cuda(q, k, v, out, dout)
    if grads_out is not None:
        dq, dk, dv = grads_out
        dq_dtype, dkv_dtype = dq.dtype, dk.dtype
    else:
        dq = torch.empty(q.shape, device=q.device, dtype=dq_dtype)
        dk = torch.empty(k.shape, device=q.device, dtype=dkv_dtype)
        dv = torch.empty(v.shape, device=q.device, dtype=dkv_dtype)
    d = _attn_desc(q, k, v, n_heads, npass, drop_p, drop_site, drop_seed, planes)
    d.out, d.o_seq_stride, d.ldo = out.data_ptr(), out.stride(0), out.stride(1)
    d.lse = lse.data_ptr()
    assert dout.stride() == out.stride() and dout.dtype == out.dtype
    d.dout = dout.data_ptr()
    d.io_flags |= (ATTN_O_BF16 if out.dtype == BF16 else 0) | (ATTN_DQ_BF16 if dq_dtype == BF16 else 0) | (ATTN_DKV_BF16 if dkv_dtype == BF16 else 0)
    d.dq, d.dq_seq_stride, d.lddq = dq.data_ptr(), dq.stride(0), dq.stride(1)
    d.dk, d.dk_seq_stride, d.lddk = dk.data_ptr(), dk.stride(0), dk.stride(1)
    d.dv, d.dv_seq_stride, d.lddv = dv.data_ptr(), dv.stride(0), dv.stride(1)
    check(lib().hftt_attn_bwd(C.byref(d), _stream(q.device)), 'attn_bwd')
    return dq, dk, dv


def ln_bwd(dy, r, mean, rstd, gamma, drop_p=0.0, drop_site=0, drop_seed=0, drop_dtype=torch.float32, dr_dtype=torch.float32):
    """dy may be stored as bf16 (bf16 gradient stream); dr is written as dr_dtype."""
    _need_cuda(dy, r)
    M, N = dy.shape
    L = lib()
    n_wg = L.hftt_ln_bwd_wgs(M)
    ws = torch.empty(n_wg * 2 * N, device=dy.device)
    dr = torch.empty(dy.shape, device=dy.device, dtype=dr_dtype)
    drd = torch.empty(dy.shape, device=dy.device, dtype=drop_dtype) if drop_p > 0 else None
    d = LnBwdDesc()
    d.M, d.N = M, N
    d.dy, d.r, d.mean, d.rstd, d.gamma = dy.data_ptr(), r.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr()
    d.dr, d.dr_drop = dr.data_ptr(), (drd.data_ptr() if drd is not None else 0)
    d.drop_p, d.drop_site, d.drop_seed = drop_p, drop_site, drop_seed
    d.ws = ws.data_ptr()
    d.drop_bf16 = 1 if drop_dtype == BF16 else 0
    d.io_flags = (1 if dy.dtype == BF16 else 0) | (2 if dr_dtype == BF16 else 0) | (4 if r.dtype == BF16 else 0)
    if r.dtype not in (BF16, torch.float32) or dy.dtype not in (BF16, torch.float32):
        raise HfttError('ln_bwd: dy / r must be fp32 or bf16')
    st = _stream(dy.device)
    check(L.hftt_ln_bwd(C.byref(d), st), 'ln_bwd')
    dg = torch.empty(N, device=dy.device)
    db = torch.empty(N, device=dy.device)
    check(L.hftt_ln_bwd_reduce(ws.data_ptr(), n_wg, N, dg.data_ptr(), db.data_ptr(), 0.0, st), 'ln_bwd_reduce')
    return dr, drd, dg, db


def colsum(x, beta=0.0, out=None):
    _need_cuda(x)
    rows, n = x.shape
    L = lib()
    ws = torch.empty(L.hftt_colsum_ws_bytes(rows, n) // 4 + 16, device=x.device)
    if out is None:
        out = torch.zeros(n, device=x.device)
    check(L.hftt_colsum(x.data_ptr(), rows, n, x.stride(0), out.data_ptr(), beta, ws.data_ptr(), 1 if x.dtype == BF16 else 0, _stream(x.device)), 'colsum')
    return out


def adam_step(p, g, m, v, step, lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0):
    _need_cuda(p, g, m, v)
    check(lib().hftt_adam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), step, lr, beta1, beta2, eps,
                               grad_scale, _stream(p.device)), 'adam_step')


def guard_buffers(n, device):
    """(ctl, ws) of the guarded step over n elements: the zeroed 32-byte hftt_guard_ctl as an int32[8] tensor (norm and coef are its first
    two words viewed as fp32, apply / skipped / clipped words 2, 3, 4) and the workspace of the norm's partials"""
    ctl = torch.zeros(8, dtype=torch.int32, device=device)
    ws = torch.empty(lib().hftt_grad_norm_ws_bytes(n) // 8, dtype=torch.float64, device=device)
    return ctl, ws


def grad_norm(g, ctl, ws, grad_scale=1.0, max_norm=math.inf):
    """ctl <- the verdict on || grad_scale * g ||_2 (norm, clip factor, apply / skip, counters): two launches, no host sync"""
    _need_cuda(g, ctl, ws)
    check(lib().hftt_grad_norm(g.data_ptr(), g.numel(), grad_scale, max_norm, ws.data_ptr(), ctl.data_ptr(), _stream(g.device)), 'grad_norm')


def adam_step_guarded(p, g, m, v, step, ctl, lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0, weight_decay=0.0):
    """adam_step through the verdict in ctl: skipped when the norm was not finite, g scaled by the clip factor, decoupled weight decay"""
    _need_cuda(p, g, m, v, ctl)
    check(lib().hftt_adam_step_guarded(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), step, lr, beta1, beta2, eps,
                                       grad_scale, weight_decay, ctl.data_ptr(), _stream(p.device)), 'adam_step_guarded')


def adam_group_map(entries, total, device=None):
    """The per-quad group map of the grouped step: entries = (offset, numel, group) of every parameter in the flat buffer of `total` elements
    (offsets multiples of 8, ascending, as layout.flat_offsets hands them out; total a multiple of 4).  A uint8 tensor [total / 4]: every quad
    of a parameter carries its group, a quad in the alignment gap behind a parameter carries that parameter's group.  Built on the host with
    numpy (it is index bookkeeping, not arithmetic on tensors) and copied to `device` once."""
    entries = sorted((int(o), int(k), int(gi)) for o, k, gi in entries)
    if total % 4 != 0 or not entries or entries[0][0] != 0:
        raise HfttError('adam_group_map: the flat buffer must be a multiple of 4 elements and start with a parameter')
    qmap = np.zeros(total // 4, dtype=np.uint8)
    for i, (o, k, gi) in enumerate(entries):
        end = entries[i + 1][0] if i + 1 < len(entries) else total
        if o % 4 != 0 or o + k > end or not 0 <= gi < ADAM_MAX_GROUPS:
            raise HfttError('adam_group_map: parameter at offset %d (%d elements, group %d) overlaps its neighbour, is not quad-aligned or names a group beyond %d'
                            % (o, k, gi, ADAM_MAX_GROUPS - 1))
        qmap[o // 4:end // 4] = gi
    t = torch.from_numpy(qmap)
    return t if device is None else t.to(device)


def grad_norm_groups(g, quad_group, frozen_mask, ctl, ws, grad_scale=1.0, max_norm=math.inf):
    """grad_norm with the quads of the groups in frozen_mask (bit k: group k) left out of the sum"""
    _need_cuda(g, quad_group, ctl, ws)
    if quad_group.dtype != torch.uint8 or quad_group.numel() * 4 != g.numel() or not quad_group.is_contiguous():
        raise HfttError('grad_norm_groups: the group map must be a contiguous uint8 tensor with one entry per quad of g')
    check(lib().hftt_grad_norm_groups(g.data_ptr(), g.numel(), quad_group.data_ptr(), int(frozen_mask), grad_scale, max_norm, ws.data_ptr(), ctl.data_ptr(),
                                      _stream(g.device)), 'grad_norm_groups')


def _adam_groups_desc(dsc, what, p, g, m, v, step, quad_group, lr, weight_decay, frozen, ctl, beta1, beta2, eps, grad_scale, map_optional=False):
    """fill an AdamGroupsDesc (hftt_adam_step_groups, and the `a` of hftt_adam_step_ema); quad_group None: one unfrozen group (the EMA step only)"""
    lr = [float(x) for x in lr]
    k = len(lr)
    weight_decay = [0.0] * k if weight_decay is None else [float(x) for x in weight_decay]
    frozen = [False] * k if frozen is None else [bool(x) for x in frozen]
    if len(weight_decay) != k or len(frozen) != k:
        raise HfttError('%s: lr, weight_decay and frozen must have one entry per group' % what)
    if quad_group is None:
        if not map_optional or k != 1 or frozen[0]:
            raise HfttError('%s: the group map may be left out only for one unfrozen group' % what)
    elif quad_group.dtype != torch.uint8 or quad_group.numel() * 4 != p.numel() or not quad_group.is_contiguous():
        raise HfttError('%s: the group map must be a contiguous uint8 tensor with one entry per quad of p' % what)
    dsc.p, dsc.g, dsc.m, dsc.v, dsc.n = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()
    dsc.quad_group, dsc.n_groups, dsc.step = None if quad_group is None else quad_group.data_ptr(), k, step
    dsc.beta1, dsc.beta2, dsc.eps, dsc.grad_scale = beta1, beta2, eps, grad_scale
    for i in range(min(k, ADAM_MAX_GROUPS)):
        dsc.lr[i], dsc.weight_decay[i], dsc.frozen[i] = lr[i], weight_decay[i], 1 if frozen[i] else 0
    dsc.ctl = None if ctl is None else ctl.data_ptr()


def adam_step_groups(p, g, m, v, step, quad_group, lr, weight_decay=None, frozen=None, ctl=None, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0):
    """One launch over the flat buffers with per-group constants: lr, weight_decay (decoupled) and frozen are sequences of one value per
    group (1..8 groups).  ctl: the guard record (None: unguarded).  Quads of a frozen group are neither read nor written."""
    _need_cuda(p, g, m, v, quad_group, ctl)
    dsc = AdamGroupsDesc()
    _adam_groups_desc(dsc, 'adam_step_groups', p, g, m, v, step, quad_group, lr, weight_decay, frozen, ctl, beta1, beta2, eps, grad_scale)
    check(lib().hftt_adam_step_groups(C.byref(dsc), _stream(p.device)), 'adam_step_groups')


def adam_step_ema(p, g, m, v, ema, ema_c, step, ema_decay, lr, quad_group=None, weight_decay=None, frozen=None, ctl=None, beta1=0.9, beta2=0.999,
                  eps=1e-8, grad_scale=1.0):
    """adam_step_groups with the averaged weights carried in the same launch: behind the update, e += (1 - ema_decay) (p - e) on the new p as
    a compensated fp32 sum (ema: the average, ema_c: its running compensation, both fp32 of p's length).  p, m, v end bit-identical to the
    step without the average; a skipped step and frozen quads leave ema and ema_c alone.  quad_group None: one unfrozen group (lr a
    one-element sequence) -- with ctl None that is adam_step, with ctl adam_step_guarded."""
    _need_cuda(p, g, m, v, ema, ema_c, quad_group, ctl)
    if ema.numel() != p.numel() or ema_c.numel() != p.numel() or ema.dtype != torch.float32 or ema_c.dtype != torch.float32:
        raise HfttError('adam_step_ema: ema and ema_c must be fp32 tensors of p\'s length')
    dsc = AdamEmaDesc()
    _adam_groups_desc(dsc.a, 'adam_step_ema', p, g, m, v, step, quad_group, lr, weight_decay, frozen, ctl, beta1, beta2, eps, grad_scale, map_optional=True)
    dsc.ema, dsc.ema_c, dsc.ema_decay = ema.data_ptr(), ema_c.data_ptr(), float(ema_decay)
    check(lib().hftt_adam_step_ema(C.byref(dsc), _stream(p.device)), 'adam_step_ema')


# ------------------------------------------------------------------------------------------------
# log-mel front end (model/amt.py:55-63)
# ------------------------------------------------------------------------------------------------
class LogMel:
    """Device-resident tables (hann window, FFT twiddles, sparse slaney/htk mel filterbank) + the kernel launch."""

    def __init__(self, device, sr=16000, n_fft=2048, hop=256, n_mels=256, log_offset=1e-8):
        self.device = torch.device(device)
        _need_cuda(torch.empty(0, device=self.device))
        self.sr, self.n_fft, self.hop, self.n_mels, self.log_offset = sr, n_fft, hop, n_mels, log_offset
        t = self.tables(sr, n_fft, n_mels)
        self.nnz = t['nnz']
        for name in ('window', 'twiddle', 'fb_start', 'fb_len', 'fb_off', 'fb_w'):
            setattr(self, name, t[name].to(self.device))

    @classmethod
    def tables(cls, sr=16000, n_fft=2048, n_mels=256):
        """The kernel's tables as host tensors, in the formats the device holds (no device needed): window [n_fft] and twiddle
        [cos | sin of 2 pi k / n_fft, k < n_fft / 2] fp32, the filterbank as CSR by mel (fb_start / fb_len / fb_off int32, fb_w fp32), nnz."""
        n = np.arange(n_fft, dtype=np.float64)
        window = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / n_fft)                       # periodic hann
        k = np.arange(n_fft // 2, dtype=np.float64)
        tw = np.concatenate([np.cos(2.0 * np.pi * k / n_fft), np.sin(2.0 * np.pi * k / n_fft)])
        fb = cls.mel_filterbank(sr, n_fft, n_mels)                                 # [n_freqs, n_mels] float64
        starts, lens, offs, weights = [], [], [], []
        for m in range(n_mels):
            nz = np.nonzero(fb[:, m])[0]
            if len(nz) == 0:
                starts.append(0); lens.append(0); offs.append(len(weights)); continue
            s, e = int(nz[0]), int(nz[-1]) + 1
            starts.append(s); lens.append(e - s); offs.append(len(weights))
            weights.extend(fb[s:e, m].tolist())
        return dict(window=torch.tensor(window, dtype=torch.float32), twiddle=torch.tensor(tw, dtype=torch.float32),
                    fb_start=torch.tensor(starts, dtype=torch.int32), fb_len=torch.tensor(lens, dtype=torch.int32),
                    fb_off=torch.tensor(offs, dtype=torch.int32), fb_w=torch.tensor(weights if weights else [0.0], dtype=torch.float32),
                    nnz=len(weights))

    @staticmethod
    def mel_filterbank(sr, n_fft, n_mels):
        """htk mel points, triangles on linspace(0, sr/2, n_fft/2+1), slaney area normalisation (float32 steps as
        torchaudio.functional.melscale_fbanks computes them)."""
        n_freqs = n_fft // 2 + 1
        all_freqs = np.linspace(0, sr // 2, n_freqs, dtype=np.float32)
        m_max = 2595.0 * math.log10(1.0 + (sr / 2.0) / 700.0)
        m_pts = np.linspace(0.0, m_max, n_mels + 2, dtype=np.float32)
        f_pts = (700.0 * (np.power(np.float32(10.0), m_pts / np.float32(2595.0)) - 1.0)).astype(np.float32)
        f_diff = f_pts[1:] - f_pts[:-1]
        slopes = f_pts[None, :] - all_freqs[:, None]
        down = (-1.0 * slopes[:, :-2]) / f_diff[:-1]
        up = slopes[:, 2:] / f_diff[1:]
        fb = np.maximum(0.0, np.minimum(down, up))
        enorm = 2.0 / (f_pts[2:n_mels + 2] - f_pts[:n_mels])
        return (fb * enorm[None, :]).astype(np.float64)

    def __call__(self, wave_mono):
        """wave [n_samples] fp32 at self.sr (device tensor) -> log-mel [n_frames, n_mels], n_frames = 1 + n//hop."""
        _need_cuda(wave_mono)
        wave = wave_mono.contiguous().float()
        n = wave.numel()
        n_frames = 1 + n // self.hop
        feat = torch.empty(n_frames, self.n_mels, device=self.device)
        d = LogmelDesc()
        d.wave, d.n_samples = wave.data_ptr(), n
        d.n_fft, d.hop, d.n_mels, d.n_frames = self.n_fft, self.hop, self.n_mels, n_frames
        d.window, d.twiddle = self.window.data_ptr(), self.twiddle.data_ptr()
        d.fb_start, d.fb_len, d.fb_off, d.fb_w = self.fb_start.data_ptr(), self.fb_len.data_ptr(), self.fb_off.data_ptr(), self.fb_w.data_ptr()
        d.log_offset = self.log_offset
        d.feat = feat.data_ptr()
        check(lib().hftt_logmel(C.byref(d), _stream(self.device)), 'logmel')
        return feat


def resample_geometry(sr_in, sr_out, lowpass_filter_width=6, rolloff=0.99):
    """(up, down, width) of resample_kernel_table without the table: taps = 2 * width + down"""
    g = math.gcd(int(sr_in), int(sr_out))
    down, up = int(sr_in) // g, int(sr_out) // g
    return up, down, math.ceil(lowpass_filter_width * down / (min(down, up) * rolloff))


def resample_kernel_table(sr_in, sr_out, lowpass_filter_width=6, rolloff=0.99):
    """(kernel [up, taps] float64 tensor, up, down, width) of torchaudio.transforms.Resample's defaults (Hann-windowed sinc): the published
    algorithm restated (torchaudio is absent: parity unpinned at that boundary)."""
    up, down, width = resample_geometry(sr_in, sr_out, lowpass_filter_width, rolloff)
    base = min(down, up) * rolloff
    idx = torch.arange(-width, width + down, dtype=torch.float64)[None, :] / down
    t = (torch.arange(0, -up, -1, dtype=torch.float64)[:, None] / up + idx) * base
    t = t.clamp(-lowpass_filter_width, lowpass_filter_width)
    window = torch.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t = t * math.pi
    kern = torch.where(t == 0, torch.ones_like(t), torch.sin(t) / t) * window * (base / down)
    return kern, up, down, width


_RESAMPLE_TABLES = {}


def resample(wave_mono, sr_in, sr_out):
    """wave [n] fp32 device tensor at sr_in -> [ceil(n * sr_out / sr_in)] at sr_out (hftt_resample: polyphase, fp32)."""
    _need_cuda(wave_mono)
    wave = wave_mono.contiguous().float()
    key = (int(sr_in), int(sr_out), str(wave.device))
    if key not in _RESAMPLE_TABLES:                  # (the table is a pure function of the two rates: built and uploaded once per device)
        kern, up, down, width = resample_kernel_table(sr_in, sr_out)
        _RESAMPLE_TABLES[key] = (kern.float().contiguous().to(wave.device), up, down, width)
    kd, up, down, width = _RESAMPLE_TABLES[key]
    n = wave.numel()
    n_out = -(-n * up // down)
    out = torch.empty(n_out, device=wave.device)
    d = ResampleDesc()
    d.wave, d.n_in, d.kernel = wave.data_ptr(), n, kd.data_ptr()
    d.up, d.down, d.width, d.taps = up, down, width, kd.shape[1]
    d.out, d.n_out = out.data_ptr(), n_out
    check(lib().hftt_resample(C.byref(d), _stream(wave.device)), 'resample')
    return out


# ------------------------------------------------------------------------------------------------
# the front end of audio that arrives in pieces (hftt_resample_stream; include/hftt_hip.h: streaming resampler)
def resample_stream_plan(n_in, n_done, up, down, width, closing):
    """What a stream that has received n_in input samples and produced n_done outputs does now -> (first output, count, first input sample
    to retain).  Pure host arithmetic, no device.  Output o reads inputs [(o / up) * down - width, + 2 * width + down): a live stream owns its
    first up * max(0, (n_in - width) // down) outputs (capped at ceil(n_in * up / down)), a closing one all ceil(n_in * up / down); the next
    output's window begins at (next / up) * down - width, clamped at 0 (and at n_in: nothing is kept that has not arrived)."""
    n_in, n_done, up, down, width = int(n_in), int(n_done), int(up), int(down), int(width)
    total = -(-n_in * up // down)
    ready = total if closing else min(total, up * max(0, (n_in - width) // down))
    count = max(0, ready - n_done)
    nxt = n_done + count
    return n_done, count, min(n_in, max(0, (nxt // up) * down - width))


def resample_stream_lds(up, down, width):
    """bytes of LDS that 256 outputs' input window takes (hftt_resample's and hftt_resample_stream's expression): refused beyond 64 KB"""
    return ((255 // int(up) + 1) * int(down) + 2 * int(width) + int(down)) * 4


def _segments(starts, lengths, device, extra=None):
    """flat indices of the segments starts[k] .. + lengths[k], concatenated, as a device int64 tensor (and `extra`[k] repeated over segment
    k): one small upload and three launches, whatever the number of segments"""
    lengths = np.asarray(lengths, np.int64)
    total = int(lengths.sum())
    off = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    rows = [np.asarray(starts, np.int64) - off] + ([np.asarray(extra, np.int64)] if extra is not None else [])
    tab = torch.from_numpy(np.stack(rows + [lengths])).to(device)
    rep = torch.repeat_interleave(tab[:-1], tab[-1], dim=1, output_size=total)
    idx = rep[0] + torch.arange(total, device=device)
    return (idx, rep[1]) if extra is not None else idx


def _put_segments(flat, starts, lengths, src):
    """flat[starts[k] .. + lengths[k]] = the k-th piece of src (the pieces concatenated): one indexed copy whatever the number of segments;
    one or two segments are plain slice copies, without the index table"""
    if len(starts) <= 2:
        o = 0
        for st, n in zip(starts, lengths):
            flat[st:st + n].copy_(src[o:o + n])
            o += n
    else:
        flat.index_copy_(0, _segments(starts, lengths, flat.device), src)


class ResampleStream:
    """The carried state of ``resample_stream`` for S streams at one input rate on one device: the kernel table (the _RESAMPLE_TABLES
    cache), the per-stream counters ON THE HOST (n_in samples received, n_done outputs produced, in0 the first retained input sample: a
    function of what was pushed, nothing is read back), the retained input tails (device, int16 or fp32, fewer than taps + down samples
    each) and the resampled store: fp32 [S, slot_len], slot s holds stream s's samples at sr_out from absolute index base[s] (a multiple of
    hop) on.  ``stream_logmel`` reads the store as S pseudo-files (``table``: a WetTable over the store, no copy), releases the frames that
    are complete and slides the slots, so that a slot never holds more than n_fft + hop samples behind a push; slot_len grows to the
    largest push seen (or is fixed by the caller with slot_len= / store=), never with the stream's age.  sr_in == sr_out: no kernel table
    and no resample launch, the samples go into the same store unchanged."""

    def __init__(self, S, sr_in, sr_out, device, n_fft=2048, hop=256, slot_len=None, store=None):
        self.S, self.sr_in, self.sr_out = int(S), int(sr_in), int(sr_out)
        self.n_fft, self.hop = int(n_fft), int(hop)
        if self.S < 1 or self.sr_in < 1 or self.sr_out < 1 or self.hop < 1 or self.n_fft < 2:
            raise HfttError('ResampleStream: S=%d streams from rate %d to rate %d (n_fft=%d, hop=%d)' % (self.S, self.sr_in, self.sr_out, self.n_fft, self.hop))
        same = self.sr_in == self.sr_out
        self.up, self.down, self.width = (1, 1, 0) if same else resample_geometry(self.sr_in, self.sr_out)
        self.taps = 2 * self.width + self.down
        if not same and resample_stream_lds(self.up, self.down, self.width) > 64 * 1024:
            raise HfttError('ResampleStream: input rate %d -> %d: the input window of one workgroup (down = %d, taps = %d) exceeds 64 KB of LDS'
                            % (self.sr_in, self.sr_out, self.down, self.taps))
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise HfttError('ResampleStream: a ROCm device is required (got %s); there is no CPU fallback' % self.device)
        self.kernel = None
        if not same:
            key = (self.sr_in, self.sr_out, str(self.device))
            if key not in _RESAMPLE_TABLES:
                kern = resample_kernel_table(self.sr_in, self.sr_out)[0]
                _RESAMPLE_TABLES[key] = (kern.float().contiguous().to(self.device), self.up, self.down, self.width)
            self.kernel = _RESAMPLE_TABLES[key][0]
        S = self.S
        self.n_in, self.n_done, self.in0, self.closed = [0] * S, [0] * S, [0] * S, [False] * S
        self.base, self.frames = [0] * S, [0] * S                 # slot position 0 in the stream's output timeline; log-mel frames released
        self.tail = [None] * S                                    # retained input samples in0 .. n_in (device, 1-d) or None
        self.fixed = store is not None or slot_len is not None
        if store is not None:
            _need_cuda(store)
            if store.dtype != torch.float32 or store.dim() != 2 or store.shape[0] != S or not store.is_contiguous():
                raise HfttError('ResampleStream: store must be a contiguous fp32 [S, slot_len] device tensor')
            self.store = store
        else:
            self.store = torch.zeros(S, int(slot_len) if slot_len is not None else self.n_fft + 2 * self.hop, dtype=torch.float32, device=self.device)
        self._zeros = torch.zeros(self.n_fft, dtype=torch.float32, device=self.device)
        self._tabled = None

    @property
    def slot_len(self):
        return self.store.shape[1]

    def table(self):
        """the store as clip_logmel reads a corpus: S pseudo-files of slot_len fp32 samples (a WetTable over the store itself)"""
        if self._tabled is None or self._tabled.wave is not self.store:
            samp0 = torch.arange(self.S + 1, dtype=torch.int64, device=self.device) * self.slot_len
            self._tabled = WetTable(self.store, samp0)
            self._tabled.device = self.device                    # as the caller named it ('cuda' and 'cuda:0' do not compare equal), as a WaveTable does
        return self._tabled

    def _room(self, need):
        """slot_len >= need: a larger store (the old slots copied) unless the caller fixed it"""
        if need <= self.slot_len:
            return
        if self.fixed:
            raise HfttError('resample_stream: a push needs %d samples per slot, the store has slot_len=%d' % (need, self.slot_len))
        new = torch.zeros(self.S, _align(need, 1024), dtype=torch.float32, device=self.device)
        new[:, :self.slot_len].copy_(self.store)
        self.store = new

    def read(self, s, first, count):
        """outputs first .. first + count of stream s as they lie in the store (a copy; they must not have been slid out)"""
        p = first - self.base[s]
        if p < 0 or p + count > self.slot_len:
            raise HfttError('ResampleStream.read: outputs %d .. %d of stream %d are not in its slot (base %d)' % (first, first + count, s, self.base[s]))
        return self.store[s, p:p + count].clone()

    def fill_of(self, n_out):
        """zeros behind the last sample of a closed file of n_out samples: up to the last sample its final frame n_out // hop reads"""
        return (n_out // self.hop) * self.hop + self.n_fft // 2 - n_out


def resample_stream(state, chunks, closing=None):
    """The one call of the streaming front end: chunks[s] = new samples of stream s at state.sr_in (1-d, int16 or floating point, host or
    device; None: nothing), closing[s]: the stream ends with this call.  Plans all streams (resample_stream_plan), uploads the per-stream
    table in ONE copy and launches hftt_resample_stream ONCE: every stream's new outputs go behind its earlier ones in its slot of
    state.store, a closing stream's zero tail with them.  int16 is converted by the kernel, (float)s * (1 / 32768) -- unless some stream
    brings floating point in the same call, then the int16 pieces are converted here, to the same values.  sr_in == sr_out: no launch, one
    indexed copy into the store.  -> [(first output, count)] per stream; nothing is read back."""
    if not isinstance(state, ResampleStream):
        raise HfttError('resample_stream: the first argument is an ops.ResampleStream')
    S, dev = state.S, state.device
    chunks = list(chunks)
    closing = [False] * S if closing is None else [bool(c) for c in closing]
    if len(chunks) != S or len(closing) != S:
        raise HfttError('resample_stream: %d chunks / %d closing flags for %d streams' % (len(chunks), len(closing), S))
    new = [None] * S
    for s, w in enumerate(chunks):
        if w is None:
            continue
        w = torch.as_tensor(w)
        if w.dim() != 1:
            raise HfttError('resample_stream: stream %d: samples are 1-d (mono), got shape %s' % (s, tuple(w.shape)))
        if w.dtype != torch.int16 and not w.dtype.is_floating_point:
            raise HfttError('resample_stream: stream %d: samples are int16 or floating point, got %s' % (s, w.dtype))
        if w.numel() == 0:
            continue
        if state.closed[s]:
            raise HfttError('resample_stream: stream %d is closed' % s)
        new[s] = w
    for s in range(S):
        if closing[s] and state.closed[s]:
            raise HfttError('resample_stream: stream %d is closed already' % s)
    live = [s for s in range(S) if new[s] is not None or closing[s]]
    if not live:
        return [(state.n_done[s], 0) for s in range(S)]
    # the pieces on the device, in one dtype: int16 only when every piece of the launch is int16
    pieces = [t for t in new if t is not None] + [state.tail[s] for s in range(S) if state.tail[s] is not None and state.tail[s].numel()]
    i16 = state.kernel is not None and len(pieces) > 0 and all(t.dtype == torch.int16 for t in pieces)

    def conv(t):
        if i16:
            return t
        return t.float() * (1.0 / 32768.0) if t.dtype == torch.int16 else t.float()
    host = [s for s in range(S) if new[s] is not None and new[s].device.type != 'cuda']
    if host:                                            # the host chunks travel in ONE copy
        if len({new[s].dtype for s in host}) == 1:
            sent = (torch.cat([new[s] for s in host]) if len(host) > 1 else new[host[0]]).to(dev)
            o = 0
            for s in host:
                n = new[s].numel()
                new[s] = sent[o:o + n]
                o += n
        else:
            for s in host:
                new[s] = new[s].to(dev)
    # the plan of every stream
    plan, parts, rows = [], [], np.zeros((8, S), np.int64)
    off = 0
    for s in range(S):
        n_new = new[s].numel() if new[s] is not None else 0
        state.n_in[s] += n_new
        first, count, keep = resample_stream_plan(state.n_in[s], state.n_done[s], state.up, state.down, state.width, closing[s])
        fill = state.fill_of(first + count) if closing[s] else 0
        plan.append((first, count, keep, fill))
        length = state.n_in[s] - state.in0[s]
        if state.tail[s] is not None and state.tail[s].numel():
            parts.append(conv(state.tail[s]))
        if new[s] is not None:
            parts.append(conv(new[s]))
        rows[:, s] = (off, state.in0[s], state.n_in[s], int(closing[s]), first, count, 0, fill)
        off += length
    state._room(max(p[0] - state.base[s] + p[1] + p[3] for s, p in enumerate(plan)))
    L = state.slot_len
    for s, p in enumerate(plan):
        rows[6, s] = s * L + p[0] - state.base[s]
    packed = torch.cat(parts) if len(parts) > 1 else (parts[0] if parts else None)
    max_count = max(p[1] for p in plan)
    if state.kernel is None:
        # equal rates: outputs are the inputs; the new samples and a closing stream's zeros in one indexed copy
        src, starts, lens = [], [], []
        o = 0
        for s, (first, count, keep, fill) in enumerate(plan):
            length = state.n_in[s] - state.in0[s]
            if count:
                src.append(packed[o + length - count:o + length])
            if fill:
                src.append(state._zeros[:fill] if fill <= state._zeros.numel() else torch.zeros(fill, device=dev))
            if count + fill:
                starts.append(int(rows[6, s])); lens.append(count + fill)
            o += length
        if src:
            _put_segments(state.store.view(-1), starts, lens, torch.cat(src) if len(src) > 1 else src[0])
    elif max_count > 0 or any(p[3] for p in plan):
        if packed is None:                              # (a close of streams that hold nothing: a pointer that is only non-null)
            packed = state._zeros[:1]
        tab = torch.from_numpy(rows).to(dev)
        d = ResampleStreamDesc()
        d.wave, d.wave_len, d.kernel, d.tab = packed.data_ptr(), (packed.numel() if parts else 0), state.kernel.data_ptr(), tab.data_ptr()
        d.store, d.store_len, d.max_count = state.store.data_ptr(), state.store.numel(), max_count
        d.S, d.up, d.down, d.width, d.taps, d.wave_i16 = S, state.up, state.down, state.width, state.taps, int(i16)
        check(lib().hftt_resample_stream(C.byref(d), _stream(dev)), 'resample_stream')
    # the counters, and the tails as views of this call's packed input
    out, o = [], 0
    for s, (first, count, keep, fill) in enumerate(plan):
        length = state.n_in[s] - state.in0[s]
        state.n_done[s] = first + count
        state.closed[s] = state.closed[s] or closing[s]
        if state.closed[s]:                             # nothing of a closed stream is read again
            keep = state.n_in[s]
        state.tail[s] = packed[o + keep - state.in0[s]:o + length] if keep < state.n_in[s] else None
        state.in0[s] = keep
        out.append((first, count))
        o += length
    return out


def stream_frames_plan(n_done, frames, closed, hop, n_fft):
    """log-mel frames first .. end that a stream with n_done resampled samples completes: frame t once samples through t * hop + n_fft / 2
    - 1 exist; a closed stream all 1 + n_done // hop.  -> (first, end), end >= first.  Pure host arithmetic."""
    end = 1 + n_done // hop if closed else ((n_done - n_fft // 2) // hop + 1 if n_done >= n_fft // 2 else 0)
    return frames, max(frames, end)


def stream_logmel(state, logmel):
    """The log-mel frames that the streams of `state` (an ops.ResampleStream) have completed since the last call, ALL streams in ONE
    hftt_clip_logmel launch over the resampled store: every stream's new frames are requested as windows of HFTT_CLIP_LOGMEL_RUN = 16 frames
    of its pseudo-file, the padding frames of a stream's last window are discarded.  Then the slots slide (one batched indexed copy): what
    lies in front of the next frame's first sample is dropped.  -> per stream a [n, n_mels] fp32 device tensor or None."""
    if not isinstance(state, ResampleStream):
        raise HfttError('stream_logmel: the first argument is an ops.ResampleStream')
    if logmel.hop != state.hop or logmel.n_fft != state.n_fft:
        raise HfttError('stream_logmel: the LogMel has n_fft=%d, hop=%d, the stream n_fft=%d, hop=%d' % (logmel.n_fft, logmel.hop, state.n_fft, state.hop))
    S, hop, W = state.S, state.hop, 16
    wf, ws, spans = [], [], [None] * S
    for s in range(S):
        t0, t1 = stream_frames_plan(state.n_done[s], state.frames[s], state.closed[s], hop, state.n_fft)
        if t1 > t0:
            spans[s] = (len(wf) * W, t1 - t0)
            for t in range(t0, t1, W):
                wf.append(s); ws.append(t - state.base[s] // hop)
            state.frames[s] = t1
    out = [None] * S
    if wf:
        win = torch.tensor([wf, ws], dtype=torch.int32).to(state.device)
        spec = clip_logmel(state.table(), logmel, win[0], win[1], W, 0.0)               # [B, n_mels, 16]
        rows = spec.permute(0, 2, 1).reshape(len(wf) * W, logmel.n_mels)
        for s in range(S):
            if spans[s] is not None:
                out[s] = rows[spans[s][0]:spans[s][0] + spans[s][1]]
    resample_stream_slide(state)
    return out


def resample_stream_slide(state):
    """Drop from every slot what no later frame reads: slot position 0 moves to the multiple of hop at or below the next frame's first
    sample, frames * hop - n_fft / 2.  One batched indexed copy for all streams (the retained pieces are at most n_fft + hop samples each)."""
    S, L, hop = state.S, state.slot_len, state.hop
    starts, lens, shifts = [], [], []
    for s in range(S):
        keep = max(state.base[s], (state.frames[s] * hop - state.n_fft // 2) // hop * hop, 0)
        shift = keep - state.base[s]
        if shift == 0 or state.closed[s]:
            continue
        n = max(0, state.n_done[s] - keep)
        if n:
            starts.append(s * L + shift); lens.append(n); shifts.append(shift)
        state.base[s] = keep
    flat = state.store.view(-1)
    if 0 < len(starts) <= 2:                            # (slice copies, the source cloned: the two ranges may overlap)
        for st, n, sh in zip(starts, lens, shifts):
            flat[st - sh:st - sh + n].copy_(flat[st:st + n].clone())
    elif starts:
        src, shift = _segments(starts, lens, state.device, extra=shifts)
        flat.index_copy_(0, src - shift, flat.index_select(0, src))


# ------------------------------------------------------------------------------------------------
# note decoding on the device (model/amt.py transcript / transcript_stride / mpe2note; csrc/notes.hip)
# ------------------------------------------------------------------------------------------------
MODE_VELOCITY = {'ignore_zero': 0, 'org': 1}
MODE_OFFSET = {'shorter': 0, 'longer': 1, 'offset': 2}


def stitch(onset, offset, mpe, velocity, rolls, dst, src0=0, length=None):
    """One model call's outputs -> the file-long rolls (hftt_stitch).  onset / offset / mpe [b, T, N] fp32 and velocity [b, T, N, V] fp32 logits
    (device tensors); rolls = (onset, offset, mpe fp32 [F, N], velocity int8 [F, N]) device tensors, written in place: rows src0 .. src0 + length
    of clip c go to rows dst[c] .. dst[c] + length, the velocity roll receives the argmax over V.  dst: b ints (host)."""
    _need_cuda(onset, offset, mpe, velocity, *rolls)
    b, T, N = onset.shape
    V = velocity.shape[3]
    length = T if length is None else int(length)
    srcs = [t if t.is_contiguous() else t.contiguous() for t in (onset, offset, mpe, velocity)]
    for t, shape in zip(srcs, ((b, T, N),) * 3 + ((b, T, N, V),)):
        if t.dtype != torch.float32 or tuple(t.shape) != shape:
            raise HfttError('stitch: the model outputs must be fp32 [b, T, N] and [b, T, N, V]')
    F = rolls[0].shape[0]
    for t, dt in zip(rolls, (torch.float32,) * 3 + (torch.int8,)):
        if t.dtype != dt or tuple(t.shape) != (F, N) or not t.is_contiguous():
            raise HfttError('stitch: the rolls must be contiguous [F, N] tensors, three fp32 and one int8')
    dst = [int(x) for x in dst]
    if len(dst) != b:
        raise HfttError('stitch: %d first rows for %d clips' % (len(dst), b))
    L = lib()
    for c0 in range(0, b, STITCH_MAX_CLIPS):
        nb = min(STITCH_MAX_CLIPS, b - c0)
        d = StitchDesc()
        d.b, d.T, d.N, d.V, d.src0, d.len, d.F = nb, T, N, V, int(src0), length, F
        d.onset, d.offset, d.mpe, d.velocity = (t[c0:c0 + nb].data_ptr() for t in srcs)
        d.roll_onset, d.roll_offset, d.roll_mpe, d.roll_velocity = (t.data_ptr() for t in rolls)
        host_dst = (C.c_int32 * nb)(*dst[c0:c0 + nb])
        d.dst = host_dst
        check(L.hftt_stitch(C.byref(d), _stream(onset.device)), 'stitch')
    return rolls


def _notes_fill(d, onset, offset, mpe, velocity, thred_onset, thred_offset, thred_mpe, hop_sec, note_min, mode_velocity, mode_offset, cap, what):
    """the fields of a NotesDesc but the outputs and the workspace; returns the bytes of the packed output buffer (int8): [n_notes int32, pad
    to 8 | onset double cap | offset double cap | pitch int32 cap | velocity int32 cap], so that the caller fetches the compact list with a
    single copy (_notes_outputs points the descriptor into it)"""
    _need_cuda(onset, offset, mpe, velocity)
    if mode_velocity not in MODE_VELOCITY or mode_offset not in MODE_OFFSET:
        raise HfttError('%s: mode_velocity %r / mode_offset %r unknown' % (what, mode_velocity, mode_offset))
    F, N = onset.shape
    for t, dt in ((onset, torch.float32), (offset, torch.float32), (mpe, torch.float32), (velocity, torch.int8)):
        if t.dtype != dt or tuple(t.shape) != (F, N) or not t.is_contiguous():
            raise HfttError('%s: the rolls must be contiguous [F, N] tensors, three fp32 and one int8' % what)
    d.F, d.N, d.note_min = F, N, int(note_min)
    d.onset, d.offset, d.mpe, d.velocity = onset.data_ptr(), offset.data_ptr(), mpe.data_ptr(), velocity.data_ptr()
    # the host compares a float32 roll with a Python scalar: the scalar is rounded to float32 (NumPy 2 promotion)
    d.thred_onset, d.thred_offset, d.thred_mpe = float(np.float32(thred_onset)), float(np.float32(thred_offset)), float(np.float32(thred_mpe))
    d.mode_velocity, d.mode_offset, d.cap = MODE_VELOCITY[mode_velocity], MODE_OFFSET[mode_offset], cap
    d.hop_sec = float(hop_sec)
    return 8 + 24 * cap


def _notes_outputs(d, base, cap):
    d.n_notes = base
    d.out_onset, d.out_offset, d.out_pitch, d.out_velocity = base + 8, base + 8 + 8 * cap, base + 8 + 16 * cap, base + 8 + 20 * cap


def _notes_packed(onset, offset, mpe, velocity, thred_onset, thred_offset, thred_mpe, hop_sec, note_min, mode_velocity, mode_offset, cap):
    """hftt_notes_decode into ONE device buffer (_notes_fill)"""
    d = NotesDesc()
    nbytes = _notes_fill(d, onset, offset, mpe, velocity, thred_onset, thred_offset, thred_mpe, hop_sec, note_min, mode_velocity, mode_offset, cap, 'notes_decode')
    L = lib()
    dev = onset.device
    ws_bytes = L.hftt_notes_ws_bytes(d.F, d.N)
    ws = torch.empty(ws_bytes, dtype=torch.int8, device=dev)
    buf = torch.empty(nbytes, dtype=torch.int8, device=dev)
    _notes_outputs(d, buf.data_ptr(), cap)
    d.ws, d.ws_bytes = ws.data_ptr(), ws_bytes
    check(L.hftt_notes_decode(C.byref(d), _stream(dev)), 'notes_decode')
    return buf


def _notes_unpack(buf, cap):
    """views of the packed buffer (device or host): total, onset, offset, pitch, velocity"""
    total = int(buf[:4].view(torch.int32)[0])
    n = min(total, cap)
    onset = buf[8:8 + 8 * cap].view(torch.float64)[:n]
    offset = buf[8 + 8 * cap:8 + 16 * cap].view(torch.float64)[:n]
    pitch = buf[8 + 16 * cap:8 + 20 * cap].view(torch.int32)[:n]
    velocity = buf[8 + 20 * cap:8 + 24 * cap].view(torch.int32)[:n]
    return total, onset, offset, pitch, velocity


def notes_default_capacity(F, N):
    """room for the notes of a first call: every frame of every pitch can be a note (N * F), real files hold far fewer"""
    return min(N * F, max(4096, N * F // 32))


def notes_decode(onset, offset, mpe, velocity, hop_sec, note_min=21, thred_onset=0.5, thred_offset=0.5, thred_mpe=0.5,
                 mode_velocity='ignore_zero', mode_offset='shorter', capacity=None, host=False):
    """The rolls of one file (device tensors: onset / offset / mpe fp32 [F, N], velocity int8 [F, N]) -> (pitch int32, velocity int32, onset
    float64, offset float64), the notes of AMT.mpe2note in front of its final sort: pitch-major, ascending onset frame (hftt_notes_decode).
    The wrapper sizes the workspace and the capacity; when more notes exist than fit it runs once more with the exact count -- unless the caller
    fixed capacity=, then it raises HfttError.  host=True: the four arrays come back as host tensors, fetched with one copy of the packed list."""
    _need_cuda(onset, offset, mpe, velocity)
    F, N = onset.shape
    cap = notes_default_capacity(F, N) if capacity is None else int(capacity)
    args = (onset, offset, mpe, velocity, thred_onset, thred_offset, thred_mpe, hop_sec, note_min, mode_velocity, mode_offset)
    buf = _notes_packed(*args, cap)
    if host:
        buf = buf.cpu()
    total, t_on, t_off, pitch, vel = _notes_unpack(buf, cap)
    if total > cap:
        if capacity is not None:
            raise HfttError('notes_decode: %d notes exist, capacity=%d' % (total, cap))
        cap = total
        buf = _notes_packed(*args, cap)
        if host:
            buf = buf.cpu()
        total, t_on, t_off, pitch, vel = _notes_unpack(buf, cap)
    return pitch, vel, t_on, t_off


def _notes_seg_packed(rolls, seg_host, seg_dev, args, cap):
    """hftt_notes_decode_seg into ONE device buffer: the list of _notes_fill, then seg_notes int32 [n_seg + 1] behind it"""
    s = NotesSegDesc()
    nbytes = _notes_fill(s.notes, *rolls, *args, cap, 'notes_decode_seg')
    n_seg = len(seg_host) - 1
    L = lib()
    dev = rolls[0].device
    ws_bytes = L.hftt_notes_seg_ws_bytes(s.notes.F, s.notes.N, n_seg)
    ws = torch.empty(ws_bytes, dtype=torch.int8, device=dev)
    buf = torch.empty(nbytes + 4 * (n_seg + 1), dtype=torch.int8, device=dev)
    _notes_outputs(s.notes, buf.data_ptr(), cap)
    s.notes.ws, s.notes.ws_bytes = ws.data_ptr(), ws_bytes
    s.n_seg = n_seg
    table = (C.c_int32 * (n_seg + 1))(*seg_host)
    s.seg_row0_host = table
    s.seg_row0 = seg_dev.data_ptr()
    s.seg_notes = buf.data_ptr() + nbytes
    check(L.hftt_notes_decode_seg(C.byref(s), _stream(dev)), 'notes_decode_seg')
    return buf


def notes_decode_seg(onset, offset, mpe, velocity, seg_rows, hop_sec, note_min=21, thred_onset=0.5, thred_offset=0.5, thred_mpe=0.5,
                     mode_velocity='ignore_zero', mode_offset='shorter', capacity=None, host=False):
    """Rolls that hold n_seg files back to back (device tensors as for notes_decode) -> (pitch, velocity, onset, offset, seg_notes): every
    segment's notes are those of notes_decode on its rows alone, segment-major; segment s is records seg_notes[s] .. seg_notes[s + 1]
    (hftt_notes_decode_seg).  seg_rows: the n_seg + 1 row borders on the host (ints; [0] == 0, non-decreasing, [-1] == F), uploaded here.
    The capacity rule is notes_decode's: notes_default_capacity(F, N), one rerun with the exact count on overflow, HfttError when the caller
    fixed capacity=.  All five arrays lie in one packed buffer: host=True is ONE device->host copy."""
    _need_cuda(onset, offset, mpe, velocity)
    F, N = onset.shape
    seg_host = [int(x) for x in seg_rows]
    if len(seg_host) < 1:
        raise HfttError('notes_decode_seg: seg_rows needs n_seg + 1 row borders')
    n_seg = len(seg_host) - 1
    seg_dev = torch.tensor(seg_host, dtype=torch.int32).to(onset.device)
    cap = notes_default_capacity(F, N) if capacity is None else int(capacity)
    args = (thred_onset, thred_offset, thred_mpe, hop_sec, note_min, mode_velocity, mode_offset)
    rolls = (onset, offset, mpe, velocity)

    def run(cap):
        buf = _notes_seg_packed(rolls, seg_host, seg_dev, args, cap)
        if host:
            buf = buf.cpu()
        return _notes_unpack(buf, cap) + (buf[8 + 24 * cap:8 + 24 * cap + 4 * (n_seg + 1)].view(torch.int32),)
    total, t_on, t_off, pitch, vel, seg_notes = run(cap)
    if total > cap:
        if capacity is not None:
            raise HfttError('notes_decode_seg: %d notes exist, capacity=%d' % (total, cap))
        total, t_on, t_off, pitch, vel, seg_notes = run(total)
    return pitch, vel, t_on, t_off, seg_notes


class NotesStreamState:
    """What hftt_notes_stream_step works on, for S streams on one device: the four rolls as rings of H rows ([S, H, N], fp32 x3 and int8; row
    r of a stream lives at ring row r % H), the device tables row_end int64 [S] / closed int32 [S], the zero-initialised state buffer, and
    the host's copy of the tables.  The producer writes rows into the rings (stitch on ``rings_flat``: stream s row r = flat row s * H +
    r % H) and then calls ``deliver``."""

    def __init__(self, S, N, H, device):
        S, N, H = int(S), int(N), int(H)
        nbytes = lib().hftt_notes_stream_state_bytes(S, N)
        if nbytes <= 0 or H < 4:
            raise HfttError('notes_stream_state: S=%d streams of N=%d notes (1..128) with H=%d ring rows (>= 4)' % (S, N, H))
        self.S, self.N, self.H, self.device = S, N, H, torch.device(device)
        if self.device.type != 'cuda':
            raise HfttError('notes_stream_state: a ROCm device is required (got %s); there is no CPU fallback' % self.device)
        self.rings = tuple(torch.zeros(S, H, N, dtype=torch.int8 if k == 3 else torch.float32, device=self.device) for k in range(4))
        self.rings_flat = tuple(t.view(S * H, N) for t in self.rings)
        self.state = torch.zeros(nbytes, dtype=torch.int8, device=self.device)
        self.tables = torch.zeros(3 * S, dtype=torch.int32, device=self.device)        # row_end as int64 [S], then closed int32 [S]
        self.row_end, self.closed = [0] * S, [False] * S
        self.max_new = 0

    def deliver(self, new_rows, close=None):
        """new_rows[s] rows were written behind row_end[s]; close[s]: stream s has ended.  One small upload."""
        close = [False] * self.S if close is None else list(close)
        for s, n in enumerate(new_rows):
            n = int(n)
            if n < 0 or (n > 0 and self.closed[s]):
                raise HfttError('notes_stream: stream %d: %d new rows for a %s stream' % (s, n, 'closed' if self.closed[s] else 'live'))
            self.row_end[s] += n
            self.max_new = max(self.max_new, n)
            self.closed[s] = self.closed[s] or bool(close[s])
        host = np.concatenate([np.asarray(self.row_end, np.int64).view(np.int32), np.asarray(self.closed, np.int32)])
        self.tables.copy_(torch.from_numpy(host))


def notes_stream_state(S, N, H, device):
    """the rings, the tables and the zeroed state of S fresh streams (NotesStreamState)"""
    return NotesStreamState(S, N, H, device)


def _notes_stream_packed(st, args, cap):
    """hftt_notes_stream_step into ONE device buffer: [n_notes int32 | stream_notes int32 [S + 1] | overflow int32 [S] | pad to 8 | onset
    double cap | offset double cap | pitch int32 cap | velocity int32 cap]"""
    thred_onset, thred_offset, thred_mpe, hop_sec, note_min, mode_velocity, mode_offset = args
    if mode_velocity not in MODE_VELOCITY or mode_offset not in MODE_OFFSET:
        raise HfttError('notes_stream_step: mode_velocity %r / mode_offset %r unknown' % (mode_velocity, mode_offset))
    S = st.S
    head = _align(4 * (2 * S + 2), 8)
    buf = torch.empty(head + 24 * cap, dtype=torch.int8, device=st.device)
    d = NotesStreamDesc()
    d.S, d.N, d.H, d.note_min = S, st.N, st.H, int(note_min)
    d.onset, d.offset, d.mpe, d.velocity = (t.data_ptr() for t in st.rings)
    d.row_end, d.closed = st.tables.data_ptr(), st.tables.data_ptr() + 8 * S
    d.thred_onset, d.thred_offset, d.thred_mpe = float(np.float32(thred_onset)), float(np.float32(thred_offset)), float(np.float32(thred_mpe))
    d.mode_velocity, d.mode_offset, d.cap, d.max_new = MODE_VELOCITY[mode_velocity], MODE_OFFSET[mode_offset], cap, st.max_new
    d.hop_sec = float(hop_sec)
    d.state, d.state_bytes = st.state.data_ptr(), st.state.numel()
    base = buf.data_ptr()
    d.n_notes, d.stream_notes, d.overflow = base, base + 4, base + 4 * (S + 2)
    d.out_onset, d.out_offset, d.out_pitch, d.out_velocity = base + head, base + head + 8 * cap, base + head + 16 * cap, base + head + 20 * cap
    check(lib().hftt_notes_stream_step(C.byref(d), _stream(st.device)), 'notes_stream_step')
    return buf, head


def notes_stream_default_capacity(S, N):
    """room for the notes of one step: a step returns what became final, a handful per stream; a long plateau that ends returns more and the
    wrapper then repeats the step"""
    return max(1024, 4 * S * N)


def notes_stream_step(st, hop_sec, note_min=21, thred_onset=0.5, thred_offset=0.5, thred_mpe=0.5, mode_velocity='ignore_zero',
                      mode_offset='shorter', capacity=None, host=True):
    """One step of S streams (hftt_notes_stream_step) on what ``st.deliver`` announced: -> (pitch int32, velocity int32, onset float64, offset
    float64, stream_notes int32 [S + 1], overflow int32 [S]).  The notes are those that no later row can change, stream-major, pitch-major,
    by ascending onset frame; stream s owns records stream_notes[s] .. stream_notes[s + 1].  Over all steps of a stream, the closing one
    included, they are exactly the notes of notes_decode on the whole rolls.  mode_offset must be 'shorter'.  When more notes are final than
    fit, the state is untouched and the wrapper repeats the step with the exact count -- unless the caller fixed capacity=, then it raises
    HfttError (and the step can be repeated).  All arrays lie in one packed buffer: host=True is ONE device->host copy per step."""
    if not isinstance(st, NotesStreamState):
        raise HfttError('notes_stream_step: the first argument is the NotesStreamState of notes_stream_state()')
    cap = notes_stream_default_capacity(st.S, st.N) if capacity is None else int(capacity)
    args = (thred_onset, thred_offset, thred_mpe, hop_sec, note_min, mode_velocity, mode_offset)

    def run(cap):
        buf, head = _notes_stream_packed(st, args, cap)
        if host:
            buf = buf.cpu()
        ints = buf[:4 * (2 * st.S + 2)].view(torch.int32)
        total = int(ints[0])
        n = total if total <= cap else 0
        t_on = buf[head:head + 8 * cap].view(torch.float64)[:n]
        t_off = buf[head + 8 * cap:head + 16 * cap].view(torch.float64)[:n]
        pitch = buf[head + 16 * cap:head + 20 * cap].view(torch.int32)[:n]
        vel = buf[head + 20 * cap:head + 24 * cap].view(torch.int32)[:n]
        return total, (pitch, vel, t_on, t_off, ints[1:st.S + 2], ints[st.S + 2:2 * st.S + 2])
    total, out = run(cap)
    if total > cap:
        if capacity is not None:
            raise HfttError('notes_stream_step: %d notes are final, capacity=%d (the state is untouched: repeat the step with more room)' % (total, cap))
        total, out = run(total)
    st.max_new = 0
    return out


def clip_windows(feature, file_row0, win_file, win_start, width, fill):
    """B clip windows of a file list -> [B, n_bins, width] fp32 in ONE launch (hftt_clip_windows): feature [R, n_bins] fp32 holds the files'
    rows concatenated (device tensor), file f = rows file_row0[f] .. file_row0[f + 1]; window b shows frames win_start[b] .. + width of file
    win_file[b], counted from the file's frame 0, transposed (model/amt.py a_input[i:i+width].T); frames outside the file are `fill`, a
    neighbouring file's frames never show.  file_row0 / win_file / win_start: int32 device tensors (or anything torch.as_tensor takes)."""
    _need_cuda(feature)
    dev = feature.device
    if feature.dim() != 2 or feature.dtype != torch.float32 or not feature.is_contiguous():
        raise HfttError('clip_windows: feature must be a contiguous fp32 [R, n_bins] tensor')
    file_row0, win_file, win_start = (torch.as_tensor(t, device=dev).to(torch.int32).contiguous() for t in (file_row0, win_file, win_start))
    if file_row0.dim() != 1 or file_row0.numel() < 1 or win_file.dim() != 1 or win_start.shape != win_file.shape:
        raise HfttError('clip_windows: file_row0 must be [n_files + 1], win_file and win_start [B]')
    R, n_bins = feature.shape
    B, width = win_file.numel(), int(width)
    keep = feature if R else torch.empty(1, dtype=torch.float32, device=dev)          # no row: nothing is read, the pointer is only non-null
    out = torch.empty((B, n_bins, max(width, 0)), dtype=torch.float32, device=dev)    # an empty request is the library's to refuse
    d = ClipWindowsDesc()
    d.feature, d.file_row0, d.win_file, d.win_start, d.out = (t.data_ptr() for t in (keep, file_row0, win_file, win_start, out))
    d.B, d.width, d.n_bins, d.n_files, d.R, d.fill = B, width, n_bins, file_row0.numel() - 1, R, float(fill)
    check(lib().hftt_clip_windows(C.byref(d), _stream(dev)), 'clip_windows')
    return out


# ------------------------------------------------------------------------------------------------
# Clip log-mel (hftt_clip_logmel): the corpus keeps the WAVEFORMS, a batch's spectrogram windows are computed when it is gathered
WAVE_DTYPES = {'int16': torch.int16, 'float32': torch.float32}


class WaveTable:
    """The waveform corpus of clip_logmel on one device, uploaded once: the files' samples (1-d arrays / tensors at the feature rate, int16 or
    floating point) concatenated without padding as `dtype` ('int16': 2 bytes per sample, value s / 32768; 'float32'), and file_samp0 int64
    [n_files + 1].  Floating-point samples stored as int16 are round(x * 32768) clipped to the int16 range; int16 samples stored as float32
    are s / 32768 (exact)."""

    def __init__(self, waves, device, dtype='int16'):
        if dtype not in WAVE_DTYPES:
            raise HfttError('WaveTable: dtype %r (int16 / float32)' % (dtype,))
        if len(waves) < 1:
            raise HfttError('WaveTable: no files')
        self.device = torch.device(device)
        self.dtype = dtype
        parts = []
        for i, w in enumerate(waves):
            w = torch.as_tensor(w)
            if w.dim() != 1:
                raise HfttError('WaveTable: file %d: a waveform is 1-d (mono), got shape %s' % (i, tuple(w.shape)))
            if w.dtype == torch.int16:
                parts.append(w if dtype == 'int16' else w.float() * (1.0 / 32768.0))
            elif w.dtype.is_floating_point:
                parts.append(w.float() if dtype == 'float32' else torch.round(w.double() * 32768.0).clamp(-32768, 32767).to(torch.int16))
            else:
                raise HfttError('WaveTable: file %d: samples are int16 or floating point, got %s' % (i, w.dtype))
        self.file_nsamp_host = np.array([p.numel() for p in parts], np.int64)
        samp0 = np.concatenate([[0], np.cumsum(self.file_nsamp_host)]).astype(np.int64)
        self.n_files, self.total_samples = len(parts), int(samp0[-1])
        wave = torch.cat(parts) if self.total_samples else torch.zeros(1, dtype=WAVE_DTYPES[dtype])      # (a pointer that is only non-null)
        self.wave = wave.contiguous().to(self.device)
        self.file_samp0 = torch.from_numpy(samp0).to(self.device)

    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in (self.wave, self.file_samp0))


def warp_table_host():
    """the prototype of hftt_wave_warp's filter as fp32 [WARP_TABLE_LEN]: sinc(u) cos^2(pi u / 2Z) at u = e / L, e = 0 .. Z L, in fp64, rounded
    once; the two entries behind u = Z are exact zeros"""
    Z, L = WARP_ZEROS, WARP_TABLE_L
    u = np.arange(WARP_TABLE_LEN, dtype=np.float64) / L
    t = np.sinc(u) * np.cos(np.pi * u / (2 * Z)) ** 2
    t[Z * L:] = 0.0
    return t.astype(np.float32)


class WarpTable:
    """the prototype table of the warp kernels on one device (uploaded once)"""

    def __init__(self, device):
        self.device = torch.device(device)
        self.proto = torch.from_numpy(warp_table_host()).to(self.device)


_WARP_TABLES = {}


def warp_table(device):
    """the WarpTable of `device`, built at the first call"""
    key = str(torch.device(device))
    if key not in _WARP_TABLES:
        _WARP_TABLES[key] = WarpTable(device)
    return _WARP_TABLES[key]


class Warp:
    """The warp of B windows as device tensors: step_q24 int32 [B] (rate * 2^24), delay_q24 int64 [B] (source samples * 2^24) and shift int32
    [B] (semitones the labels move by; None = 0).  What the kernels take besides is derived here, on the device, and nowhere else:
        cut      fp32   (float)(0.99 * min(1, 2^24 / step))          the quotient and the product in fp64, rounded once to fp32
        t_scale  fp64   2^24 / step
        t_delay  fp64   delay / 2^24 / sr                            (the first quotient is exact)"""

    def __init__(self, step_q24, delay_q24, shift=None):
        self.step_q24 = torch.as_tensor(step_q24).to(torch.int32).contiguous()
        dev = self.step_q24.device
        self.delay_q24 = torch.as_tensor(delay_q24, device=dev).to(torch.int64).contiguous()
        self.shift = (torch.zeros_like(self.step_q24) if shift is None else torch.as_tensor(shift, device=dev).to(torch.int32).contiguous())
        if self.step_q24.dim() != 1 or self.delay_q24.shape != self.step_q24.shape or self.shift.shape != self.step_q24.shape:
            raise HfttError('Warp: step_q24, delay_q24 and shift must be [B]')

    def cut(self):
        return (0.99 * torch.clamp(float(1 << 24) / self.step_q24.double(), max=1.0)).float()

    def t_scale(self):
        return float(1 << 24) / self.step_q24.double()

    def t_delay(self, sr):
        return self.delay_q24.double() / float(1 << 24) / float(sr)

    def _holds(self, what, B, dev):
        if self.step_q24.device != dev or self.step_q24.numel() != B:
            raise HfttError('%s: the warp holds %d windows on %s, the request %d on %s' % (what, self.step_q24.numel(), self.step_q24.device, B, dev))

    def _args(self, what, B, dev):
        """(WarpArgs, the tensors it points to) for a launch on `dev` with B windows"""
        self._holds(what, B, dev)
        _need_cuda(self.step_q24, self.delay_q24)
        cut, proto = self.cut().contiguous(), warp_table(dev).proto
        a = WarpArgs()
        a.step_q24, a.delay_q24 = self.step_q24.data_ptr(), self.delay_q24.data_ptr()
        a.cut, a.proto = cut.data_ptr(), proto.data_ptr()
        return a, (cut, proto)

    def _label_map(self, what, B, dev, table):
        """(shift, t_delay, t_scale), to keep alive: the label map of `table` (a LabelsTable) for a launch on `dev` with B windows"""
        self._holds(what, B, dev)
        ts = (self.shift, self.t_delay(table.sr).contiguous(), self.t_scale().contiguous())
        _need_cuda(*ts, table.file_end_sec)
        return ts


def wave_warp(table, win_file, win_start, length, warp):
    """B windows of `length` WARPED samples of a waveform corpus -> fp32 [B, length] in ONE launch (hftt_wave_warp): window b shows warped
    samples win_start[b] .. + length (int64, counted from the warped file's sample 0) of file win_file[b] of `table` (a WaveTable) under
    `warp` (a Warp), before gain and noise; zeros outside the warped file.  No CPU fallback."""
    dev = table.device
    win_file = torch.as_tensor(win_file, device=dev).to(torch.int32).contiguous()
    win_start = torch.as_tensor(win_start, device=dev).to(torch.int64).contiguous()
    if not isinstance(warp, Warp):
        raise HfttError('wave_warp: warp must be an ops.Warp')
    if win_file.dim() != 1 or win_start.shape != win_file.shape:
        raise HfttError('wave_warp: win_file and win_start must be [B]')
    B, length = win_file.numel(), int(length)
    wa, keep = warp._args('wave_warp', B, dev)
    _need_cuda(table.wave, table.file_samp0, win_file, win_start)
    out = torch.empty((B, max(length, 0)), dtype=torch.float32, device=dev)
    d = WaveWarpDesc()
    d.wave, d.file_samp0, d.win_file, d.win_start = table.wave.data_ptr(), table.file_samp0.data_ptr(), win_file.data_ptr(), win_start.data_ptr()
    d.total_samples, d.wave_i16, d.n_files, d.B, d.len = table.total_samples, int(table.dtype == 'int16'), table.n_files, B, length
    d.warp, d.out = wa, out.data_ptr()
    check(lib().hftt_wave_warp(C.byref(d), _stream(dev)), 'wave_warp')
    return out


class Mix:
    """The PARTNERS of B windows (clip mixing) as device tensors: file int32 [B] (an index outside 0 .. n_files: the window has no partner),
    start int32 [B] (the partner frame that column 0 shows, counted in the partner's own -- warped -- file), gain fp32 [B], and warp: the
    partners' own ops.Warp or None (played back as they are)."""

    def __init__(self, file, start, gain, warp=None):
        if warp is not None and not isinstance(warp, Warp):
            raise HfttError('Mix: warp must be an ops.Warp')
        self.file = torch.as_tensor(file).to(torch.int32).contiguous()
        dev = self.file.device
        self.start = torch.as_tensor(start, device=dev).to(torch.int32).contiguous()
        self.gain = torch.as_tensor(gain, device=dev).to(torch.float32).contiguous()
        self.warp = warp
        if self.file.dim() != 1 or self.start.shape != self.file.shape or self.gain.shape != self.file.shape:
            raise HfttError('Mix: file, start and gain must be [B]')
        if warp is not None and (warp.step_q24.shape != self.file.shape or warp.step_q24.device != dev):
            raise HfttError('Mix: the warp holds %d windows on %s, the partners %d on %s' % (warp.step_q24.numel(), warp.step_q24.device, self.file.numel(), dev))

    def _check(self, what, B, dev):
        if self.file.device != dev or self.file.numel() != B:
            raise HfttError('%s: the mix holds %d windows on %s, the request %d on %s' % (what, self.file.numel(), self.file.device, B, dev))
        _need_cuda(self.file, self.start, self.gain)


def _identity_warp(B, dev):
    return Warp(torch.full((B,), 1 << 24, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int64, device=dev))


def audio_frames(table, hop, win_file, warp=None):
    """int64 [B] on the device: the AUDIO frame count 1 + n' / hop of each window's file of `table` (a WaveTable) as clip_logmel sees it -- n' the
    file's samples, under `warp` (an ops.Warp or None) the warped file's -- and 0 for a window without a valid file or warp.  What
    labels_render takes as a_frames next to a mix."""
    dev = table.device
    f = torch.as_tensor(win_file, device=dev).long()
    ok = (f >= 0) & (f < table.n_files)
    fc = f.clamp(0, table.n_files - 1)
    n = table.file_samp0[fc + 1] - table.file_samp0[fc]
    if warp is not None:
        if not isinstance(warp, Warp):
            raise HfttError('audio_frames: warp must be an ops.Warp')
        step, delay, cut = warp.step_q24.long(), warp.delay_q24, warp.cut()
        ok = ok & (step >= WARP_STEP_MIN) & (step <= WARP_STEP_MAX) & (delay >= 0) & (delay <= WARP_DELAY_MAX) & (cut >= 0.25) & (cut <= 1.0)
        step = step.clamp(WARP_STEP_MIN, WARP_STEP_MAX)
        n = torch.where(n > 0, (((n - 1) << 24) + delay) // step + 1, torch.zeros_like(n))
    return torch.where(ok, 1 + n // int(hop), torch.zeros_like(n)).contiguous()


class RoomBank:
    """The impulse responses of clip_room on one device, uploaded once: ir fp32 [n_ir, L] (1 <= L <= ROOM_MAX_TAPS; tap 0 is the direct path, so
    that no onset moves -- corpus.synth_audio.align_ir does that to a measured response) and taps int32 [n_ir] with 1 <= taps[r] <= L (None: L
    for every response): the entries of response r at or behind taps[r] are not read.  An equalisation filter is a response like any other."""

    def __init__(self, ir, device, taps=None):
        ir = torch.as_tensor(ir)
        if ir.dim() != 2 or ir.shape[0] < 1 or not 1 <= ir.shape[1] <= ROOM_MAX_TAPS:
            raise HfttError('RoomBank: ir must be [n_ir >= 1, 1 <= L <= %d], got shape %s' % (ROOM_MAX_TAPS, tuple(ir.shape)))
        if not ir.dtype.is_floating_point or not bool(torch.isfinite(ir).all()):
            raise HfttError('RoomBank: ir must be finite floating point, got %s' % ir.dtype)
        self.n_ir, self.L = int(ir.shape[0]), int(ir.shape[1])
        taps = torch.full((self.n_ir,), self.L, dtype=torch.int32) if taps is None else torch.as_tensor(taps)
        if taps.shape != (self.n_ir,) or taps.dtype.is_floating_point or int(taps.min()) < 1 or int(taps.max()) > self.L:
            raise HfttError('RoomBank: taps must be integers [n_ir] inside 1 .. L=%d' % self.L)
        self.device = torch.device(device)
        self.ir = ir.to(torch.float32).contiguous().to(self.device)
        self.taps = taps.to(torch.int32).contiguous().to(self.device)

    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in (self.ir, self.taps))


class WetTable:
    """what clip_room wrote, in the shape clip_logmel reads a WaveTable in: fp32 samples [B, span] as 2 B pseudo-files"""
    dtype = 'float32'

    def __init__(self, wave, file_samp0):
        self.device, self.wave, self.file_samp0 = wave.device, wave, file_samp0
        self.n_files, self.total_samples = file_samp0.numel() - 1, wave.numel()


def room_span(width, hop, n_fft=2048):
    """the samples of a scratch row that a window of `width` frames can show: (P + width - 1) * hop + n_fft / 2, P = ceil((n_fft / 2) / hop)"""
    hop, half = int(hop), int(n_fft) // 2
    return (-(-half // max(hop, 1)) + int(width) - 1) * hop + half


def clip_room(table, win_file, win_start, width, bank, ir_index, hop, n_fft=2048, gain=None, warp=None, mix=None):
    """The WET samples of B clip windows in ONE launch (hftt_clip_room): the signal clip_logmel would stage for window b -- file win_file[b] of
    `table` (a WaveTable) under `warp` / `mix` / gain exactly as there, in front of the noise -- convolved with response ir_index[b] (int32
    [B]) of `bank` (a RoomBank): wet[i] = sum_k h[k] dry[i - k] over the file's own extent, the tail behind its end cut.  ir_index < 0 leaves
    the window dry (bit for bit), ir_index >= bank.n_ir makes it a window without a file.  Returns (scratch fp32 [B, span], out_samp0 int64
    [2 B + 1], out_win_file int32 [B], out_win_start int32 [B]): row b holds the wet samples window b's frames read as pseudo-file 2 b, and a
    plain clip_logmel over them with the two window tables gives the log-mel of the wet file.  Nothing is read back to the host."""
    dev = table.device
    if not isinstance(bank, RoomBank):
        raise HfttError('clip_room: bank must be an ops.RoomBank')
    if warp is not None and not isinstance(warp, Warp):
        raise HfttError('clip_room: warp must be an ops.Warp')
    if mix is not None and not isinstance(mix, Mix):
        raise HfttError('clip_room: mix must be an ops.Mix')
    win_file = torch.as_tensor(win_file, device=dev).to(torch.int32).contiguous()
    win_start = torch.as_tensor(win_start, device=dev).to(torch.int32).contiguous()
    ir_index = torch.as_tensor(ir_index, device=dev).to(torch.int32).contiguous()
    _need_cuda(table.wave, table.file_samp0, win_file, win_start, ir_index, bank.ir, bank.taps)
    if bank.device != dev:
        raise HfttError('clip_room: the bank lives on %s, the corpus on %s' % (bank.device, dev))
    if win_file.dim() != 1 or win_start.shape != win_file.shape or ir_index.shape != win_file.shape:
        raise HfttError('clip_room: win_file, win_start and ir_index must be [B]')
    B, width = win_file.numel(), int(width)
    if gain is not None:
        gain = torch.as_tensor(gain, device=dev).to(torch.float32).contiguous()
        _need_cuda(gain)
        if gain.shape != win_file.shape:
            raise HfttError('clip_room: gain must be [B]')
    span = (room_span(width, hop, n_fft) + 3) // 4 * 4 if width >= 1 and int(hop) >= 1 else 4      # (a bad request is the library's to refuse)
    out = torch.empty((B, span), dtype=torch.float32, device=dev)
    samp0 = torch.empty(2 * B + 1, dtype=torch.int64, device=dev)
    ofile, ostart = torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
    d = ClipRoomDesc()
    d.wave, d.file_samp0, d.win_file, d.win_start = table.wave.data_ptr(), table.file_samp0.data_ptr(), win_file.data_ptr(), win_start.data_ptr()
    d.total_samples, d.wave_i16, d.n_files, d.B, d.width = table.total_samples, int(table.dtype == 'int16'), table.n_files, B, width
    d.n_fft, d.hop, d.n_ir, d.L = int(n_fft), int(hop), bank.n_ir, bank.L
    d.gain = gain.data_ptr() if gain is not None else None
    d.ir, d.ir_taps, d.ir_index, d.span = bank.ir.data_ptr(), bank.taps.data_ptr(), ir_index.data_ptr(), span
    d.out, d.out_samp0, d.out_win_file, d.out_win_start = out.data_ptr(), samp0.data_ptr(), ofile.data_ptr(), ostart.data_ptr()
    keep = []
    if mix is not None:
        mix._check('clip_room', B, dev)
        d.mix.mix_file, d.mix.mix_start, d.mix.mix_gain = mix.file.data_ptr(), mix.start.data_ptr(), mix.gain.data_ptr()
        if warp is not None or mix.warp is not None:
            wa, wb = warp or _identity_warp(B, dev), mix.warp or _identity_warp(B, dev)
            d.warp, ka = wa._args('clip_room', B, dev)
            d.mix_warp, kb = wb._args('clip_room', B, dev)
            keep += [wa, wb, ka, kb]
    elif warp is not None:
        d.warp, ka = warp._args('clip_room', B, dev)
        keep.append(ka)
    check(lib().hftt_clip_room(C.byref(d), _stream(dev)), 'clip_room')
    return out, samp0, ofile, ostart


def clip_logmel(table, logmel, win_file, win_start, width, fill, gain=None, noise_std=None, seed=0, warp=None, mix=None, room=None):
    """B clip windows of a waveform corpus -> spec [B, n_mels, width] fp32 in ONE launch (hftt_clip_logmel): window b shows log-mel frames
    win_start[b] .. + width of file win_file[b] of `table` (a WaveTable), each frame computed from that file's samples alone with the device
    tables of `logmel` (an ops.LogMel); frames outside the file are `fill`.  gain / noise_std: fp32 [B] device tensors or None (per-window
    gain factor; standard deviation of additive noise keyed on (seed, file, sample)).  warp: an ops.Warp or None -- with one, the files are
    played back at each window's rate and delay (hftt_clip_logmel_warp), win_start counts frames of the warped file and the noise is keyed on
    the warped sample.  mix: an ops.Mix or None -- with one (hftt_clip_logmel_mix / _mix_warp) each window's partner is added onto the primary's
    extent: gain * primary + mix.gain * partner, then the noise; a warp on either side takes both through the warped sample (the other side
    under the identity, which is exact).  room: (an ops.RoomBank, ir_index int32 [B]) or None -- with one, TWO launches and no host
    synchronisation between them: hftt_clip_room convolves each window's dry signal (warp, gain and mix applied: both instruments stand in the
    same room) with its response (ir_index < 0: the window stays dry) into a scratch corpus, and the plain hftt_clip_logmel reads that with
    gain=None and the caller's noise_std / seed.  The noise is then the microphone's, behind the room, and keyed on (seed, pseudo-file 2 b,
    position inside the scratch row), not on the source file.  Nothing is read back to the host."""
    dev = table.device
    if room is not None:
        if not (isinstance(room, tuple) and len(room) == 2 and isinstance(room[0], RoomBank)):
            raise HfttError('clip_logmel: room must be (an ops.RoomBank, ir_index)')
        _need_cuda(table.wave, table.file_samp0, logmel.window)
        wet, samp0, ofile, ostart = clip_room(table, win_file, win_start, width, room[0], room[1], logmel.hop, logmel.n_fft, gain=gain, warp=warp, mix=mix)
        return clip_logmel(WetTable(wet, samp0), logmel, ofile, ostart, width, fill, noise_std=noise_std, seed=seed)
    if warp is not None and not isinstance(warp, Warp):
        raise HfttError('clip_logmel: warp must be an ops.Warp')
    if mix is not None and not isinstance(mix, Mix):
        raise HfttError('clip_logmel: mix must be an ops.Mix')
    win_file = torch.as_tensor(win_file, device=dev).to(torch.int32).contiguous()
    win_start = torch.as_tensor(win_start, device=dev).to(torch.int32).contiguous()
    _need_cuda(table.wave, table.file_samp0, logmel.window, win_file, win_start)
    if logmel.device != dev:
        raise HfttError('clip_logmel: the LogMel tables live on %s, the corpus on %s' % (logmel.device, dev))
    if win_file.dim() != 1 or win_start.shape != win_file.shape:
        raise HfttError('clip_logmel: win_file and win_start must be [B]')
    B, width = win_file.numel(), int(width)
    aug = []
    for name, t in (('gain', gain), ('noise_std', noise_std)):
        if t is not None:
            t = torch.as_tensor(t, device=dev).to(torch.float32).contiguous()
            _need_cuda(t)
            if t.shape != win_file.shape:
                raise HfttError('clip_logmel: %s must be [B]' % name)
        aug.append(t)
    out = torch.empty((B, logmel.n_mels, max(width, 0)), dtype=torch.float32, device=dev)      # an empty request is the library's to refuse
    d = ClipLogmelDesc()
    d.wave, d.file_samp0, d.win_file, d.win_start = table.wave.data_ptr(), table.file_samp0.data_ptr(), win_file.data_ptr(), win_start.data_ptr()
    d.total_samples, d.wave_i16, d.n_files, d.B, d.width = table.total_samples, int(table.dtype == 'int16'), table.n_files, B, width
    d.n_fft, d.hop, d.n_mels, d.log_offset = logmel.n_fft, logmel.hop, logmel.n_mels, logmel.log_offset
    d.window, d.twiddle = logmel.window.data_ptr(), logmel.twiddle.data_ptr()
    d.fb_start, d.fb_len, d.fb_off, d.fb_w = logmel.fb_start.data_ptr(), logmel.fb_len.data_ptr(), logmel.fb_off.data_ptr(), logmel.fb_w.data_ptr()
    d.fill = float(fill)
    d.gain, d.noise_std = (t.data_ptr() if t is not None else None for t in aug)
    d.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    d.out = out.data_ptr()
    if mix is not None:
        mix._check('clip_logmel', B, dev)
        ma = ClipMixArgs()
        ma.mix_file, ma.mix_start, ma.mix_gain = mix.file.data_ptr(), mix.start.data_ptr(), mix.gain.data_ptr()
        if warp is None and mix.warp is None:
            m = ClipLogmelMixDesc()
            m.base, m.mix = d, ma
            check(lib().hftt_clip_logmel_mix(C.byref(m), _stream(dev)), 'clip_logmel_mix')
            return out
        wa, wb = warp or _identity_warp(B, dev), mix.warp or _identity_warp(B, dev)
        m = ClipLogmelMixWarpDesc()
        m.base, m.mix = d, ma
        m.warp, keep_a = wa._args('clip_logmel', B, dev)
        m.mix_warp, keep_b = wb._args('clip_logmel', B, dev)
        check(lib().hftt_clip_logmel_mix_warp(C.byref(m), _stream(dev)), 'clip_logmel_mix_warp')
        return out
    if warp is not None:
        w = ClipLogmelWarpDesc()
        w.base = d
        w.warp, keep = warp._args('clip_logmel', B, dev)
        check(lib().hftt_clip_logmel_warp(C.byref(w), _stream(dev)), 'clip_logmel_warp')
        return out
    check(lib().hftt_clip_logmel(C.byref(d), _stream(dev)), 'clip_logmel')
    return out


# ------------------------------------------------------------------------------------------------
# Labels from note lists (hftt_labels_render): the corpus keeps notes, a batch's labels are rendered when it is gathered
LABEL_NOTE = np.dtype([('onset_sec', np.float64), ('offset_sec', np.float64), ('velocity', np.int32), ('flags', np.int32)])
assert LABEL_NOTE.itemsize == C.sizeof(LabelNote)
LABELS_FORM = {'train': LABELS_TRAIN, 'store': LABELS_STORE}


def labels_grid(config):
    """(hop_ms, fps, tol) as the reference forms them (corpus/conv_note2label.py:11-13,20)"""
    cf = config['feature']
    hop_ms = 1000 * cf['hop_sample'] / cf['sr']
    return hop_ms, cf['sr'] / cf['hop_sample'], int(50.0 / hop_ms + 0.5)


def labels_table_host(notes_per_file, config):
    """The note table of hftt_labels_render as numpy arrays: notes_per_file = one note list per file (dicts with 'pitch', 'onset', 'offset' in
    seconds and 'velocity', as note2label takes them) -> dict(notes [n] LABEL_NOTE records grouped by (file, pitch) and inside a group in LIST
    order, row_ptr int32 [n_files * N + 1], file_nframe int32 [n_files], N, hop_ms, fps, tol; for the warped render: file_end_sec fp64
    [n_files] (the largest offset, 0 without notes), pitch_min / pitch_max int32 [n_files] (the lowest and highest sounding pitch index;
    N - 1 and 0 for a file without notes: no shift moves anything out of range) and sr).  Raises HfttError for a note outside the
    reference's working domain (there it indexes out of range or overflows int8)."""
    cm = config['midi']
    N, note_min = int(cm['num_note']), int(cm['note_min'])
    hop_ms, fps, tol = labels_grid(config)
    n_files = len(notes_per_file)
    if n_files < 1:
        raise HfttError('labels_table: no files')
    if not 1 <= N <= 128 or n_files * N + 1 >= 1 << 31:
        raise HfttError('labels_table: num_note=%d outside 1..128 (or too many files)' % N)
    if tol < 1:
        raise HfttError('labels_table: tol=%d: a hop of %g ms leaves the 50 ms triangle no frame' % (tol, hop_ms))
    counts = np.array([len(a) for a in notes_per_file], np.int64)
    flat = [n for a in notes_per_file for n in a]
    try:
        pitch = np.array([n['pitch'] for n in flat], np.float64)
        velocity = np.array([n['velocity'] for n in flat], np.float64)
        onset = np.array([n['onset'] for n in flat], np.float64) + 0.0          # (-0.0 -> +0.0)
        offset = np.array([n['offset'] for n in flat], np.float64) + 0.0
    except (KeyError, TypeError, ValueError) as e:
        raise HfttError('labels_table: a note needs numeric pitch / onset / offset / velocity (%r)' % (e,))
    file = np.repeat(np.arange(n_files), counts)

    def refuse(bad, what):
        if bad.any():
            i = int(np.argmax(bad))
            raise HfttError('labels_table: file %d, note %d: %s (%r)' % (file[i], i - int(counts[:file[i]].sum()), what, flat[i]))
    refuse(~((pitch == np.floor(pitch)) & (pitch >= note_min) & (pitch <= note_min + N - 1)), 'pitch outside note_min .. note_min + num_note - 1 = %d .. %d' % (note_min, note_min + N - 1))
    refuse(~((onset >= 0.0) & (onset <= offset)), 'needs 0 <= onset <= offset')
    refuse(~(offset * fps + 0.5 < float((1 << 31) - 1)), 'offset beyond 2^31 frames')
    refuse(~((velocity == np.floor(velocity)) & (velocity >= 0) & (velocity <= 127)), 'velocity outside 0..127')
    if len(flat) >= 1 << 31:
        raise HfttError('labels_table: %d notes exceed the int32 index' % len(flat))
    group = file * N + (pitch.astype(np.int64) - note_min)
    # bit 0: the offset equals, as a double, the onset of a note (this one included) of the same file and pitch (conv_note2label.py:76-83)
    key_on, key_off = np.empty(len(flat), np.complex128), np.empty(len(flat), np.complex128)
    key_on.real = key_off.real = group
    key_on.imag, key_off.imag = onset, offset
    order = np.argsort(group, kind='stable')                                    # list order inside a group; never by time
    notes = np.zeros(len(flat), LABEL_NOTE)
    notes['onset_sec'], notes['offset_sec'] = onset[order], offset[order]
    notes['velocity'] = velocity[order].astype(np.int32)
    notes['flags'] = np.isin(key_off, key_on)[order].astype(np.int32)
    row_ptr = np.zeros(n_files * N + 1, np.int32)
    row_ptr[1:] = np.cumsum(np.bincount(group, minlength=n_files * N))
    max_offset = np.zeros(n_files, np.float64)
    np.maximum.at(max_offset, file, offset)
    file_nframe = ((max_offset * fps + 0.5).astype(np.int64) + 1).astype(np.int32)      # conv_note2label.py:20-27
    pidx = pitch.astype(np.int64) - note_min
    pitch_min, pitch_max = np.full(n_files, N - 1, np.int64), np.zeros(n_files, np.int64)
    np.minimum.at(pitch_min, file, pidx)
    np.maximum.at(pitch_max, file, pidx)
    return {'notes': notes, 'row_ptr': row_ptr, 'file_nframe': file_nframe, 'N': N, 'hop_ms': hop_ms, 'fps': fps, 'tol': tol,
            'file_end_sec': max_offset, 'pitch_min': pitch_min.astype(np.int32), 'pitch_max': pitch_max.astype(np.int32), 'sr': config['feature']['sr']}


class LabelsTable:
    """the note table on one device (labels_table) + the three grid constants; file_nframe_host stays for callers that size outputs"""

    def __init__(self, host, device):
        self.device = torch.device(device)
        self.N, self.hop_ms, self.fps, self.tol = host['N'], host['hop_ms'], host['fps'], host['tol']
        self.file_nframe_host = host['file_nframe']
        self.n_files, self.n_notes = len(host['file_nframe']), len(host['notes'])
        self.notes = torch.from_numpy(np.ascontiguousarray(host['notes']).view(np.uint8).reshape(-1)).to(self.device)
        self.row_ptr = torch.from_numpy(host['row_ptr']).to(self.device)
        self.file_nframe = torch.from_numpy(host['file_nframe']).to(self.device)
        # the warped render's per-file columns (a host table from before they existed renders unwarped only)
        self.sr = host.get('sr')
        self.file_end_sec, self.pitch_min, self.pitch_max = (torch.from_numpy(host[k]).to(self.device) if k in host else None
                                                             for k in ('file_end_sec', 'pitch_min', 'pitch_max'))

    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in (self.notes, self.row_ptr, self.file_nframe, self.file_end_sec, self.pitch_min, self.pitch_max)
                   if t is not None)


def labels_table(notes_per_file, config, device):
    """note lists of a corpus -> the device-resident note table of labels_render (built once: labels_table_host + one upload)"""
    return LabelsTable(labels_table_host(notes_per_file, config), device)


def labels_render(table, win_file, win_start, length, form='train', duration_tolerance=False, warp=None, mix=None, a_frames=None):
    """B windows of `length` frames -> (onset, offset, mpe, velocity) [B, length, N] device tensors in ONE launch (hftt_labels_render).
    win_file / win_start: int32 [B] device tensors (file index; first frame counted from the file's frame 0, may be negative or behind the file:
    frames outside the file are zero) -- nothing is read back to the host.  form 'train': fp32, fp32, fp32, int64 (what engine.loss takes);
    'store': fp32, fp32, bool, int8 (the dtypes of corpus.conv_note2label.note2label_arrays).  warp: an ops.Warp or None -- with one
    (hftt_labels_render_warp) window b shows the labels of the file played back under it: pitches moved by shift[b], note times
    (t + t_delay) * t_scale, win_start in frames of the warped file.  mix: an ops.Mix or None -- with one (hftt_labels_render_mix) each cell
    walks the partner's notes (under mix.warp's map, if any) behind the primary's with the same carried state: the labels of the summed
    audio; a_frames: int64 [B] device tensor, the primaries' audio frame counts (ops.audio_frames), required with a mix -- the partner's
    notes show only where the primary has audio.  mix.gain is not read."""
    if form not in LABELS_FORM:
        raise HfttError('labels_render: form %r (train / store)' % (form,))
    dev = table.device

    def need_warp_columns():
        if table.file_end_sec is None or table.sr is None:
            raise HfttError('labels_render: the note table carries no file_end_sec / sr (built before the warped render): rebuild it with labels_table_host')
    if warp is not None:
        if not isinstance(warp, Warp):
            raise HfttError('labels_render: warp must be an ops.Warp')
        need_warp_columns()
    if mix is not None:
        if not isinstance(mix, Mix):
            raise HfttError('labels_render: mix must be an ops.Mix')
        if a_frames is None:
            raise HfttError('labels_render: a mix needs a_frames (the primaries\' audio frame counts: ops.audio_frames)')
        if mix.warp is not None:
            need_warp_columns()
    win_file = torch.as_tensor(win_file, device=dev).to(torch.int32).contiguous()
    win_start = torch.as_tensor(win_start, device=dev).to(torch.int32).contiguous()
    _need_cuda(table.notes, table.row_ptr, table.file_nframe, win_file, win_start)
    B, length = win_file.numel(), int(length)
    if win_file.dim() != 1 or win_start.shape != win_file.shape:
        raise HfttError('labels_render: win_file and win_start must be [B]')
    shape = (B, length, table.N)
    train = form == 'train'
    onset = torch.empty(shape, dtype=torch.float32, device=dev)
    offset = torch.empty(shape, dtype=torch.float32, device=dev)
    mpe = torch.empty(shape, dtype=torch.float32 if train else torch.uint8, device=dev)
    velocity = torch.empty(shape, dtype=torch.int64 if train else torch.int8, device=dev)
    d = LabelsDesc()
    d.notes, d.row_ptr, d.file_nframe = table.notes.data_ptr() if table.n_notes else None, table.row_ptr.data_ptr(), table.file_nframe.data_ptr()
    d.win_file, d.win_start = win_file.data_ptr(), win_start.data_ptr()
    d.n_files, d.n_notes = table.n_files, table.n_notes
    d.B, d.len, d.N, d.tol = B, length, table.N, table.tol
    d.duration_tolerance, d.form = int(bool(duration_tolerance)), LABELS_FORM[form]
    d.hop_ms, d.fps = table.hop_ms, table.fps
    d.onset, d.offset, d.mpe, d.velocity = onset.data_ptr(), offset.data_ptr(), mpe.data_ptr(), velocity.data_ptr()
    if mix is not None:
        mix._check('labels_render', B, dev)
        a_frames = torch.as_tensor(a_frames, device=dev).to(torch.int64).contiguous()
        _need_cuda(a_frames)
        if a_frames.shape != win_file.shape:
            raise HfttError('labels_render: a_frames must be [B]')
        m = LabelsMixDesc()
        m.base = d
        keep = []
        for w, names in ((warp, ('shift', 't_delay', 't_scale')), (mix.warp, ('mix_shift', 'mix_t_delay', 'mix_t_scale'))):
            if w is None:
                continue
            ts = w._label_map('labels_render', B, dev, table)
            keep.append(ts)
            for name, t in zip(names, ts):
                setattr(m, name, t.data_ptr())
            m.file_end_sec = table.file_end_sec.data_ptr()
        m.mix_file, m.mix_start, m.a_frames = mix.file.data_ptr(), mix.start.data_ptr(), a_frames.data_ptr()
        check(lib().hftt_labels_render_mix(C.byref(m), _stream(dev)), 'labels_render_mix')
    elif warp is not None:
        ts = warp._label_map('labels_render', B, dev, table)
        w = LabelsWarpDesc()
        w.base = d
        w.shift, w.t_delay, w.t_scale, w.file_end_sec = [t.data_ptr() for t in ts] + [table.file_end_sec.data_ptr()]
        check(lib().hftt_labels_render_warp(C.byref(w), _stream(dev)), 'labels_render_warp')
    else:
        check(lib().hftt_labels_render(C.byref(d), _stream(dev)), 'labels_render')
    return onset, offset, (mpe if train else mpe.view(torch.bool)), velocity


# ------------------------------------------------------------------------------------------------
# Clip synth (hftt_clip_synth): the corpus keeps NOTES only, a batch's waveforms are rendered from them when it is gathered
class VoiceBank:
    """The voices of clip_synth on one device, uploaded once: V voices of H decaying partials for each of N pitches --
        inc uint32 [V, N, H] (phase increment, turns per sample in Q32; integers inside 0 .. 2^32 - 1 of any integer dtype), amp fp32 [V, N, H]
        (0: the partial is off), dec fp32 [V, N, H] >= 0 (log2 units per sample), vel_gain fp32 [V, 128], rel fp32 [V] >= 0 (additional decay per
        sample behind the offset), attack int [V] >= 1 and release int [V] >= 0 (samples)
    with 1 <= H <= SYNTH_MAX_PARTIALS.  The kernel is a generic modal synthesizer: the instrument lives in whatever fills these tables
    (corpus.synth_audio.synth_voice_bank / pluck_voice)."""

    def __init__(self, inc, amp, dec, vel_gain, rel, attack, release, device):
        def tensor(t):                                  # (numpy's unsigned integers as int64: torch has no arithmetic on them)
            if torch.is_tensor(t):
                return t.cpu()
            a = np.asarray(t)
            return torch.from_numpy(np.ascontiguousarray(a.astype(np.int64) if a.dtype.kind in 'ui' else a))
        inc, amp, dec, vel_gain, rel, attack, release = (tensor(t) for t in (inc, amp, dec, vel_gain, rel, attack, release))
        if amp.dim() != 3 or min(amp.shape) < 1 or not 1 <= amp.shape[1] <= 128 or not 1 <= amp.shape[2] <= SYNTH_MAX_PARTIALS:
            raise HfttError('VoiceBank: amp must be [V >= 1, 1 <= N <= 128, 1 <= H <= %d], got shape %s' % (SYNTH_MAX_PARTIALS, tuple(amp.shape)))
        self.V, self.N, self.H = (int(n) for n in amp.shape)
        if self.V * self.N * self.H >= 1 << 31:
            raise HfttError('VoiceBank: V * N * H = %d entries exceed 2^31' % (self.V * self.N * self.H))
        for name, t, shape in (('inc', inc, amp.shape), ('dec', dec, amp.shape), ('vel_gain', vel_gain, (self.V, 128)), ('rel', rel, (self.V,)),
                               ('attack', attack, (self.V,)), ('release', release, (self.V,))):
            if tuple(t.shape) != tuple(shape):
                raise HfttError('VoiceBank: %s must have shape %s, got %s' % (name, tuple(shape), tuple(t.shape)))
        for name, t in (('amp', amp), ('dec', dec), ('vel_gain', vel_gain), ('rel', rel)):
            if not t.dtype.is_floating_point or not bool(torch.isfinite(t).all()):
                raise HfttError('VoiceBank: %s must be finite floating point, got %s' % (name, t.dtype))
        for name, t in (('dec', dec), ('rel', rel)):
            if bool((t < 0).any()):
                raise HfttError('VoiceBank: %s must not be negative' % name)
        for name, t, lo, hi in (('inc', inc, 0, (1 << 32) - 1), ('attack', attack, 1, (1 << 31) - 1), ('release', release, 0, (1 << 31) - 1)):
            if t.dtype.is_floating_point or t.dtype == torch.bool or int(t.min()) < lo or int(t.max()) > hi:
                raise HfttError('VoiceBank: %s must be integers inside %d .. %d' % (name, lo, hi))
        self.device = torch.device(device)
        # (torch has no uint32 arithmetic: the increments travel as the int32 with the same bits)
        inc = inc.to(torch.int64)
        self.inc = torch.where(inc >= 1 << 31, inc - (1 << 32), inc).to(torch.int32).contiguous().to(self.device)
        self.amp, self.dec, self.vel_gain, self.rel = (t.to(torch.float32).contiguous().to(self.device) for t in (amp, dec, vel_gain, rel))
        self.attack, self.release = (t.to(torch.int32).contiguous().to(self.device) for t in (attack, release))

    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in (self.inc, self.amp, self.dec, self.vel_gain, self.rel, self.attack, self.release))


def synth_span(width, hop, lead=0, n_fft=2048):
    """the samples of a scratch row that a window of `width` frames with `lead` further frames in front can show:
    (P + lead + width - 1) * hop + n_fft / 2, P = ceil((n_fft / 2) / hop)"""
    return room_span(int(width) + int(lead), hop, n_fft)


class SynthPart:
    """The SECOND PARTS of B windows of clip_synth as device tensors, in the manner of Mix: file int32 [B] (an index outside 0 .. n_files: the
    window has no partner), start int32 [B] (the partner frame that column 0 shows, counted in the partner's own -- mapped -- file), voice int32
    [B] (the partner's voice of the bank; outside 0 .. V - 1: no partner), gain fp32 [B], play: the partners' own ops.Warp or None (as
    written), tune: the partners' tuning, uint32-valued [B] in Q31 (2^31 = unison), or None."""

    def __init__(self, file, start, voice, gain, play=None, tune=None):
        if play is not None and not isinstance(play, Warp):
            raise HfttError('SynthPart: play must be an ops.Warp')
        self.file = torch.as_tensor(file).to(torch.int32).contiguous()
        dev = self.file.device
        self.start = torch.as_tensor(start, device=dev).to(torch.int32).contiguous()
        self.voice = torch.as_tensor(voice, device=dev).to(torch.int32).contiguous()
        self.gain = torch.as_tensor(gain, device=dev).to(torch.float32).contiguous()
        self.play = play
        self.tune = None if tune is None else _tune_bits(tune, dev)
        shapes = [t.shape for t in (self.start, self.voice, self.gain)] + ([] if self.tune is None else [self.tune.shape])
        if self.file.dim() != 1 or any(sh != self.file.shape for sh in shapes):
            raise HfttError('SynthPart: file, start, voice, gain and tune must be [B], got shapes %s' % ([tuple(self.file.shape)] + [tuple(sh) for sh in shapes],))
        if play is not None and (play.step_q24.shape != self.file.shape or play.step_q24.device != dev):
            raise HfttError('SynthPart: the play holds %d windows on %s, the partners %d on %s' % (play.step_q24.numel(), play.step_q24.device, self.file.numel(), dev))

    def _check(self, what, B, dev):
        if self.file.device != dev or self.file.numel() != B:
            raise HfttError('%s: the part holds %d windows on %s, the request %d on %s' % (what, self.file.numel(), self.file.device, B, dev))


def _tune_bits(tune, dev):
    """a uint32-valued tuning table (any integer dtype, values 0 .. 2^32 - 1, or the int32 with the same bits) as int32 bits, like VoiceBank.inc"""
    t = torch.as_tensor(tune, device=dev)
    if t.dtype.is_floating_point or t.dtype == torch.bool:
        raise HfttError('clip_synth: tune must be integers (Q31: 2^31 = unison), got %s' % t.dtype)
    if t.dtype != torch.int32:
        t = t.to(torch.int64)
        t = torch.where(t >= 1 << 31, t - (1 << 32), t).to(torch.int32)
    return t.contiguous()


def tune_q31(cents):
    """cents (a number or an array) -> the Q31 tuning factor round(2^(cents / 1200) * 2^31) as int64 numpy: what clip_synth takes as `tune`"""
    return np.round(np.exp2(np.asarray(cents, np.float64) / 1200.0) * 2.0 ** 31).astype(np.int64)


def synth_nsamp(table, file_nsamp, win_file, play=None):
    """int64 [B] on the device: the length n' of each window's synthetic file under `play` (an ops.Warp or None) --
    file_nsamp[f] + ceil(t'(file_end_sec[f]) * sr) - ceil(file_end_sec[f] * sr) with t' = (t + t_delay) * t_scale, so the release tail behind
    the last offset keeps its length -- and 0 for a file outside the table.  What clip_synth takes as nsamp."""
    if not isinstance(table, LabelsTable):
        raise HfttError('synth_nsamp: table must be an ops.LabelsTable')
    if play is not None and not isinstance(play, Warp):
        raise HfttError('synth_nsamp: play must be an ops.Warp')
    dev = table.device
    file_nsamp = torch.as_tensor(file_nsamp, device=dev).to(torch.int64)
    if file_nsamp.shape != (table.n_files,):
        raise HfttError('synth_nsamp: file_nsamp must be [n_files=%d], got shape %s' % (table.n_files, tuple(file_nsamp.shape)))
    f = torch.as_tensor(win_file, device=dev).long()
    if f.dim() != 1:
        raise HfttError('synth_nsamp: win_file must be [B], got shape %s' % (tuple(f.shape),))
    ok = (f >= 0) & (f < table.n_files)
    fc = f.clamp(0, table.n_files - 1)
    n = file_nsamp[fc]
    if play is not None:
        if table.file_end_sec is None or table.sr is None:
            raise HfttError('synth_nsamp: the note table carries no file_end_sec / sr: rebuild it with labels_table_host')
        play._holds('synth_nsamp', f.numel(), dev)
        end, sr = table.file_end_sec[fc], float(table.sr)
        mapped = (end + play.t_delay(sr)) * play.t_scale()
        n = n + torch.ceil(mapped * sr).long() - torch.ceil(end * sr).long()
    return torch.where(ok, n, torch.zeros_like(n)).contiguous()


def synth_frames(nsamp, hop):
    """int64 [B]: the audio frame count 1 + n' / hop of each window's synthetic file (nsamp: synth_nsamp's result), 0 for an invalid window
    (n' < 0).  What labels_render takes as a_frames next to a second part."""
    n = torch.as_tensor(nsamp).to(torch.int64)
    return torch.where(n >= 0, 1 + n // int(hop), torch.zeros_like(n)).contiguous()


def clip_synth(table, file_nsamp, bank, voice_index, win_file, win_start, width, hop, sr, lead=0, n_fft=2048, play=None, tune=None, part=None, nsamp=None):
    """The samples of B clip windows RENDERED in ONE launch (hftt_clip_synth): window b shows frames win_start[b] .. + width of the synthetic
    file that the notes of file win_file[b] of `table` (a LabelsTable) make under voice voice_index[b] (int32 [B]) of `bank` (a VoiceBank);
    file_nsamp int64 [n_files] (a device tensor) is each file's length in samples.  lead: further frames rendered in front of each window, so
    that a room can follow (clip_room over the result as its corpus needs lead >= ceil(taps / hop)).  Returns what clip_room returns: (scratch
    fp32 [B, span], out_samp0 int64 [2 B + 1], out_win_file int32 [B], out_win_start int32 [B]); a plain clip_logmel over WetTable(scratch,
    out_samp0) with the two window tables gives the log-mel of the synthetic file.  A voice index outside 0 .. V - 1 makes a window without a
    file.  Nothing is read back to the host; no CPU fallback.
    With play, tune, part or nsamp the launch is hftt_clip_synth_parts: play, an ops.Warp, is how the windows are PLAYED -- shift [B] semitones
    of transposition (an index into the bank), step_q24 the TEMPO * 2^24 and delay_q24 a delay in samples * 2^24, from which Warp derives
    t_scale and t_delay (cut and proto are not used); tune, uint32-valued [B], the tuning in Q31 (2^31 = unison; ops.tune_q31); part, an
    ops.SynthPart, a second part per window under its own voice and play, summed onto the first; nsamp int64 [B], the windows' file lengths
    under their map (None: ops.synth_nsamp of file_nsamp and play).  With all four None the launch is hftt_clip_synth as it always was."""
    launch, outs = _clip_synth_prepare(table, file_nsamp, bank, voice_index, win_file, win_start, width, hop, sr, lead, n_fft, play, tune, part, nsamp)
    launch()
    return outs


def _clip_synth_prepare(table, file_nsamp, bank, voice_index, win_file, win_start, width, hop, sr, lead, n_fft, play, tune, part, nsamp):
    """clip_synth's checks, derived tables and descriptor -> (launch, outputs): launch() enqueues the one kernel and nothing else (it keeps the
    tensors the descriptor points to alive), so that a benchmark can time the launch without the derivations in front of it"""
    if not isinstance(table, LabelsTable):
        raise HfttError('clip_synth: table must be an ops.LabelsTable')
    if not isinstance(bank, VoiceBank):
        raise HfttError('clip_synth: bank must be an ops.VoiceBank')
    dev = table.device
    if bank.device != dev:
        raise HfttError('clip_synth: the bank lives on %s, the note table on %s' % (bank.device, dev))
    if bank.N != table.N:
        raise HfttError('clip_synth: the bank holds N=%d pitches, the note table N=%d' % (bank.N, table.N))
    file_nsamp = torch.as_tensor(file_nsamp, device=dev).to(torch.int64).contiguous()
    if file_nsamp.shape != (table.n_files,):
        raise HfttError('clip_synth: file_nsamp must be [n_files=%d], got shape %s' % (table.n_files, tuple(file_nsamp.shape)))
    win_file = torch.as_tensor(win_file, device=dev).to(torch.int32).contiguous()
    win_start = torch.as_tensor(win_start, device=dev).to(torch.int32).contiguous()
    voice_index = torch.as_tensor(voice_index, device=dev).to(torch.int32).contiguous()
    if win_file.dim() != 1 or win_start.shape != win_file.shape or voice_index.shape != win_file.shape:
        raise HfttError('clip_synth: win_file, win_start and voice_index must be [B]')
    _need_cuda(table.notes, table.row_ptr, file_nsamp, win_file, win_start, voice_index, bank.inc)
    B, width, lead = win_file.numel(), int(width), int(lead)
    span = (synth_span(width, hop, lead, n_fft) + 3) // 4 * 4 if width >= 1 and int(hop) >= 1 and lead >= 0 else 4      # (a bad request is the library's to refuse)
    out = torch.empty((B, span), dtype=torch.float32, device=dev)
    samp0 = torch.empty(2 * B + 1, dtype=torch.int64, device=dev)
    ofile, ostart = torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
    d = ClipSynthDesc()
    d.notes, d.row_ptr, d.file_nsamp = table.notes.data_ptr() if table.n_notes else None, table.row_ptr.data_ptr(), file_nsamp.data_ptr()
    d.win_file, d.win_start, d.voice_index = win_file.data_ptr(), win_start.data_ptr(), voice_index.data_ptr()
    d.n_files, d.n_notes, d.B, d.width, d.N = table.n_files, table.n_notes, B, width, table.N
    d.n_fft, d.hop, d.lead, d.sr, d.V, d.H = int(n_fft), int(hop), lead, float(sr), bank.V, bank.H
    d.inc, d.amp, d.dec, d.vel_gain, d.rel = (t.data_ptr() for t in (bank.inc, bank.amp, bank.dec, bank.vel_gain, bank.rel))
    d.attack, d.release, d.span = bank.attack.data_ptr(), bank.release.data_ptr(), span
    d.out, d.out_samp0, d.out_win_file, d.out_win_start = out.data_ptr(), samp0.data_ptr(), ofile.data_ptr(), ostart.data_ptr()
    if play is None and tune is None and part is None and nsamp is None:
        def launch(keep=(file_nsamp, win_file, win_start, voice_index)):
            check(lib().hftt_clip_synth(C.byref(d), _stream(dev)), 'clip_synth')
        return launch, (out, samp0, ofile, ostart)
    if play is not None and not isinstance(play, Warp):
        raise HfttError('clip_synth: play must be an ops.Warp')
    if part is not None and not isinstance(part, SynthPart):
        raise HfttError('clip_synth: part must be an ops.SynthPart')
    m = ClipSynthPartsDesc()
    m.base = d
    nsamp = synth_nsamp(table, file_nsamp, win_file, play) if nsamp is None else torch.as_tensor(nsamp, device=dev).to(torch.int64).contiguous()
    if nsamp.shape != win_file.shape:
        raise HfttError('clip_synth: nsamp must be [B=%d], got shape %s' % (B, tuple(nsamp.shape)))
    keep = [nsamp]
    m.nsamp = nsamp.data_ptr()

    def fill(args, p, t):
        if p is not None:
            ts = p._label_map('clip_synth', B, dev, table)
            keep.append(ts)
            args.shift, args.t_delay, args.t_scale = (x.data_ptr() for x in ts)
        if t is not None:
            t = _tune_bits(t, dev)
            if t.shape != win_file.shape:
                raise HfttError('clip_synth: tune must be [B=%d], got shape %s' % (B, tuple(t.shape)))
            _need_cuda(t)
            keep.append(t)
            args.tune_q31 = t.data_ptr()
    fill(m.play, play, tune)
    if part is not None:
        part._check('clip_synth', B, dev)
        pn = synth_nsamp(table, file_nsamp, part.file, part.play)
        _need_cuda(part.file, part.start, part.voice, part.gain, pn)
        keep.append(pn)
        m.part_file, m.part_start, m.part_voice, m.part_gain = part.file.data_ptr(), part.start.data_ptr(), part.voice.data_ptr(), part.gain.data_ptr()
        m.part_nsamp = pn.data_ptr()
        fill(m.part_play, part.play, part.tune)
    _need_cuda(nsamp)
    keep += [file_nsamp, win_file, win_start, voice_index]

    def launch(keep=keep):
        check(lib().hftt_clip_synth_parts(C.byref(m), _stream(dev)), 'clip_synth_parts')
    return launch, (out, samp0, ofile, ostart)
