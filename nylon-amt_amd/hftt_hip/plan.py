"""Launch plans of one workspace (one batch size) of the engine.

A `PlanBuilder` lives for one `HfttEngine.workspace(B)` call.  It carries the workspace dict, the plan being written, the dropout-site
counter and the mode OF THIS WORKSPACE as plain fields; the engine's own mode (`eng.strip`, `eng.hh`, ...) is only read.  Its methods come
in three layers: descriptor emitters (`nt`, `sl`, `mlp`, `tn`, `attn`, `lnb`: one C descriptor + one plan entry each), the model's blocks
(self attention and FFN, forward and backward, each written once) and the three plans (`forward` twice, `backward`).

The `*_meta` functions name the kernel a launch resolves to (as rocprofv3 prints it: tests/test_kernel_names_gpu.py holds every name
against a kernel trace) and count its algorithmic bytes.  They are pure and mirror the C dispatch each of them points to.
"""
import ctypes as C
import math
import os

import torch

from . import _capi
from ._capi import (AttnDesc, FfnDesc, GemmNtDesc, GemmTnDesc, LnBwdDesc, StripDesc,
                    SL_C_BF16, SL_C_F16PAIR, SL_H_BF16, SL_PRE_BF16, SL_RELU, SL_X3_GRAD_HI, SL_RES_BF16, SL_X_BF16, SL_X3_F16, SL_X3_BF16, SL_X_DROP,
                    ATTN_Q_F16PAIR, ATTN_KV_F16PAIR)
from .layout import _align, qkv_planes


def attn_fwd8_takes(npass, hb, dh, Lq, Lk, probs):
    """Does hftt_attn_fwd launch attn_fwd8_kernel for this shape (csrc/attn_fwd8.hip: hftt_attn_fwd8_try)?  hb: q, k, v and out all bf16;
    probs: the attention map is an output.  HFTT_ATTN_FWD8 is read once per process on the C side."""
    return (hb and dh == 64 and npass == 1 and 128 < Lk <= 256 and 128 < Lq <= 256 and not probs
            and os.environ.get('HFTT_ATTN_FWD8', '1')[:1] != '0')


def _tf(v):
    return 'true' if v else 'false'


def _env_on(name):
    return os.environ.get(name, '1')[:1] != '0'


def nt_meta(npass, a_hi, M, N, K, a_bf, c_bf, gate_bf, res_bf, add_table, gate, drop_site, residual, ln):
    """hftt_gemm_nt (mirrors dispatch_nt_bf16 in csrc/gemm_nt.hip); npass: the descriptor's (4: x3 with a gradient operand), ln: fused LayerNorm"""
    n_pad = _align(N, 64)
    bn = N if ln else (256 if n_pad % 256 == 0 else (128 if n_pad % 128 == 0 else 64))
    esz = 2 if npass == 1 else 4                # (x3: two 16-bit planes = 4 bytes per weight)
    nbytes = (2 if a_bf else 4) * M * K + (2 if c_bf else 4) * M * N + esz * N * K + ((2 if res_bf else 4) * M * N if residual else 0) + (4 * M * N if ln else 0) \
        + ((2 if gate_bf else 4) * M * N if gate else 0)
    rich = bool(add_table or gate or drop_site or residual or ln)
    if npass == 1 and N % 256 == 0 and K <= 768 and M >= 256:
        pf = 2 if (K // 32) % 2 == 0 else 1
        if K <= 256:
            elementwise = not (add_table or residual or ln) and c_bf and (not gate or gate_bf)
            if not rich:
                kname = 'gemm_nt_as1_kernel<64, 0, false, %d>' % pf
            elif elementwise:
                kname = 'gemm_nt_as1_kernel<64, 0, true, %d>' % pf
            elif N == 256:
                kname = 'gemm_nt_as1_kernel<64, 1, false, %d>' % pf
            else:
                kname = 'gemm_nt_as1_kernel<32, 2, false, 1>'
        elif N == 256 and K > 512:
            kname = 'gemm_nt_as1_kernel<64, 1, false, %d>' % pf
        elif N == 256 and pf == 2:
            kname = 'gemm_nt_as1_kernel<%d, 1, false, 2>' % (32 if ln else 64)
        else:
            kname = 'gemm_nt_as1_kernel<32, 2, false, 1>'
    elif (npass in (2, 4) and not a_hi and not ln and K <= 256 and (N == 256 or (K == 256 and N <= 256)) and (N % 4 == 0 or not rich)
          and _env_on('HFTT_NT_STREAM')):
        # (nt_as3_takes: the A-stationary split form; the C side reads HFTT_NT_STREAM at every call, this name is fixed when the plan is built)
        kname = 'gemm_nt_as3_kernel<%d, %d, %s>' % (npass, 4 if K <= 128 else 8, _tf((K // 32) % 2 == 0))
    else:
        kname = 'gemm_nt_kernel<%d, %d, %s>' % (bn, 5 if a_hi else npass, _tf(ln))
    return {'kernel': kname, 'flops': 2.0 * M * N * K, 'bytes': float(nbytes), 'shape': (M, N, K)}


def sl_meta(x3, small, hh, g8, backward, M, N, K, ln, pre_saved, residual, gate, c_planes, x_drop):
    """hftt_strip_linear (the C side picks the pipelined bf16 form by the rule mirrored here: strip_gemm2.hip hftt_strip_linear2_try; the x3
    forms: x3_strip.hip launch_xl; the small-width families: x3s_strip.h, bs_strip.hip)"""
    bf = not x3                                  # bf16 strip plans: x, C and the residual are all bf16; x3: all fp32
    nbytes = (2 if bf else 4) * M * K + (2 if bf else 4) * M * N + ((2 if (bf or hh) else 4) * M * N if pre_saved else 0) + (4 if x3 else 2) * N * K \
        + ((2 if bf else 4) * M * N if residual else 0) + (2 * M * N if gate else 0)
    passes, kch = N // 256, K // 256
    if small:
        kname = ('x3s_linear_kernel<%d, %d, %d, %s, %s>' % (4 if backward else 2, K // 32, N // 32, _tf(ln), _tf(residual))) if x3 \
            else 'bs_linear_kernel<%d, %d, %s, %s>' % (K // 32, N // 32, _tf(ln), _tf(residual))
    elif x3:
        xe = (5 if g8 else 4) if backward else 2
        if not ln and kch == 1:
            kname = 'x3_linear_n_kernel<%d, %d, %s, %s, %s>' % (xe, N // 32, _tf(residual), _tf(c_planes), _tf(x_drop))
        else:
            # (last argument: resident strip chunks -- the one-pass forms without LayerNorm keep half a set and run two workgroups per CU)
            kname = 'x3_linear_kernel<%d, %s, %d, %d, %s, %d>' % (xe, _tf(ln), passes, kch, _tf(residual), 8 if (not ln and passes == 1) else 16)
    elif (_env_on('HFTT_STRIP_V2') and K % 256 == 0 and M % 32 == 0 and not gate
          and ((ln and kch <= 3) or (not ln and (kch, passes) in ((1, 1), (1, 2), (1, 3), (2, 1), (3, 1))))):
        kname = 'strip_linear2_kernel<%s, %d, %d, %s, %s>' % (_tf(ln), 1 if ln else passes, kch, _tf(residual), _tf(_env_on('HFTT_LINEAR2_PATCH')))
    else:
        kname = 'strip_linear_kernel<true, true, %s>' % _tf(ln)
    return {'kernel': kname, 'flops': 2.0 * M * N * K, 'bytes': float(nbytes), 'shape': (M, N, K)}


def mlp_meta(x3, small, hh, g8, mode, M, d, p, residual, pre_saved, h_out, gate):
    """hftt_ffn_res_ln_fwd (mode 0) / hftt_ffn_bwd_dx (mode 1).  The bf16 fused block takes its whole-line store path, the last template
    argument, for the training forward only: strip_gemm2.hip hftt_strip_mlp2_try"""
    esz = 4.0 if x3 else 2.0
    hsz = 2.0 if (hh or not x3) else 4.0
    nbytes = esz * M * d * (2 + (1 if residual else 0)) + (hsz * M * d if pre_saved else 0) + (hsz * M * p if h_out else 0) + (hsz * M * p if gate else 0) + 2 * esz * d * p
    if x3:
        kname = ('x3s_mlp_kernel<%d, %s>' % (mode, _tf(hh))) if small else 'x3_mlp_kernel<%d, 16, %s, %s>' % (mode, _tf(hh), _tf(mode == 1 and g8))
    elif small:
        kname = 'bs_mlp_kernel<%d>' % mode
    elif _env_on('HFTT_STRIP_V2') and p == 512 and M % 32 == 0 and not (mode == 0 and residual):
        stp = os.environ.get('HFTT_MLP2_PATCH')
        stp = (stp[:1] != '0') if stp else (mode == 0 and bool(h_out or pre_saved))
        kname = 'strip_mlp2_kernel<%d, 16, %s>' % (mode, _tf(stp))
    else:
        kname = 'strip_mlp_kernel<%d>' % mode
    return {'kernel': kname, 'flops': 4.0 * M * d * p, 'bytes': nbytes, 'shape': (M, d, p), 'saves': bool(h_out or pre_saved)}


def tn_meta(npass, M, N, K, dy_bf, x_bf, dy_hi, dy_drop):
    """hftt_gemm_tn (csrc/gemm_tn.hip tn_plan); npass: the descriptor's"""
    tile = '2, 4' if (N >= 256 and K >= 256) else ('1, 2' if (N >= 128 and K >= 128) else '1, 1')
    if tile == '2, 4' and N <= 256 and K <= 256:
        tile = '1, 4'                           # (the 128 x 256 tile for single-tile shapes)
    return {'kernel': 'gemm_tn_kernel<%s, %d, %s, %s>' % (tile, 6 if dy_drop else (5 if dy_hi else npass), _tf(dy_bf), _tf(x_bf)), 'flops': 2.0 * M * N * K,
            'bytes': (2.0 if dy_bf else 4.0) * M * N + (2.0 if x_bf else 4.0) * M * K + 4.0 * N * K, 'shape': (M, N, K)}


def attn_meta(npass, bwd, n_seq, H, Lq, Lk, d, flags, planes, probs, dm):
    """hftt_attn_fwd / hftt_attn_bwd (csrc/attn.hip, x3_attn.hip, x3_attn_pl.hip, attn_fwd8.hip).  probs: the attention map is written;
    dm: dropout form of the x3 kernels (a template parameter, chosen by the C side from drop_p and the shape): 0 none, 1 per key quad, 2 per element"""
    dh = d // H
    kt = (Lk + 31) // 32
    kt = kt if kt <= 4 else 8
    eq, ekv, eo = (2.0 if flags & 1 else 4.0), (2.0 if flags & 2 else 4.0), (2.0 if flags & 4 else 4.0)
    qkv_bytes = n_seq * (eq * Lq + 2 * ekv * Lk) * d
    hb = (flags & 7) == 7
    if bwd:
        kname = ('x3_attn_bwd_kernel<%d, %d, %s, %d>' % (kt, dh, _tf(planes), dm)) if npass == 2 else 'attn_bwd_kernel<%d, %d, %d, %s>' % (kt, dh, npass, _tf(hb))
        return {'kernel': kname, 'flops': 10.0 * n_seq * H * Lq * Lk * dh,
                'bytes': qkv_bytes + n_seq * ((2.0 if flags & 8 else 4.0) * Lq + 2 * (2.0 if flags & 16 else 4.0) * Lk) * d + 2 * eo * n_seq * Lq * d
                + 8.0 * n_seq * H * Lq, 'shape': (n_seq, H, Lq, Lk, dh)}
    if attn_fwd8_takes(npass, hb, dh, Lq, Lk, probs):
        kname = 'attn_fwd8_kernel'
    elif npass != 2:
        kname = 'attn_fwd_kernel<%d, %d, %d, %s>' % (kt, dh, npass, _tf(hb))
    elif planes:
        kname = 'x3p_attn_fwd_kernel<%d, %d, %s, %d>' % (kt, 8 if (kt == 8 and Lq > 128) else 4, _tf(probs), dm)
    else:
        kname = 'x3_attn_fwd_kernel<%d, %d, %d, %s>' % (kt, dh, 8 if kt == 8 else 4, _tf(probs))
    # q, k, v, out + the row statistics (max, 1/sum) + the attention map where it is a model output (fp32, mandatory)
    return {'kernel': kname, 'flops': 4.0 * n_seq * H * Lq * Lk * dh,
            'bytes': qkv_bytes + eo * n_seq * Lq * d + 8.0 * n_seq * H * Lq + (4.0 * n_seq * H * Lq * Lk if probs else 0.0), 'shape': (n_seq, H, Lq, Lk, dh)}


class PlanBuilder:
    def __init__(self, eng, B, ws=None):
        """ws: a finished workspace of this engine and batch size, to write one more plan into it (build_decoder_backward); the builder is
        not kept by the workspace -- a reference from there would tie the engine into a cycle and its device memory to the garbage collector"""
        self.eng, self.lib = eng, eng.lib
        self.ws = ws if ws is not None else {'bufs': {}, 'drop': [], 'keep': [], 'tn': [], 'ln': [], 'B': B}
        self.plan = None
        self.site = 0
        # The x3 strip kernels take whole 32-token strips (hftt_x3_strip_linear / hftt_x3_strip_mlp: M % 32 == 0).  A batch whose token counts
        # are not multiples of 32 (B * T % 4 != 0 with 88 notes: odd batch x odd frame count) gets the block-GEMM plans of the same precision
        # for THIS workspace only -- same arithmetic (npass 2 / 4 in gemm_nt / gemm_tn), fp32 saved tensors.
        Se, Sn = B * eng.T * eng.F, B * eng.T * eng.N
        self.strip = eng.strip and not (eng.x3 and (Se % 32 or Sn % 32))
        self.bfs, self.hh = self.strip and eng.bfs, self.strip and eng.hh
        self.backward = False                       # the backward plan is being written (x3: products with a gradient operand)
        self.inference = False                      # the plan that saves nothing is being written (it runs without dropout)
        self.ws['strip'] = self.strip
        # masked-in-consumers: the LayerNorm backward writes no masked copy; its consumers apply the dropout mask while they load dr
        # (x3 strip plans at d = 256, dropout on)
        self.mic = bool(self.strip and eng.x3 and not eng.strip_small and not eng.g8 and eng.ln_mask_in_consumers_opt and eng.dropout > 0.0)
        # (first address, end address, stored as bf16) of every workspace tensor
        self._spans = [(t.data_ptr(), t.data_ptr() + t.numel() * t.element_size(), t.dtype == torch.bfloat16) for t in self.ws['bufs'].values()]
        self._bf16_content = set()                  # fp32-declared tensors that hold bf16 at this point of the plan (HFTT_BF16_GRAD)

    # ------------------------------------------------------------------ tensors
    def buf(self, name, *shape, dtype=torch.float32, half=False, hidden=False):
        """half=True: a GEMM-only tensor -> bf16 when the engine stores such tensors as bf16; hidden=True: the FFN hidden / its gradient
        (bf16 in the x3 strip plans too)."""
        if (half and self.eng.sb) or (hidden and self.hh):
            dtype = torch.bfloat16
        t = self.ws['bufs'].get(name)
        if t is not None:
            if tuple(t.shape) != tuple(shape) or t.dtype != dtype:
                raise _capi.HfttError('workspace buffer %s re-declared with a different shape / dtype' % name)
            return t
        t = torch.empty(*shape, dtype=dtype, device=self.eng.device)
        self.ws['bufs'][name] = t
        self._spans.append((t.data_ptr(), t.data_ptr() + t.numel() * t.element_size(), dtype == torch.bfloat16))
        return t

    def abuf(self, name, *shape):
        """activation-stream tensor: bf16 when the strip kernels run (bf16 residual stream), fp32 otherwise"""
        return self.buf(name, *shape, dtype=torch.bfloat16 if self.bfs else torch.float32)

    def pbuf(self, name, *shape):
        """saved pre-LayerNorm sum (read by the LayerNorm backward only): bf16 on the bf16 stream and in the x3 strip plans"""
        return self.buf(name, *shape, dtype=torch.bfloat16 if (self.bfs or self.hh) else torch.float32)

    def is_bf16(self, addr):
        """is the workspace tensor at this address stored as bf16?  (parameters, gradients and null pointers: no)"""
        for lo, hi, bf in self._spans:
            if lo <= addr < hi:
                return bf or lo in self._bf16_content
        return False

    def new_site(self):
        self.site += 1
        return self.site

    def planes(self, H, Lq, Lk):
        return self.strip and qkv_planes(self.eng.modes, self.eng.opts, self.eng.d, H, Lq, Lk)

    # ------------------------------------------------------------------ descriptor emitters
    def _epilogue(self, dsc, gate=0, ldg=0, gate_scale=1.0, ln=None, drop=False):
        """the tail the emitters share: the hidden-layer gate (a tuple as gate_scale: the run-time 1/(1-p), patched per step), the fused
        LayerNorm (gamma, beta, pre-LN sum out, mean out, rstd out), registration for the per-step dropout patch.  Returns: is the pre-LN sum saved"""
        if isinstance(gate_scale, tuple):
            self.ws.setdefault('gate_descs', []).append(dsc)
            gate_scale = 1.0
        dsc.gate, dsc.ldg, dsc.gate_scale = gate, ldg, gate_scale
        if ln is not None:
            dsc.ln_gamma, dsc.ln_beta, dsc.pre_ln_out, dsc.ln_mean, dsc.ln_rstd = ln
        if drop:
            self.ws['drop'].append(dsc)
        self.ws['keep'].append(dsc)
        return ln is not None and bool(ln[2])

    def nt(self, M, N, K, A, lda, W, bias, Cp, ldc, act=0, out_scale=1.0, add_table=0, add_mod=0,
           gate=0, ldg=0, gate_scale=1.0, drop_site=0, residual=0, ldr=0, res_mod=0, ln=None):
        """hftt_gemm_nt plan entry: C = epi(A . W^T + bias), W a prepared matrix plane (eng.Wp)"""
        e = self.eng
        a_bf, c_bf, gate_bf, res_bf = self.is_bf16(A), self.is_bf16(Cp), self.is_bf16(gate), self.is_bf16(residual)
        dsc = GemmNtDesc()
        npass = e.npass if e.npass != 2 else (4 if self.backward else 2)       # x3: fp16 halves forward, bf16 halves with gradients
        a_hi = npass == 4 and e.g8                  # (every block GEMM of the backward has a gradient as its A operand)
        dsc.io_flags = (1 if a_bf else 0) | (2 if c_bf else 0) | (4 if gate_bf else 0) | (8 if res_bf else 0) | (16 if a_hi else 0)
        dsc.M, dsc.N, dsc.K, dsc.npass = M, N, K, npass
        dsc.A, dsc.lda = A, lda
        dsc.W = W
        dsc.W_lo = e.Wp_lo(W)
        dsc.bias = bias
        dsc.C, dsc.ldc = Cp, ldc
        dsc.act, dsc.out_scale = act, out_scale
        dsc.add_table, dsc.add_mod = add_table, add_mod
        dsc.drop_p, dsc.drop_site, dsc.drop_seed = 0.0, drop_site, 0
        dsc.residual, dsc.ldr, dsc.res_mod = residual, ldr, (res_mod or M)
        self._epilogue(dsc, gate, ldg, gate_scale, ln, drop=drop_site)
        meta = nt_meta(npass, a_hi, M, N, K, a_bf, c_bf, gate_bf, res_bf, add_table, gate, drop_site, residual, ln is not None)
        self.plan.append((self.lib.hftt_gemm_nt, (C.byref(dsc),), 'gemm_nt', meta))
        return dsc

    def sl(self, M, N, K, x, ldx, wkey, bias, Cp, ldc, relu=False, out_scale=1.0, gate=0, ldg=0, gate_scale=1.0, drop_site=0,
           residual=0, ldr=0, res_mod=0, ln=None, c_planes=False, x_drop_site=0):
        """hftt_strip_linear plan entry (N % 256 == 0): C = epi(x . Wl^T + bias), Wl = strip pack `wkey`.  bf16 strip plans: x, C and the
        residual are bf16; x3: fp32 tensors, fp16 halves on forward products, bf16 halves where a gradient is an operand"""
        e = self.eng
        dsc = StripDesc()
        dsc.M, dsc.N, dsc.K = M, N, K
        if e.x3:
            dsc.flags = (SL_X3_BF16 if self.backward else SL_X3_F16) | (SL_RELU if relu else 0) | (SL_PRE_BF16 if (self.hh and ln is not None) else 0) \
                | (SL_X3_GRAD_HI if (self.backward and e.g8) else 0) | (SL_C_F16PAIR if c_planes else 0) | (SL_X_DROP if x_drop_site else 0)
            if x_drop_site:                          # HFTT_SL_X_DROP: x (the LayerNorm backward's dr) is masked while it is loaded
                assert self.backward and not drop_site and N == 256 and K == 256
                drop_site = x_drop_site
        else:
            dsc.flags = SL_X_BF16 | SL_C_BF16 | (SL_RES_BF16 if residual else 0) | (SL_RELU if relu else 0)
        dsc.x, dsc.ldx, dsc.w, dsc.bias = x, ldx, e.Ws(wkey), bias
        dsc.C, dsc.ldc, dsc.out_scale = Cp, ldc, out_scale
        dsc.drop_p, dsc.drop_site, dsc.drop_seed = 0.0, drop_site, 0
        dsc.residual, dsc.ldr, dsc.res_mod = residual, ldr, res_mod
        pre_saved = self._epilogue(dsc, gate, ldg, gate_scale, ln, drop=drop_site)
        meta = sl_meta(e.x3, e.strip_small, self.hh, e.g8, self.backward, M, N, K, ln is not None, pre_saved, bool(residual), bool(gate), c_planes, bool(x_drop_site))
        self.plan.append((self.lib.hftt_strip_linear, (C.byref(dsc),), 'strip_linear', meta))
        return dsc

    def linear(self, M, N, K, x, ldx, wkey, bias, Cp, ldc, c_planes=False, x_drop_site=0, **epilogue):
        """One linear layer C = epi(x . W[wkey]^T + bias) in this workspace's kernel family: the strip kernel on the strip pack, or the block
        GEMM on the prepared plane (storage formats follow from the tensors).  c_planes (C as f16-pair planes) and x_drop_site (x masked on
        load) exist in the x3 strip plans only: `planes()` and `mic` are false elsewhere."""
        if self.strip:
            return self.sl(M, N, K, x, ldx, wkey, bias, Cp, ldc, c_planes=c_planes, x_drop_site=x_drop_site, **epilogue)
        assert not c_planes and not x_drop_site
        return self.nt(M, N, K, x, ldx, self.eng.Wp(wkey), bias, Cp, ldc, **epilogue)

    def mlp(self, mode, M, x, wkey, y, b1=0, b2=0, h_out=0, gate=0, gate_scale=1.0, site_h=0, site_o=0, residual=0, ln=None):
        """fused two-GEMM block: mode 0 = hftt_ffn_res_ln_fwd (x -> relu/dropout hidden -> + x -> LayerNorm), mode 1 = hftt_ffn_bwd_dx."""
        e = self.eng
        d, p = e.d, e.p
        dsc = FfnDesc()
        dsc.M, dsc.d, dsc.p, dsc.mode = M, d, p, mode
        dsc.flags = ((SL_X3_F16 if mode == 0 else SL_X3_BF16) | (SL_H_BF16 | SL_PRE_BF16 if self.hh else 0) | (SL_X3_GRAD_HI if (mode == 1 and e.g8) else 0)) if e.x3 \
            else (SL_X_BF16 | SL_C_BF16 | SL_RES_BF16)
        dsc.x, dsc.ldx, dsc.w = x, d, e.Ws(wkey)
        dsc.b1, dsc.b2 = b1, b2
        dsc.h_out, dsc.ldh = h_out, p
        dsc.drop_p, dsc.site_h, dsc.site_o, dsc.drop_seed = 0.0, site_h, site_o, 0
        dsc.residual, dsc.ldr = residual, d
        dsc.y, dsc.ldy = y, d
        # mode 1: site_o = the dropout whose OUTPUT gradient the strip dy is (masked on load)
        pre_saved = self._epilogue(dsc, gate, p, gate_scale, ln, drop=(site_h or site_o) if mode == 0 else site_o)
        meta = mlp_meta(e.x3, e.strip_small, self.hh, e.g8, mode, M, d, p, bool(residual), pre_saved, bool(h_out), bool(gate))
        self.plan.append((self.lib.hftt_ffn_res_ln_fwd if mode == 0 else self.lib.hftt_ffn_bwd_dx, (C.byref(dsc),), 'ffn_fwd' if mode == 0 else 'ffn_bwd_dx', meta))
        return dsc

    def tn(self, M, N, K, dY, lddy, X, ldx, segs, K_out=None, out_scale=1.0, beta=0.0, dy_drop_site=0):
        """hftt_gemm_tn plan entry: dW = dY^T X.  segs: list of (row0, rows, dw_addr, db_addr or 0)"""
        e, ws = self.eng, self.ws
        ws['tn_need'] = max(ws.get('tn_need', 0), self.lib.hftt_gemm_tn_ws_bytes(M, N, K))
        dsc = GemmTnDesc()
        dsc.M, dsc.N, dsc.K, dsc.npass = M, N, K, (4 if e.npass == 2 else e.npass)
        dy_bf, x_bf = self.is_bf16(dY), self.is_bf16(X)
        dsc.io_flags = (1 if dy_bf else 0) | (2 if x_bf else 0) | (4 if (e.g8 and not dy_bf) else 0) | (8 if dy_drop_site else 0)
        if dy_drop_site:                             # HFTT_TN_DY_DROP: dY (fp32, the LayerNorm backward's dr) is masked while it is loaded
            assert not dy_bf and lddy == N and not e.g8
            dsc.drop_p, dsc.drop_site, dsc.drop_seed = 0.0, dy_drop_site, 0
            ws['drop'].append(dsc)
        dsc.dY, dsc.lddy, dsc.X, dsc.ldx = dY, lddy, X, ldx
        dsc.out_scale, dsc.beta = out_scale, beta
        dsc.n_seg = len(segs)
        for i, (r0, rows, dw, db) in enumerate(segs):
            dsc.seg_row0[i], dsc.seg_rows[i], dsc.seg_dw[i], dsc.seg_db[i] = r0, rows, dw, db
        dsc.K_out = K_out or K
        ws['tn'].append(dsc)
        ws['keep'].append(dsc)
        self.plan.append((self.lib.hftt_gemm_tn, (C.byref(dsc),), 'gemm_tn', tn_meta(dsc.npass, M, N, K, dy_bf, x_bf, bool(dsc.io_flags & 4), bool(dy_drop_site))))
        return dsc

    def attn(self, bwd, n_seq, H, Lq, Lk, q, qss, ldq, k, kss, ldk, v, vss, ldv, out, oss, ldo, lse, probs=0,
             drop_site=0, dout=0, dq=0, dqss=0, lddq=0, dk=0, dkss=0, lddk=0, dv=0, dvss=0, lddv=0, flags=0, planes=False, map_out=False):
        e = self.eng
        flags = (flags if e.sb else 0) | ((ATTN_Q_F16PAIR | ATTN_KV_F16PAIR) if planes else 0)
        dsc = AttnDesc()
        dsc.io_flags = flags
        dsc.n_seq, dsc.n_heads, dsc.Lq, dsc.Lk, dsc.dh, dsc.npass = n_seq, H, Lq, Lk, e.d // H, e.npass
        dsc.q, dsc.q_seq_stride, dsc.ldq = q, qss, ldq
        dsc.k, dsc.k_seq_stride, dsc.ldk = k, kss, ldk
        dsc.v, dsc.v_seq_stride, dsc.ldv = v, vss, ldv
        dsc.out, dsc.o_seq_stride, dsc.ldo = out, oss, ldo
        dsc.lse, dsc.probs = lse, probs
        dsc.drop_p, dsc.drop_site, dsc.drop_seed = 0.0, drop_site, 0
        dsc.dout = dout
        dsc.dq, dsc.dq_seq_stride, dsc.lddq = dq, dqss, lddq
        dsc.dk, dsc.dk_seq_stride, dsc.lddk = dk, dkss, lddk
        dsc.dv, dsc.dv_seq_stride, dsc.lddv = dv, dvss, lddv
        if drop_site:
            self.ws['drop'].append(dsc)
        self.ws['keep'].append(dsc)
        dm = 0 if (not (drop_site and e.dropout > 0.0) or self.inference) else (1 if (Lk % 4 == 0 and (n_seq * H * Lq * Lk) >> 34 == 0) else 2)
        meta = attn_meta(e.npass, bwd, n_seq, H, Lq, Lk, e.d, flags, planes, bool(probs or map_out), dm)
        self.plan.append((self.lib.hftt_attn_bwd if bwd else self.lib.hftt_attn_fwd, (C.byref(dsc),), 'attn_bwd' if bwd else 'attn_fwd', meta))
        return dsc

    def lnb(self, M, dy, r, mean, rstd, gamma, dr, dr_drop, drop_site, dgamma, dbeta, beta):
        """LayerNorm backward + the reduction of its per-workgroup dgamma / dbeta partials (beta: accumulate onto the gradient)"""
        e, ws = self.eng, self.ws
        n_wg = self.lib.hftt_ln_bwd_wgs(M)
        ws['ln_need'] = max(ws.get('ln_need', 0), n_wg * 2 * e.d * 4)
        dsc = LnBwdDesc()
        dsc.M, dsc.N = M, e.d
        dsc.dy, dsc.r, dsc.mean, dsc.rstd, dsc.gamma = dy, r, mean, rstd, gamma
        dsc.dr, dsc.dr_drop = dr, dr_drop
        dsc.drop_bf16 = 1 if self.is_bf16(dr_drop) else 0
        dsc.io_flags = (1 if self.is_bf16(dy) else 0) | (2 if self.is_bf16(dr) else 0) | (4 if self.is_bf16(r) else 0)
        dsc.drop_p, dsc.drop_site, dsc.drop_seed = 0.0, drop_site, 0
        ws['ln'].append(dsc)
        if drop_site:
            ws['drop'].append(dsc)
        ws['keep'].append(dsc)
        self.plan.append((self.lib.hftt_ln_bwd, (C.byref(dsc),), 'ln_bwd', None))
        self.plan.append(('ln_reduce', (n_wg, e.d, dgamma, dbeta, beta), 'ln_bwd_reduce', None))

    # ------------------------------------------------------------------ the model's blocks.  Buffers of a block: <tag>.<name>
    def _ln_params(self, pre):
        e = self.eng
        return e.P(pre + 'layer_norm.weight'), e.P(pre + 'layer_norm.bias'), e.G(pre + 'layer_norm.weight'), e.G(pre + 'layer_norm.bias')

    def self_attn_fwd(self, tag, pre, S, n_seq, L, H, x_in, save):
        """qkv projection -> attention -> fc_o + dropout + residual + LayerNorm (model_spec2midi.py:230-240).  Returns (output address, sites)"""
        e, d = self.eng, self.eng.d
        hz = 2 if e.sb else 4                       # element size of the GEMM-only ("half") tensors
        qkv = self.buf(tag + '.qkv', S, 3 * d, half=True)
        ctx = self.buf(tag + '.ctx', S, d, half=True)
        lse = self.buf(tag + '.lse', n_seq * H * L * 2)
        r1 = self.pbuf(tag + '.r1', S, d); x1 = self.abuf(tag + '.x1', S, d)
        m1 = self.buf(tag + '.m1', S); s1 = self.buf(tag + '.s1', S)
        sa, so = self.new_site(), self.new_site()
        sv = (lambda t: t.data_ptr()) if save else (lambda t: 0)
        gam, bet, _, _ = self._ln_params(pre)
        pln = self.planes(H, L, L)
        self.linear(S, 3 * d, d, x_in, d, tag + '.sa.qkv', e.Fp(tag + '.sa.qkv_b'), qkv.data_ptr(), 3 * d, c_planes=pln)
        q = qkv.data_ptr()
        self.attn(False, n_seq, H, L, L, q, L * 3 * d, 3 * d, q + hz * d, L * 3 * d, 3 * d, q + 2 * hz * d, L * 3 * d, 3 * d,
                  ctx.data_ptr(), L * d, d, lse.data_ptr(), drop_site=sa, flags=1 | 2 | 4, planes=pln)
        self.linear(S, d, d, ctx.data_ptr(), d, tag + '.sa.o', e.P(pre + 'self_attention.fc_o.bias'), x1.data_ptr(), d,
                    drop_site=so, residual=x_in, ldr=d, ln=(gam, bet, sv(r1), sv(m1), sv(s1)))
        return x1.data_ptr(), (sa, so)

    def ffn_fwd(self, tag, pre, S, x_in, save):
        """fc_1 + ReLU + dropout -> fc_2 + dropout + residual + LayerNorm (model_spec2midi.py:241-245).  Returns (output address, sites)"""
        e, d, p = self.eng, self.eng.d, self.eng.p
        h = self.buf(tag + '.h', S, p, half=True, hidden=True)
        r2 = self.pbuf(tag + '.r2', S, d); x2 = self.abuf(tag + '.x2', S, d)
        m2 = self.buf(tag + '.m2', S); s2 = self.buf(tag + '.s2', S)
        sh, sf = self.new_site(), self.new_site()
        sv = (lambda t: t.data_ptr()) if save else (lambda t: 0)
        gam, bet, _, _ = self._ln_params(pre)
        b1, b2 = e.P(pre + 'positionwise_feedforward.fc_1.bias'), e.P(pre + 'positionwise_feedforward.fc_2.bias')
        ln = (gam, bet, sv(r2), sv(m2), sv(s2))
        if self.strip:
            self.mlp(0, S, x_in, tag + '.ffn', x2.data_ptr(), b1=b1, b2=b2, h_out=sv(h), site_h=sh, site_o=sf, ln=ln)
        else:
            self.nt(S, p, d, x_in, d, e.Wp(tag + '.f1'), b1, h.data_ptr(), p, act=1, drop_site=sh)
            self.nt(S, d, p, h.data_ptr(), p, e.Wp(tag + '.f2'), b2, x2.data_ptr(), d, drop_site=sf, residual=x_in, ldr=d, ln=ln)
        return x2.data_ptr(), (sh, sf)

    def enc_layer_fwd(self, tag, pre, S, n_seq, L, H, x_in, save):
        """EncoderLayer (model_spec2midi.py:230-245).  Returns address of the layer output [S, d]."""
        x1, s_attn = self.self_attn_fwd(tag, pre, S, n_seq, L, H, x_in, save)
        x2, s_ffn = self.ffn_fwd(tag, pre, S, x1, save)
        self.ws['sites'][tag] = s_attn + s_ffn
        return x2

    # backward blocks: the gradient of the block's output arrives in GA and the gradient of its input leaves in GA.
    # G = (GA stream, GB the LayerNorm backward's dr, GC its dropout-masked copy, Gh dh, Gq dqkv, Gx dctx)
    def _ln_bwd(self, tag, n, pre, S, G, site, beta):
        """LayerNorm n (1: behind fc_o, 2: behind the FFN) backward.  Returns dbr: what the dropout in front of the sum hands back"""
        GA, GB, GC = G[:3]
        b = self.ws['bufs']
        gam, _, dgam, dbet = self._ln_params(pre)
        masked = self.eng.dropout > 0.0 and not self.mic
        self.lnb(S, GA, b['%s.r%d' % (tag, n)].data_ptr(), b['%s.m%d' % (tag, n)].data_ptr(), b['%s.s%d' % (tag, n)].data_ptr(), gam,
                 GB, GC if masked else 0, site, dgam, dbet, beta)
        return GC if masked else GB

    def ffn_bwd(self, tag, pre, S, x_in, G, sites, ln_beta):
        """strip plans: the two dX GEMMs are one fused launch (hftt_ffn_bwd_dx)"""
        e, d, p = self.eng, self.eng.d, self.eng.p
        GA, GB, GC, Gh, Gq, Gx = G
        sh, sf = sites
        h = self.ws['bufs'][tag + '.h'].data_ptr()
        pf = pre + 'positionwise_feedforward.'
        dbr = self._ln_bwd(tag, 2, pre, S, G, sf, ln_beta)
        self.tn(S, d, p, dbr, d, h, p, [(0, d, e.G(pf + 'fc_2.weight'), e.G(pf + 'fc_2.bias'))], dy_drop_site=sf if self.mic else 0)
        if self.strip:
            self.mlp(1, S, dbr, tag + '.ffn_t', GA, h_out=Gh, gate=h, gate_scale=('inv_keep',), residual=GB, site_o=sf if self.mic else 0)
        else:
            self.nt(S, p, d, dbr, d, e.Wp(tag + '.f2_t'), 0, Gh, p, gate=h, ldg=p, gate_scale=('inv_keep',))
        self.tn(S, p, d, Gh, p, x_in, d, [(0, p, e.G(pf + 'fc_1.weight'), e.G(pf + 'fc_1.bias'))])
        if not self.strip:
            self.nt(S, d, p, Gh, p, e.Wp(tag + '.f1_t'), 0, GA, d, residual=GB, ldr=d)

    def self_attn_bwd(self, tag, pre, S, n_seq, L, H, x_in, G, sites, dx_fp32=False):
        """dx_fp32: the bf16 gradient stream of HFTT_BF16_GRAD ends with this block's dX"""
        e, d = self.eng, self.eng.d
        GA, GB, GC, Gh, Gq, Gx = G
        sa, so = sites
        b = self.ws['bufs']
        hz = 2 if e.sb else 4
        pa = pre + 'self_attention.'
        qkv, ctx = b[tag + '.qkv'].data_ptr(), b[tag + '.ctx'].data_ptr()
        dbr = self._ln_bwd(tag, 1, pre, S, G, so, 1.0)
        self.tn(S, d, d, dbr, d, ctx, d, [(0, d, e.G(pa + 'fc_o.weight'), e.G(pa + 'fc_o.bias'))], dy_drop_site=so if self.mic else 0)
        self.linear(S, d, d, dbr, d, tag + '.sa.o_t', 0, Gx, d, x_drop_site=so if self.mic else 0)
        self.attn(True, n_seq, H, L, L, qkv, L * 3 * d, 3 * d, qkv + hz * d, L * 3 * d, 3 * d, qkv + 2 * hz * d, L * 3 * d, 3 * d,
                  ctx, L * d, d, b[tag + '.lse'].data_ptr(), drop_site=sa, dout=Gx,
                  dq=Gq, dqss=L * 3 * d, lddq=3 * d, dk=Gq + hz * d, dkss=L * 3 * d, lddk=3 * d, dv=Gq + 2 * hz * d, dvss=L * 3 * d, lddv=3 * d,
                  flags=1 | 2 | 4 | 8 | 16, planes=self.planes(H, L, L))
        self.tn(S, 3 * d, d, Gq, 3 * d, x_in, d, [(i * d, d, e.G(pa + n + '.weight'), e.G(pa + n + '.bias')) for i, n in enumerate(('fc_q', 'fc_k', 'fc_v'))])
        if dx_fp32:
            self._bf16_content.discard(GA)
        self.linear(S, d, 3 * d, Gq, 3 * d, tag + '.sa.qkv_t', 0, GA, d, residual=GB, ldr=d)

    def enc_layer_bwd(self, tag, pre, S, n_seq, L, H, x_in, G, dx_fp32=False):
        sa, so, sh, sf = self.ws['sites'][tag]
        self.ffn_bwd(tag, pre, S, self.ws['bufs'][tag + '.x1'].data_ptr(), G, (sh, sf), 0.0)
        self.self_attn_bwd(tag, pre, S, n_seq, L, H, x_in, G, (sa, so), dx_fp32)

    # ------------------------------------------------------------------ the plans
    def build(self):
        eng, ws = self.eng, self.ws
        self.forward(save=True)
        if self.strip:                               # inference plan: same buffers, nothing saved for a backward
            n_sites, self.site, self.inference = self.site, 0, True
            self.forward(save=False)
            self.inference = False
            assert self.site == n_sites
        self.backward = True
        self.build_backward()
        tnb = torch.empty(max(ws.get('tn_need', 8), 8) // 4 + 16, dtype=torch.float32, device=eng.device)
        lnb = torch.empty(max(ws.get('ln_need', 8), 8) // 4 + 16, dtype=torch.float32, device=eng.device)
        ws['bufs']['tn_ws'], ws['bufs']['ln_ws'] = tnb, lnb
        for dsc in ws['tn']:
            dsc.ws, dsc.ws_bytes = tnb.data_ptr(), tnb.numel() * 4
        for dsc in ws['ln']:
            dsc.ws = lnb.data_ptr()
        ws['ln_ws_ptr'] = lnb.data_ptr()
        return ws

    def build_decoder_backward(self):
        """The frozen-encoder backward plan of a finished workspace (PlanBuilder(eng, B, ws)), built on first use by the same builder code
        (build_backward(enc_grad=False)): it declares no new tensor and its products are shapes the full plan already has, so the two workspaces are shared as they are."""
        ws = self.ws
        if 'bwd_dec' in ws:
            return
        need, n_tn, n_ln, n_buf = (ws.get('tn_need'), ws.get('ln_need')), len(ws['tn']), len(ws['ln']), len(ws['bufs'])
        self.backward = True
        self.build_backward(enc_grad=False)
        assert (ws.get('tn_need'), ws.get('ln_need')) == need and len(ws['bufs']) == n_buf
        tnb, lnb = ws['bufs']['tn_ws'], ws['bufs']['ln_ws']
        for dsc in ws['tn'][n_tn:]:
            dsc.ws, dsc.ws_bytes = tnb.data_ptr(), tnb.numel() * 4
        for dsc in ws['ln'][n_ln:]:
            dsc.ws = lnb.data_ptr()

    def forward(self, save=True):
        """save=True: the training plan (everything a backward needs is written); save=False (strip mode only): the inference plan --
        no pre-LayerNorm sums, statistics or hidden activations are stored."""
        e, ws = self.eng, self.ws
        B, T, F, N, d = ws['B'], e.T, e.F, e.N, e.d
        Se, Sn, BT, BN = B * T * F, B * T * N, B * T, B * N
        plan = self.plan = []
        ws['sites'] = {}
        st, bs = self.strip, self.bfs
        self.buf('spec', B, F, e.W)
        win = self.buf('win', Se, e.Kp)
        x0 = self.abuf('x0', Se, d)
        enc_ = 'encoder_spec2midi.'
        plan.append(('im2win', (win.data_ptr(), B, F, T, e.n_proc, e.Kp), 'im2win', None))       # (the source pointer is this forward's: ws['spec_ptr'])
        s_emb = self.new_site()
        ws['sites']['embed'] = s_emb
        self.nt(Se, d, e.Kp, win.data_ptr(), e.Kp, e.Wp('embed'), e.Fp('embed_b'), x0.data_ptr(), d,
                out_scale=math.sqrt(d), add_table=e.P(enc_ + 'pos_embedding_freq.weight'), add_mod=F, drop_site=s_emb)
        x = x0.data_ptr()
        ws['enc_in'] = [x]
        for i in range(e.Le):
            x = self.enc_layer_fwd(f'enc{i}', f'{enc_}layers_freq.{i}.', Se, BT, F, e.He, x, save)
            ws['enc_in'].append(x)
        enc = x
        # ---------------- decoder, frequency axis (cross attention notes x bins) ----------------
        dd = 'decoder_spec2midi.'
        H = e.Hd
        pos_dec = e.P(dd + 'pos_embedding_freq.weight')
        hz = 2 if e.sb else 4
        q0 = self.buf('dec0.q0', N, d, half=True)
        trg = None
        ws['dec_out'] = []
        sv = (lambda t: t.data_ptr()) if save else (lambda t: 0)
        plc = self.planes(H, N, F)
        for j in range(e.Ld):
            tag = f'dec{j}'
            sites = {}
            ws['sites'][tag] = sites
            pre = dd + ('layer_zero_freq.' if j == 0 else f'layers_freq.{j - 1}.')
            gam, bet, _, _ = self._ln_params(pre)
            if j > 0:
                cross_in, sites['self'] = self.self_attn_fwd(tag, pre, Sn, BT, N, H, trg, save)
                cq = self.buf(tag + '.cq', Sn, d, half=True)
                self.linear(Sn, d, d, cross_in, d, tag + '.ca.q', e.P(pre + 'encoder_attention.fc_q.bias'), cq.data_ptr(), d, c_planes=plc)
                qaddr, qss = cq.data_ptr(), N * d
                res, res_mod = cross_in, 0
            else:
                # layer zero: query = fc_q(pos_embedding_freq) shared by all sequences -- N rows, always the block GEMM
                self.nt(N, d, d, pos_dec, d, e.Wp(tag + '.ca.q'), e.P(pre + 'encoder_attention.fc_q.bias'), q0.data_ptr(), d)
                qaddr, qss = q0.data_ptr(), 0
                if plc:                               # the shared query of layer zero comes from the block GEMM as fp32: one small conversion
                    q0p = self.buf('dec0.q0p', N, d)
                    plan.append((self.lib.hftt_x3_to_planes, (q0.data_ptr(), d, q0p.data_ptr(), d, N, d), 'x3_to_planes', None))
                    qaddr = q0p.data_ptr()
                res, res_mod = (e.wbf.data_ptr() + 2 * e.Woff['dec_pos_bf'] if bs else pos_dec), N
            merged = st and e.merge_ckv
            ldkv = (e.Ld if merged else 1) * 2 * d
            if merged:
                ckv = self.buf('dec.ckv_all', Se, ldkv)
                if j == 0:                            # one projection for every layer's K / V (the layers' column blocks of one [Se, Ld * 2d] plane tensor)
                    self.sl(Se, ldkv, d, enc, d, 'dec.ca.kv_all', e.Fp('dec.ca.kv_all_b'), ckv.data_ptr(), ldkv, c_planes=True)
            else:
                ckv = self.buf(tag + '.ckv', Se, 2 * d, half=True)
            cctx = self.buf(tag + '.cctx', Sn, d, half=True)
            clse = self.buf(tag + '.clse', BT * H * N * 2)
            cr = self.pbuf(tag + '.cr', Sn, d); cx = self.abuf(tag + '.cx', Sn, d)
            cm = self.buf(tag + '.cm', Sn); cs = self.buf(tag + '.cs', Sn)
            c_a, c_o = self.new_site(), self.new_site()
            sites['cross'] = (c_a, c_o)
            if not merged:
                self.linear(Se, 2 * d, d, enc, d, tag + '.ca.kv', e.Fp(tag + '.ca.kv_b'), ckv.data_ptr(), 2 * d, c_planes=plc)
            kk = ckv.data_ptr() + (j * 2 * d * hz if merged else 0)
            ws.setdefault('ckv_at', {})[tag] = (kk, ldkv)
            ad = self.attn(False, BT, H, N, F, qaddr, qss, d, kk, F * ldkv, ldkv, kk + hz * d, F * ldkv, ldkv,
                           cctx.data_ptr(), N * d, d, clse.data_ptr(), drop_site=c_a, flags=1 | 2 | 4, planes=plc, map_out=(j == e.Ld - 1))
            if j == e.Ld - 1:
                ws.setdefault('attn_out_descs', []).append(ad)
            self.linear(Sn, d, d, cctx.data_ptr(), d, tag + '.ca.o', e.P(pre + 'encoder_attention.fc_o.bias'), cx.data_ptr(), d,
                        drop_site=c_o, residual=res, ldr=d, res_mod=res_mod, ln=(gam, bet, sv(cr), sv(cm), sv(cs)))
            trg, sites['ffn'] = self.ffn_fwd(tag, pre, Sn, cx.data_ptr(), save)
            ws['dec_out'].append(trg)
        # ---------------- heads A ----------------
        logits_f = self.buf('logits_f', Sn, e.NHp)
        self.nt(Sn, e.NH, d, trg, d, e.Wp('heads_f'), e.Fp('heads_f_b'), logits_f.data_ptr(), e.NHp)
        plan.append(('heads', (logits_f.data_ptr(), 0), 'heads_split', None))
        # ---------------- decoder, time axis ----------------
        y0 = self.abuf('y0', Sn, d)
        s_t = self.new_site()
        ws['sites']['time_embed'] = s_t
        plan.append(('time_embed', (trg, e.P(dd + 'pos_embedding_time.weight'), y0.data_ptr(), s_t, 3 if bs else 0), 'time_embed_fwd', None))
        y = y0.data_ptr()
        ws['time_in'] = [y]
        for i in range(e.Ld):
            y = self.enc_layer_fwd(f'time{i}', f'{dd}layers_time.{i}.', Sn, BN, T, H, y, save)
            ws['time_in'].append(y)
        logits_t = self.buf('logits_t', Sn, e.NHp)
        self.nt(Sn, e.NH, d, y, d, e.Wp('heads_t'), e.Fp('heads_t_b'), logits_t.data_ptr(), e.NHp)
        plan.append(('heads', (logits_t.data_ptr(), 1), 'heads_split', None))
        if e.x3 and st and not e.strip_small and (e.fuse_offn_opt == 'all' or (e.fuse_offn_opt == 'inference' and not save)):
            plan = self._fuse_attn_out_ffn(plan, save)
        ws['fwd' if save else 'fwd_inf'] = plan
        ws['enc'] = enc

    def _fuse_attn_out_ffn(self, plan, save):
        """Peephole over a forward plan: hftt_strip_linear (fc_o + dropout + residual + LayerNorm, 256 -> 256) directly followed by the
        hftt_ffn_res_ln_fwd that reads its output becomes ONE hftt_attn_out_ffn_fwd launch on the same two descriptors (their dropout sites, saved
        tensors and statistics unchanged); in the inference plan the LayerNorm-1 output is not written at all.  The launch reads the two
        weight packs as one stream: WeightLayout asserts that a block's FFN pack follows its fc_o pack."""
        out, i = [], 0
        while i < len(plan):
            e = plan[i]
            nx = plan[i + 1] if i + 1 < len(plan) else None
            if nx is not None and e[2] == 'strip_linear' and nx[2] == 'ffn_fwd':
                o, f = e[1][0]._obj, nx[1][0]._obj
                if (o.ln_gamma and o.N == 256 and o.K == 256 and o.residual and f.mode == 0 and f.d == 256 and f.p == 512 and f.x == o.C
                        and f.w == o.w + 2 * 2 * 256 * 256 and not o.gate and not f.residual):
                    if not save:
                        o.C = 0                           # (x1 lives in registers only)
                    mo, mf = e[3], nx[3]
                    M = o.M
                    meta = {'kernel': 'x3_oln_mlp_kernel<%s>' % _tf(self.hh), 'flops': mo['flops'] + mf['flops'],
                            'bytes': mo['bytes'] + mf['bytes'] - 4.0 * M * 256 * (1 if save else 2), 'shape': (M, 256, 512), 'saves': mf.get('saves', False),
                            'fused': ('strip_linear', 'ffn_fwd'), 'ffn_flops': mf['flops']}
                    out.append((self.lib.hftt_attn_out_ffn_fwd, (e[1][0], nx[1][0]), 'ffn_fwd', meta))
                    i += 2
                    continue
            out.append(e)
            i += 1
        return out

    def build_backward(self, enc_grad=True):
        """enc_grad=False: the backward of a model whose encoder is frozen -- the same layers, without the launches that form the encoder-output
        gradient, ending where the frequency decoder's range is final (ws['bwd_dec'], two marks); nothing below the decoder is written"""
        e, ws = self.eng, self.ws
        B, T, F, N, V, d, p = ws['B'], e.T, e.F, e.N, e.V, e.d, e.p
        Se, Sn, BT, BN = B * T * F, B * T * N, B * T, B * N
        b = ws['bufs']
        plan = self.plan = []
        H = e.Hd
        dd = 'decoder_spec2midi.'
        enc_ = 'encoder_spec2midi.'
        use_drop = e.dropout > 0.0
        st, bs = self.strip, self.bfs               # strip kernels; bs: on the bf16 stream (then the whole gradient stream is bf16)
        # bf16 gradient stream on the bin-token (encoder-sized) set: the residual-stream gradient and the LN-backward output stored
        # as bf16 between the decoder's cross-attention and the first encoder layer.  Built, parity-tested and MEASURED (r01, B=8):
        # ln_bwd 90.9 -> 79.5 us, but the dX GEMMs' row-pass epilogue then moves 8 bytes per lane instead of 16 and gets slower
        # (K=512: 253 -> 284 us, K=768: 324 -> 366 us) -- net zero, so it is OFF by default (HFTT_BF16_GRAD=1 enables) until the
        # row pass handles 8 columns per lane for bf16 residual / C.
        # (needs the A-stationary GEMM on every encoder dX: d % 256 == 0, K = ff and 3d <= 768, >= 256 bin tokens)
        egb = (not st and e.sb and os.environ.get('HFTT_BF16_GRAD', '0') == '1' and d % 256 == 0 and max(p, 3 * d) <= 768 and Se >= 256)
        ws['bf16_grad'] = bool(egb or bs)
        # gradient scratch: note-token sized and bin-token sized sets
        nGA = self.abuf('g.nA', Sn, d).data_ptr(); nGB = self.abuf('g.nB', Sn, d).data_ptr()
        hz = 2 if e.sb else 4
        nGC = self.buf('g.nC', Sn, d, half=True).data_ptr(); nGD = self.abuf('g.nD', Sn, d).data_ptr()
        nGh = self.buf('g.nh', Sn, p, half=True, hidden=True).data_ptr(); nGq = self.buf('g.nq', Sn, 3 * d, half=True).data_ptr()
        nGx = self.buf('g.nx', Sn, d, half=True).data_ptr()
        q1f = self.buf('g.q1f', Sn, d).data_ptr() if bs else 0          # layer zero's per-sequence dq stays fp32 (summed over sequences)
        eGA = self.abuf('g.eA', Se, d).data_ptr(); eGB = self.abuf('g.eB', Se, d).data_ptr()
        eGC = self.buf('g.eC', Se, d, half=True).data_ptr()
        eGh = self.buf('g.eh', Se, p, half=True, hidden=True).data_ptr(); eGq = self.buf('g.eq', Se, 3 * d, half=True).data_ptr()
        eGx = self.buf('g.ex', Se, d, half=True).data_ptr()
        if egb:                                      # (declared as fp32 stream tensors, half used)
            self._bf16_content.update((eGA, eGB))
        dlog = self.buf('g.dlog', Sn, e.NHp).data_ptr()
        cs_n = max(F * d, N * d, T * d)
        cs_ws = self.buf('g.cs', self.lib.hftt_colsum_ws_bytes(1, cs_n) // 4 + 16).data_ptr()
        dq0s = self.buf('g.dq0', N * d).data_ptr()
        # incoming gradients of the 8 differentiable outputs (filled by the loss kernel or by autograd glue)
        for nm in ('onset_A', 'offset_A', 'mpe_A', 'onset_B', 'offset_B', 'mpe_B'):
            self.buf('d.' + nm, Sn)
        self.buf('d.velocity_A', Sn, V); self.buf('d.velocity_B', Sn, V)

        def head_segs(tag):
            return [(r0, rows, e.G(f'{dd}fc_{nm}_{tag}.weight'), e.G(f'{dd}fc_{nm}_{tag}.bias'))
                    for r0, rows, nm in ((0, V, 'velocity'), (V, 1, 'onset'), (V + 1, 1, 'offset'), (V + 2, 1, 'mpe'))]

        # ---- heads B + time layers ----
        plan.append(('heads_bwd', ('B', dlog, 1), 'heads_split_bwd', None))
        self.tn(Sn, e.NHp, d, dlog, e.NHp, ws['time_in'][-1], d, head_segs('time'))
        self.nt(Sn, d, e.NHp, dlog, e.NHp, e.Wp('heads_t_t'), 0, nGA, d)
        Gn = (nGA, nGB, nGC, nGh, nGq, nGx)
        for i in reversed(range(e.Ld)):
            self.enc_layer_bwd(f'time{i}', f'{dd}layers_time.{i}.', Sn, BN, T, H, ws['time_in'][i], Gn)
        # ---- heads A, then the time-embedding transpose back onto the note-major gradient ----
        # (heads A's weight-gradient product writes the FREQUENCY range of flat_grads: it is emitted behind the first mark below, so that the
        #  plan's prefix up to that mark writes the time range and nothing else -- the backward of frozen_stages = 2.  Same launch, same
        #  operands: dlog is not written again in this backward)
        plan.append(('heads_bwd', ('A', dlog, 0), 'heads_split_bwd', None))
        self.nt(Sn, d, e.NHp, dlog, e.NHp, e.Wp('heads_f_t'), 0, nGD, d)
        plan.append(('time_embed_bwd', (nGA, nGD, nGB if use_drop else 0, ws['sites']['time_embed'], 7 if bs else 0), 'time_embed_bwd', None))
        plan.append(('colsum', (nGB if use_drop else nGA, BN, T * d, T * d, e.G(dd + 'pos_embedding_time.weight'), 0.0, cs_ws, 1 if bs else 0), 'colsum', None))
        # gradient buckets in the order they become final (flat ranges are contiguous: state_dict order is encoder,
        # frequency decoder + heads A, time decoder + heads B): (plan length when final, flat lo, flat hi)
        o_dec, o_time, o_end = e.poff[dd + 'pos_embedding_freq.weight'], e.poff[dd + 'pos_embedding_time.weight'], e.flat_grads.numel()
        marks = [(len(plan), o_time, o_end)]
        self.tn(Sn, e.NHp, d, dlog, e.NHp, ws['dec_out'][-1], d, head_segs('freq'))
        # ---- frequency decoder layers, last to first.  Gradient stream lives in A (= nGD), per-sequence dq in Q1 (= nGA);
        #      the encoder-output gradient accumulates in eGA ----
        A, Bf, Q1 = nGD, nGB, nGA
        Gd = (A, Bf, nGC, nGh, nGq, nGx)
        mic = self.mic
        first_enc_grad = True
        enc = ws['enc']
        plc = self.planes(H, N, F)
        # merged (x3 strip plans, three decoder layers): dk / dv of every layer go into the column blocks of ONE [Se, 6d] tensor; the weight
        # gradients (one product, six segments) and the encoder-output gradient (two K = 768 halves) are formed once, behind layer zero --
        # the encoder output is read once instead of three times, the accumulating gradient makes one round trip less
        mb = st and e.merge_ckv_bwd
        ldg = e.Ld * 2 * d if mb else 2 * d
        for j in reversed(range(e.Ld)):
            tag = f'dec{j}'
            pre = dd + ('layer_zero_freq.' if j == 0 else f'layers_freq.{j - 1}.')
            sites = ws['sites'][tag]
            pc = pre + 'encoder_attention.'
            self.ffn_bwd(tag, pre, Sn, b[tag + '.cx'].data_ptr(), Gd, sites['ffn'], 0.0)
            # ---- cross-attention block ----
            c_a, c_o = sites['cross']
            gam, _, dgam, dbet = self._ln_params(pre)
            masked = use_drop and not mic
            self.lnb(Sn, A, b[tag + '.cr'].data_ptr(), b[tag + '.cm'].data_ptr(), b[tag + '.cs'].data_ptr(), gam,
                     Bf, nGC if masked else 0, c_o, dgam, dbet, 1.0)
            dbr = nGC if masked else Bf
            self.tn(Sn, d, d, dbr, d, b[tag + '.cctx'].data_ptr(), d, [(0, d, e.G(pc + 'fc_o.weight'), e.G(pc + 'fc_o.bias'))], dy_drop_site=c_o if mic else 0)
            self.linear(Sn, d, d, dbr, d, tag + '.ca.o_t', 0, nGx, d, x_drop_site=c_o if mic else 0)
            kk, ldkv = ws['ckv_at'][tag]
            if j > 0:
                qaddr, qss = b[tag + '.cq'].data_ptr(), N * d
            else:
                qaddr, qss = b['dec0.q0p' if plc else 'dec0.q0'].data_ptr(), 0
            # dq (per sequence) -> Q1 ; dk,dv -> eGq viewed as [Se, 2d]
            # per-sequence dq stays fp32 (layer zero sums it over sequences with the fp32 colsum); dk, dv are "half" tensors
            # strip mode: dq of the layers with their own query projection is a GEMM operand only -> bf16; layer zero keeps fp32 (q1f)
            dq_buf = Q1 if not bs else (Q1 if j > 0 else q1f)
            gkv = (self.buf('g.ekv_all', Se, ldg).data_ptr() + j * 2 * d * 4) if mb else eGq
            self.attn(True, BT, H, N, F, qaddr, qss, d, kk, F * ldkv, ldkv, kk + hz * d, F * ldkv, ldkv,
                      b[tag + '.cctx'].data_ptr(), N * d, d, b[tag + '.clse'].data_ptr(), drop_site=c_a, dout=nGx,
                      dq=dq_buf, dqss=N * d, lddq=d, dk=gkv, dkss=F * ldg, lddk=ldg, dv=gkv + hz * d, dvss=F * ldg, lddv=ldg,
                      flags=1 | 2 | 4 | 16 | (8 if (st and j > 0) else 0), planes=plc)
            if mb:
                if j == 0:
                    gall = b['g.ekv_all'].data_ptr()
                    segs = []
                    for jj in range(e.Ld):
                        pcj = dd + ('layer_zero_freq.' if jj == 0 else f'layers_freq.{jj - 1}.') + 'encoder_attention.'
                        segs += [(2 * jj * d, d, e.G(pcj + 'fc_k.weight'), e.G(pcj + 'fc_k.bias')), ((2 * jj + 1) * d, d, e.G(pcj + 'fc_v.weight'), e.G(pcj + 'fc_v.bias'))]
                    self.tn(Se, ldg, d, gall, ldg, enc, d, segs)
                    if enc_grad:
                        self.sl(Se, d, 3 * d, gall, ldg, 'dec.ca.kv_all_t0', 0, eGA, d)
                        self.sl(Se, d, 3 * d, gall + 3 * d * 4, ldg, 'dec.ca.kv_all_t1', 0, eGA, d, residual=eGA, ldr=d)
            else:
                self.tn(Se, 2 * d, d, eGq, 2 * d, enc, d, [(0, d, e.G(pc + 'fc_k.weight'), e.G(pc + 'fc_k.bias')), (d, d, e.G(pc + 'fc_v.weight'), e.G(pc + 'fc_v.bias'))])
                # (strip kernels: in place -- a lane reads exactly the residual elements it then overwrites; their descriptor carries ldr either way)
                if enc_grad:
                    self.linear(Se, d, 2 * d, eGq, 2 * d, tag + '.ca.kv_t', 0, eGA, d, residual=0 if first_enc_grad else eGA,
                                ldr=d if (st or not first_enc_grad) else 0)
                first_enc_grad = False
            if j > 0:
                # q projection of the cross attention (input x1, which is also the residual of this block)
                self.tn(Sn, d, d, Q1, d, b[tag + '.x1'].data_ptr(), d, [(0, d, e.G(pc + 'fc_q.weight'), e.G(pc + 'fc_q.bias'))])
                self.linear(Sn, d, d, Q1, d, tag + '.ca.q_t', 0, A, d, residual=Bf, ldr=d)
                # self-attention block (input trg = previous layer output)
                self.self_attn_bwd(tag, pre, Sn, BT, N, H, ws['dec_out'][j - 1], Gd, sites['self'])
            else:
                # layer zero: query = fc_q(pos_embedding_freq) shared by all sequences, residual = pos_embedding_freq
                gpos = e.G(dd + 'pos_embedding_freq.weight')
                plan.append(('colsum', (Bf, BT, N * d, N * d, gpos, 0.0, cs_ws, 1 if bs else 0), 'colsum', None))       # residual path (undropped dr)
                plan.append(('colsum', (q1f if bs else Q1, BT, N * d, N * d, dq0s, 0.0, cs_ws, 0), 'colsum', None))     # sum of per-sequence dq
                self.tn(N, d, d, dq0s, d, e.P(dd + 'pos_embedding_freq.weight'), d, [(0, d, e.G(pc + 'fc_q.weight'), e.G(pc + 'fc_q.bias'))])
                self.nt(N, d, d, dq0s, d, e.Wp(tag + '.ca.q_t'), 0, gpos, d, residual=gpos, ldr=d)
        marks.append((len(plan), o_dec, o_time))
        if not enc_grad:                             # frozen encoder: no encoder layer backward, no embedding backward
            ws['bwd_dec'], ws['bwd_dec_marks'] = plan, marks
            return
        # ---- encoder layers ----
        Ge = (eGA, eGB, eGC, eGh, eGq, eGx)
        for i in reversed(range(e.Le)):
            self.enc_layer_bwd(f'enc{i}', f'{enc_}layers_freq.{i}.', Se, BT, F, e.He, ws['enc_in'][i], Ge, dx_fp32=(i == 0))     # the embedding stage below reads fp32
        # ---- embedding ----
        # (the dropout mask and the position-embedding gradient's column sum in one pass over the gradient: ld == n, so the element index is row * n + col)
        plan.append(('dropout_bwd_colsum', (eGA, BT, F * d, F * d, ws['sites']['embed'], e.G(enc_ + 'pos_embedding_freq.weight'), 0.0, cs_ws, 1 if bs else 0),
                     'dropout_bwd_colsum', None))
        self.tn(Se, d, e.Kp, eGA, d, b['win'].data_ptr(), e.Kp, [(0, d, e.dweff.data_ptr(), e.dbeff.data_ptr())], out_scale=math.sqrt(d))
        plan.append((self.lib.hftt_embed_fold_bwd, (C.byref(e.fold),), 'embed_fold_bwd', None))
        marks.append((len(plan), 0, o_dec))
        ws['bwd'] = plan
        ws['bwd_marks'] = marks
