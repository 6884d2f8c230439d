"""Host-side engine of the MI355X hFT-Transformer path.

It owns (a) ONE flat fp32 parameter buffer + ONE flat gradient buffer (the module's nn.Parameters are views
into the first), (b) the prepared bf16 weight planes the MFMA kernels consume, (c) all activation /
gradient workspaces for a batch size, and (d) pre-built launch plans: lists of C-ABI calls
(libhftt_hip.so) with their descriptors filled in once, replayed every step on torch's current HIP stream.

Where the prepared weights live is computed by hftt_hip/layout.py (pure arithmetic), the plans are written by hftt_hip/plan.py;
this file allocates, uploads and runs.

PyTorch is used for device memory, streams and autograd glue only; every arithmetic op of the path is a
HIP kernel behind the C ABI (include/hftt_hip.h).  There is no fallback: without the library or on a CPU
tensor the engine raises.

Reference algorithm: hftt_code/model/model_spec2midi.py (forward), training/train.py:141-159 (loss,
backward, step).  Shapes follow the reference: T frames, F bins, N notes, V velocities, d hidden, p ffn.
"""
from __future__ import annotations

import ctypes as C
import math
import os

import torch

from . import _capi
from ._capi import FoldDesc, LossDesc, LossWDesc, PrepEntry, StripPackEntry, check, lib
from .layout import PRECISION_NPASS, Options, WeightLayout, _align, flat_offsets, model_dims, precision_modes   # noqa: F401  (PRECISION_NPASS: re-export)
from .plan import PlanBuilder, attn_fwd8_takes   # noqa: F401  (attn_fwd8_takes: re-export)


def keep_scale(p):
    """scale of the kept elements of a dropout site (csrc/hftt_common.h: hftt_keep_scale): 256 / thr, thr = round((1 - p) * 256) -- the
    reciprocal of the keep probability the 8-bit generator actually applies, so E[dropout(x)] = x exactly (nn.Dropout's contract)."""
    if not p > 0.0:
        return 1.0
    import numpy as np
    kk = (1.0 - float(np.float32(p))) * 256.0 + 0.5
    thr = 256 if kk >= 256.0 else (0 if kk <= 0.0 else int(kk))
    return float(np.float32(256.0) / np.float32(thr)) if thr > 0 else 0.0


def _table(entry_type, rows):
    return torch.frombuffer(bytearray(bytes((entry_type * len(rows))(*[entry_type(*r) for r in rows]))), dtype=torch.uint8)


class HfttEngine:
    _dropout_notice_given = False

    def __init__(self, cfg, device, precision='parity', dropout=0.0, seed=1234):
        """cfg: dict with n_margin,n_frame,n_bin,cnn_channel,cnn_kernel,hid_dim,pf_dim,enc_layer,dec_layer,
        enc_head,dec_head,n_note,n_velocity (the constructor arguments of the reference classes)."""
        self.lib = lib()
        self.cfg = dict(cfg)
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise _capi.HfttError('HfttEngine needs a ROCm device (got %s): the HIP kernels are the only compute path' % device)
        self.dims = model_dims(self.cfg)
        vars(self).update(vars(self.dims))          # T, F, N, V, d, p, He, Hd, Le, Ld, n_proc, Kp, W, nw, NH, NHp
        if self.d % 32 or self.p % 32 or self.d not in (64, 128, 256):
            raise _capi.HfttError('hid_dim must be 64/128/256 and pf_dim a multiple of 32 (got %d/%d)' % (self.d, self.p))
        for h in (self.He, self.Hd):
            if self.d % h or (self.d // h) not in (32, 64):
                raise _capi.HfttError('head_dim must be 32 or 64 (hid_dim %d, heads %d)' % (self.d, h))
        if max(self.T, self.F, self.N) > 256:
            raise _capi.HfttError('sequence axes must be <= 256')
        if self.V % 4:
            raise _capi.HfttError('n_velocity must be a multiple of 4')
        env = os.environ.get
        self.store_bf16_opt = env('HFTT_BF16_STORE', '1') != '0'
        self.strip_opt = env('HFTT_STRIP', '1') != '0'
        self.planes_opt = env('HFTT_X3_PLANES', '1') != '0'      # x3 strip plans: q / k / v between projection and attention as f16-pair planes
        self.merge_ckv_opt = env('HFTT_X3_MERGE_CKV', '1') != '0'      # (see WeightLayout.merge_ckv)
        self.opts = Options(store_bf16=self.store_bf16_opt, strip=self.strip_opt, planes=self.planes_opt, merge_ckv=self.merge_ckv_opt)
        # x3 strip plans (d = 256): the LayerNorm backward writes NO dropout-masked copy of its result; its consumers -- the weight-gradient
        # product (HFTT_TN_DY_DROP), the fused FFN's dX (site_o) and the fc_o dX (HFTT_SL_X_DROP) -- apply the mask while they load dr
        self.ln_mask_in_consumers_opt = env('HFTT_X3_LN_MASK_IN_CONSUMERS', '1') != '0'
        # round 6 (ABI v8): fc_o + residual + LayerNorm and the FFN block behind it as ONE launch (hftt_attn_out_ffn_fwd) -- 'all' in both forward plans,
        # 'inference' only in the plan that writes nothing in between, '0' never
        self.fuse_offn_opt = env('HFTT_X3_FUSE_OFFN', 'all')
        self.dropout = float(dropout)
        # The device generator decides per element with ONE byte of a hash word (csrc/hftt_common.h: hftt_keep_thr), so the keep probability is
        # quantised to 1/256: `-dropout 0.1` of m_training.py is applied as 26/256 = 0.1016 (kept elements are scaled by 256/230, the reciprocal of
        # the probability actually applied: E[dropout(x)] = x).  Not silent: the applied rate is an attribute and a one-time notice.
        self.dropout_applied = (1.0 - 1.0 / keep_scale(self.dropout)) if self.dropout > 0.0 else 0.0
        if self.dropout > 0.0 and abs(self.dropout_applied - self.dropout) > 1e-6 and not HfttEngine._dropout_notice_given:
            HfttEngine._dropout_notice_given = True
            import warnings
            warnings.warn('hftt_hip: dropout p = %g is applied as %d/256 = %.4f (8-bit keep decisions of the device generator; kept elements are '
                          'scaled by the reciprocal of the applied keep probability, so the expectation is unchanged)'
                          % (self.dropout, round(self.dropout_applied * 256), self.dropout_applied), stacklevel=2)
        self.base_seed = int(seed)
        self.step_counter = 0
        self.generation = 0
        self._bound = None                          # list of (name, param, offset, numel)
        self._ws = {}
        self._site = 0                              # dropout sites of the workspace built last
        self.profiler = None                        # optional per-launch HIP-event timer (bench.py)
        self.frozen_weights = False                 # the caller's promise that the parameters do not change (see prepare_weights)
        self._prepared_frozen = False
        self.set_precision(precision)

    # ------------------------------------------------------------------ precision / parameters
    def set_precision(self, precision):
        if precision not in PRECISION_NPASS:
            raise ValueError('precision must be one of %s' % list(PRECISION_NPASS))
        self.precision = precision
        self._ws = {}
        self.modes = m = precision_modes(self.d, self.p, PRECISION_NPASS[precision], self.opts, fp32_hidden=os.environ.get('HFTT_X3_FP32_HIDDEN', '0') == '1')
        self.npass, self.x3, self.sb, self.strip, self.strip_small, self.bfs, self.hh = m.npass, m.x3, m.sb, m.strip, m.strip_small, m.bfs, m.hh
        # Option (HFTT_X3_GRAD_HI=1): the GRADIENT operand of every GEMM-shaped backward product (dY of dW = dY^T X, the strip of a dX kernel,
        # A of the block dX GEMMs) enters as its bf16 rounding only -- two MFMA passes against the saved operand's / the weights' bf16 pair
        # instead of three: +3.5 % (260 against 251 clips/s on one box), every gradient tensor's cosine against the exact-fp32 mode still
        # >= 0.9999 at paper size, but the gradients move from 2e-4 to 3e-3 .. 6e-3 of the fp32 reference's (relative to the tensor's maximum) --
        # outside the 1e-3 the default mode keeps for gradients too, hence opt-in.
        self.g8 = self.x3 and os.environ.get('HFTT_X3_GRAD_HI', '0') == '1' and not self.strip_small
        if self.g8 and not (lib().hftt_build_options() & 1):
            raise _capi.HfttError('HFTT_X3_GRAD_HI=1 needs a library built with HFTT_BUILD_GRAD_HI=1 (python nylon-amt_amd/build.py writes '
                                  'libhftt_hip_g.so; hftt_hip/_capi.py loads it under the same switch): the default library does not carry the '
                                  'gradient-rounding kernels')
        self._prepared_frozen = False
        self.merge_ckv = self.merge_ckv_bwd = False  # (decided with the layout: _build_prep)
        if self._bound is not None:
            self._build_prep()

    def bind(self, named_params):
        """Flatten the module's parameters into one buffer (reference state_dict order) and rebind .data as views."""
        named = list(named_params)
        offs, total = flat_offsets((n, p.numel()) for n, p in named)
        flat = torch.zeros(total, dtype=torch.float32, device=self.device)
        for (n, p), o in zip(named, offs):
            flat[o:o + p.numel()].copy_(p.data.reshape(-1).to(self.device, torch.float32))
            p.data = flat[o:o + p.numel()].view(p.shape)
        self.flat_params = flat
        self.flat_grads = torch.zeros_like(flat)
        self.poff = {n: o for (n, _), o in zip(named, offs)}
        self.pshape = {n: tuple(p.shape) for n, p in named}
        self._bound = [(n, p, o, p.numel()) for (n, p), o in zip(named, offs)]
        from .trainer import register_binding     # lets FusedAdam(model.parameters()) built before this bind find the engine
        register_binding(self, [p for _, p in named])
        self._build_prep()
        self._ws = {}

    def is_bound(self):
        if self._bound is None:
            return False
        base = self.flat_params.data_ptr()
        for _, p, o, _ in self._bound:
            if p.data_ptr() != base + 4 * o:
                return False
        return True

    def grad_views(self, source=None):
        src = self.flat_grads if source is None else source
        return [src[o:o + n].view(self.pshape[name]) for name, _, o, n in self._bound]

    def P(self, name):   # device address of a parameter
        return self.flat_params.data_ptr() + 4 * self.poff[name]

    def G(self, name):   # device address of a parameter's gradient
        return self.flat_grads.data_ptr() + 4 * self.poff[name]

    # ------------------------------------------------------------------ prepared weights
    def _build_prep(self):
        """device side of the weight layout: the planes, the strip-pack stream, the uploaded tables, the embed-fold descriptor"""
        lay = self.layout = WeightLayout(self.dims, self.modes, self.opts, self.poff, self.pshape,
                                         merge_ckv_bwd_opt=os.environ.get('HFTT_X3_MERGE_CKV_BWD', '1') != '0')
        self.merge_ckv, self.merge_ckv_bwd = lay.merge_ckv, lay.merge_ckv_bwd
        self.Woff = W = lay.Woff
        dev = self.device
        # prepared matrices: bf16 plane (npass 1) or fp32 copy (npass 3, parity) -- same element offsets
        self.wbf = torch.zeros(lay.n_w if self.npass == 1 else 8, dtype=torch.int16, device=dev)
        self.wf32 = torch.zeros(lay.n_w if self.npass == 3 else 8, dtype=torch.float32, device=dev)
        # x3: every prepared matrix as two 16-bit planes (hi, lo) at the same element offsets -- fp16 halves for the forward matrices,
        # bf16 halves for the transposed ones (they only meet gradients)
        self.whi = torch.zeros(lay.n_w if self.npass == 2 else 8, dtype=torch.int16, device=dev)
        self.wlo = torch.zeros(lay.n_w if self.npass == 2 else 8, dtype=torch.int16, device=dev)
        self.fprep = torch.zeros(lay.n_f, dtype=torch.float32, device=dev)
        self._wp_used, self._prep_built_for = set(), -1
        self._set_prep_table(lay.prep)
        self.n_spack, self.n_spack_t = len(lay.spack), len(lay.spack_t)
        if lay.spack:
            self.wstrip = torch.zeros(lay.n_s, dtype=torch.int16, device=dev)
            self.spack_table = _table(StripPackEntry, lay.spack).to(dev)
        if lay.spack_t:
            self.spack_table_t = _table(StripPackEntry, lay.spack_t).to(dev)
        # embed-fold scratch (dWeff, dbeff)
        self.dweff = torch.zeros(self.d * self.Kp, dtype=torch.float32, device=dev)
        self.dbeff = torch.zeros(self.d, dtype=torch.float32, device=dev)
        e = 'encoder_spec2midi.'
        self.fold = FoldDesc(self.d, self.cfg['cnn_channel'], self.cfg['cnn_kernel'], self.n_proc, self.Kp, _align(self.d, 64),
                             self.P(e + 'conv.weight'), self.P(e + 'conv.bias'), self.P(e + 'tok_embedding_freq.weight'),
                             self.P(e + 'tok_embedding_freq.bias'),
                             (self.wbf.data_ptr() + 2 * W['embed']) if self.npass == 1 else 0,
                             (self.wf32.data_ptr() + 4 * W['embed']) if self.npass == 3 else 0,
                             self.fprep.data_ptr() + 4 * W['embed_b'],
                             self.dweff.data_ptr(), self.dbeff.data_ptr(),
                             self.G(e + 'conv.weight'), self.G(e + 'conv.bias'), self.G(e + 'tok_embedding_freq.weight'),
                             self.G(e + 'tok_embedding_freq.bias'),
                             (self.whi.data_ptr() + 2 * W['embed']) if self.npass == 2 else 0,
                             (self.wlo.data_ptr() + 2 * W['embed']) if self.npass == 2 else 0)

    def _set_prep_table(self, entries):
        # (last field, pad: x3 element type -- transposed = backward = bf16 halves)
        self.prep_table = _table(PrepEntry, [e + (4 if e[6] == 1 else 2,) for e in entries]).to(self.device)
        self.n_prep = len(entries)

    def _refresh_prep_table(self):
        """strip plans: prepare only the per-block planes a launch plan has asked for (layout.BLOCK_PLANES)"""
        if not self.strip or self._prep_built_for == len(self._wp_used):
            return
        self._set_prep_table(self.layout.prep_for(self._wp_used))
        self._prep_built_for = len(self._wp_used)

    def Wp(self, key):   # device address of a prepared matrix (bf16 plane or fp32 copy, by precision)
        o = self.Woff[key]
        self._wp_used.add(key)
        if self.npass == 2:
            return self.whi.data_ptr() + 2 * o
        return (self.wbf.data_ptr() + 2 * o) if self.npass == 1 else (self.wf32.data_ptr() + 4 * o)

    def Wp_lo(self, W):   # x3: the lo plane of the prepared matrix whose hi plane sits at device address W
        return (W - self.whi.data_ptr() + self.wlo.data_ptr()) if self.npass == 2 else 0

    def Fp(self, key):
        return self.fprep.data_ptr() + 4 * self.Woff[key]

    def Ws(self, key):   # device address of a strip-packed weight stream
        return self.wstrip.data_ptr() + 2 * self.Woff['s.' + key]

    def prepare_weights(self, stream):
        """parameters -> the kernels' operand forms (bf16 / fp32 planes, folded embedding, strip packs): every forward, because the flat buffer
        may have changed in ways nobody tells the engine about (an optimizer step, ``p.data.copy_``) -- unless the caller has declared the
        parameters constant (``frozen_weights``: inference servers; model.amt.AMT does), then once."""
        if self.frozen_weights and self._prepared_frozen:
            return
        self._refresh_prep_table()
        if self.npass == 2:
            check(self.lib.hftt_prep_weights_x3(self.flat_params.data_ptr(), self.whi.data_ptr(), self.wlo.data_ptr(),
                                                self.fprep.data_ptr(), self.prep_table.data_ptr(), self.n_prep, stream), 'prep_weights_x3')
        else:
            check(self.lib.hftt_prep_weights(self.flat_params.data_ptr(), self.wbf.data_ptr() if self.npass == 1 else 0,
                                             self.wf32.data_ptr() if self.npass == 3 else 0,
                                             self.fprep.data_ptr(), self.prep_table.data_ptr(), self.n_prep, stream), 'prep_weights')
        check(self.lib.hftt_embed_fold_fwd(C.byref(self.fold), stream), 'embed_fold_fwd')
        if self.strip and self.n_spack:
            if self.x3:
                check(self.lib.hftt_x3_strip_pack(self.flat_params.data_ptr(), self.wstrip.data_ptr(), self.spack_table.data_ptr(), self.n_spack, 2, stream), 'x3_strip_pack')
                check(self.lib.hftt_x3_strip_pack(self.flat_params.data_ptr(), self.wstrip.data_ptr(), self.spack_table_t.data_ptr(), self.n_spack_t, 4, stream), 'x3_strip_pack')
            elif self.strip_small:                   # bf16 mode, small widths: compact packs with bf16 halves for both directions
                check(self.lib.hftt_x3_strip_pack(self.flat_params.data_ptr(), self.wstrip.data_ptr(), self.spack_table.data_ptr(), self.n_spack, 4, stream), 'x3_strip_pack')
                if self.n_spack_t:
                    check(self.lib.hftt_x3_strip_pack(self.flat_params.data_ptr(), self.wstrip.data_ptr(), self.spack_table_t.data_ptr(), self.n_spack_t, 4, stream), 'x3_strip_pack')
            else:
                check(self.lib.hftt_strip_pack(self.flat_params.data_ptr(), self.wstrip.data_ptr(), self.spack_table.data_ptr(), self.n_spack, stream), 'strip_pack')
        self._prepared_frozen = self.frozen_weights

    # ------------------------------------------------------------------ workspace + plans for one batch size
    def workspace(self, B):
        if B in self._ws:
            return self._ws[B]
        if not self.is_bound():
            raise _capi.HfttError('engine parameters are not bound')
        builder = PlanBuilder(self, B)
        ws = self._ws[B] = builder.build()
        self._site = builder.site
        return ws

    # ------------------------------------------------------------------ running plans
    def _run(self, ws, plan, stream, outs=None, seed=0, p=0.0):
        L = self.lib
        B, T, N, V, d = ws['B'], self.T, self.N, self.V, self.d
        prof = self.profiler
        for fn, args, name, meta in plan:
            if prof is not None:
                prof.begin(name, meta)
            if not isinstance(fn, str):
                rc = fn(*args, stream)
            elif fn == 'im2win':
                rc = L.hftt_im2win(ws['spec_ptr'], *args, stream)
            elif fn == 'ln_reduce':
                n_wg, n, dg, db, beta = args
                rc = L.hftt_ln_bwd_reduce(ws['ln_ws_ptr'], n_wg, n, dg, db, beta, stream)
            elif fn == 'heads':
                logits, tm = args
                o = outs[5:9] if tm else outs[0:4]
                rc = L.hftt_heads_split(logits, self.NHp, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), B, T, N, V, tm, stream)
            elif fn == 'heads_bwd':
                side, dlog, tm = args
                b = ws['bufs']
                po = outs[5:8] if tm else outs[0:3]
                rc = L.hftt_heads_split_bwd(po[0].data_ptr(), po[1].data_ptr(), po[2].data_ptr(),
                                            b['d.onset_' + side].data_ptr(), b['d.offset_' + side].data_ptr(), b['d.mpe_' + side].data_ptr(),
                                            b['d.velocity_' + side].data_ptr(), dlog, self.NHp, B, T, N, V, tm, stream)
            elif fn == 'time_embed':
                x, pos, y, site, iof = args
                rc = L.hftt_time_embed_fwd(x, pos, y, B, T, N, d, math.sqrt(d), p, site, seed, iof, stream)
            elif fn == 'time_embed_bwd':
                dy, dx, dym, site, iof = args
                rc = L.hftt_time_embed_bwd(dy, dx, dym, B, T, N, d, math.sqrt(d), p, site, seed, 1, iof, stream)
            elif fn == 'colsum':
                x, rows, n, ld, out, beta, wsp, xbf = args
                rc = L.hftt_colsum(x, rows, n, ld, out, beta, wsp, xbf, stream)
            elif fn == 'dropout_bwd':
                g, n, site, gbf = args
                rc = L.hftt_dropout_bwd(g, n, p, site, seed, gbf, stream) if p > 0.0 else 0
            elif fn == 'dropout_bwd_colsum':
                g, rows, n, ld, site, out, beta, wsp, gbf = args
                rc = L.hftt_dropout_bwd_colsum(g, rows, n, ld, p, site, seed, out, beta, wsp, gbf, stream)
            else:
                raise _capi.HfttError('unknown plan op %s' % fn)
            if prof is not None:
                prof.end()
            if rc != 0:
                check(rc, name)

    def _patch(self, ws, p, seed):
        inv_keep = keep_scale(p)
        for dsc in ws['drop']:
            dsc.drop_p = p
            dsc.drop_seed = seed
        for dsc in ws.get('gate_descs', ()):
            dsc.gate_scale = inv_keep

    def forward(self, spec, training=False, outputs=None, save=None):
        """spec [B, n_bin, M+T+M] (any device/dtype/strides) -> 9-tuple of fresh fp32 tensors on the engine's device."""
        if spec.dim() != 3 or spec.shape[1] != self.F or spec.shape[2] != self.W:
            raise _capi.HfttError('input_spec must be [B, %d, %d], got %s' % (self.F, self.W, tuple(spec.shape)))
        if not self.is_bound():
            raise _capi.HfttError('engine parameters are not bound (call bind first)')
        B = spec.shape[0]
        with torch.cuda.device(self.device):         # launches, stream lookup and device queries all refer to the engine's GPU
            return self._forward(spec, B, training, outputs, save)

    def _forward(self, spec, B, training, outputs, save):
        ws = self.workspace(B)
        self._cur_ws = ws
        # the window gather reads the caller's tensor in place when it already is what the kernel wants (fp32, contiguous, on this device);
        # anything else is converted into the workspace copy.  (torch's device-to-device copy_ is ~24 blit launches of 64 KB here: 80 us.)
        if spec.is_cuda and spec.device == self.device and spec.dtype == torch.float32 and spec.is_contiguous():
            ws['spec_ptr'], ws['spec_ref'] = spec.data_ptr(), spec
        else:
            ws['bufs']['spec'].copy_(spec)
            ws['spec_ptr'], ws['spec_ref'] = ws['bufs']['spec'].data_ptr(), None
        T, N, V = self.T, self.N, self.V
        dev = self.device
        outs = outputs
        if outs is None:
            outs = [torch.empty(B, T, N, device=dev) for _ in range(3)] + [torch.empty(B, T, N, V, device=dev)] \
                + [torch.empty(B, T, self.Hd, N, self.F, device=dev)] \
                + [torch.empty(B, T, N, device=dev) for _ in range(3)] + [torch.empty(B, T, N, V, device=dev)]
        for ad in ws['attn_out_descs']:
            ad.probs = outs[4].data_ptr()
        p = self.dropout if training else 0.0
        if training:
            self.step_counter += 1
        seed = (self.base_seed * 1000003 + self.step_counter) & 0xFFFFFFFFFFFFFFFF
        ws['seed'], ws['p'], ws['outs'] = seed, p, outs
        self._patch(ws, p, seed)
        stream = torch.cuda.current_stream(dev).cuda_stream
        self.prepare_weights(stream)
        if save is None:
            save = training
        plan = ws['fwd'] if (save or 'fwd_inf' not in ws) else ws['fwd_inf']      # inference plan: nothing is saved for a backward
        ws['saved'] = plan is ws['fwd']
        self._run(ws, plan, stream, outs=outs, seed=seed, p=p)
        self.generation += 1
        ws['generation'] = self.generation
        return tuple(outs)

    def frozen_border(self, frozen_stages):
        """flat offset below which backward(frozen_stages=...) writes nothing: 0, the frequency decoder's first parameter, the time decoder's"""
        dd = 'decoder_spec2midi.'
        return (0, self.poff[dd + 'pos_embedding_freq.weight'], self.poff[dd + 'pos_embedding_time.weight'])[frozen_stages]

    def backward_plan(self, B, frozen_stages=0):
        """(launch list, marks) of the backward with the first `frozen_stages` stages of the flat layout frozen.  0: the workspace's full plan
        (the same object as ever).  2: its prefix up to the first mark (time decoder + heads B).  1: a second plan, built on first use by the
        same builder code: the full plan up to the second mark without the launches that form the encoder-output gradient."""
        ws = self.workspace(B)
        if frozen_stages == 0:
            return ws['bwd'], ws['bwd_marks']
        if frozen_stages == 2:
            marks = ws['bwd_marks'][:1]
            return ws['bwd'][:marks[0][0]], marks
        if frozen_stages != 1:
            raise _capi.HfttError('frozen_stages=%r must be 0, 1 (encoder) or 2 (encoder + frequency decoder)' % (frozen_stages,))
        if 'bwd_dec' not in ws:
            with torch.cuda.device(self.device):
                PlanBuilder(self, B, ws).build_decoder_backward()
        return ws['bwd_dec'], ws['bwd_dec_marks']

    def backward(self, B, generation=None, on_ready=None, frozen_stages=0):
        """Backward through the most recent forward of batch size B; the gradients of the 8 outputs must be in
        the 'd.*' workspace buffers.  Fills flat_grads (every parameter written exactly once).
        on_ready(lo, hi), if given, is called three times, each as soon as every launch that writes flat_grads[lo:hi] has
        been enqueued (time decoder, frequency decoder, encoder): the data-parallel all-reduce of that range can then
        overlap the rest of the backward (hftt_hip/ddp.py).
        frozen_stages = 1 (encoder) / 2 (encoder + frequency decoder): the backward stops where nothing trainable remains (backward_plan).
        flat_grads below frozen_border(frozen_stages) is not written -- it keeps what it held -- and on_ready is called for the ranges that were
        produced only.  The forward plan is the same either way."""
        ws = self._ws.get(B)
        if ws is None or 'outs' not in ws:
            raise _capi.HfttError('backward called without a forward')
        if not ws.get('saved', True):
            raise _capi.HfttError('backward after an inference-plan forward (model.eval()): nothing was saved; run the forward in training mode')
        if generation is not None and generation != ws['generation']:
            raise _capi.HfttError('backward called for a stale forward (activations were overwritten by a later forward)')
        self._cur_ws = ws
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            plan, marks = self.backward_plan(B, frozen_stages)     # (in front of the patch: a plan built just now brings new descriptors)
            self._patch(ws, ws['p'], ws['seed'])
            if on_ready is None:
                self._run(ws, plan, stream, outs=ws['outs'], seed=ws['seed'], p=ws['p'])
                return
            start = 0
            for end, lo, hi in marks:
                self._run(ws, plan[start:end], stream, outs=ws['outs'], seed=ws['seed'], p=ws['p'])
                on_ready(lo, hi)
                start = end

    # ------------------------------------------------------------------ fused loss (training/train.py:141-153)
    def loss(self, B, labels, weight_A=1.0, weight_B=1.0, with_grad=True, spec=None):
        """labels: (onset, offset, mpe, velocity) device tensors [B,T,N] (fp32, fp32, fp32, int64).
        Returns a [9] device tensor (total + 8 terms); with_grad fills the 'd.*' buffers.
        spec: None launches hftt_loss (the reference's criteria); a hftt_hip.criteria.LossSpec launches hftt_loss_w with its options
        (the two velocity divisors W_A, W_B then follow the nine values in the same buffer, 'loss_out'[9:11])."""
        ws = self._ws[B]
        outs = ws['outs']
        b = ws['bufs']
        n = B * self.T * self.N
        if 'loss_ws' not in b:
            b['loss_ws'] = torch.empty(self.lib.hftt_loss_ws_bytes(n) // 4 + 16, dtype=torch.float32, device=self.device)
            b['loss_out'] = torch.zeros(16, dtype=torch.float32, device=self.device)
        lo, lf, lm, lv = labels
        for t, dt in ((lo, torch.float32), (lf, torch.float32), (lm, torch.float32), (lv, torch.int64)):
            if t.dtype != dt or not t.is_contiguous() or t.device != self.device or t.numel() != n:
                raise _capi.HfttError('labels must be contiguous device tensors [B,T,N] (fp32,fp32,fp32,int64)')
        if spec is not None and (spec.Nn != self.N or spec.V != self.V):
            raise _capi.HfttError('loss spec built for Nn=%d, V=%d; the model has Nn=%d, V=%d' % (spec.Nn, spec.V, self.N, self.V))
        wdsc = LossWDesc() if spec is not None else None
        dsc = LossDesc() if spec is None else wdsc.base
        dsc.n, dsc.V = n, self.V
        for i, k in enumerate((0, 1, 2, 5, 6, 7)):
            dsc.prob[i] = outs[k].data_ptr()
        dsc.vel[0], dsc.vel[1] = outs[3].data_ptr(), outs[8].data_ptr()
        dsc.label_onset, dsc.label_offset, dsc.label_mpe, dsc.label_velocity = lo.data_ptr(), lf.data_ptr(), lm.data_ptr(), lv.data_ptr()
        dsc.weight_A, dsc.weight_B, dsc.grad_scale = weight_A, weight_B, 1.0
        if with_grad:
            for i, nm in enumerate(('onset_A', 'offset_A', 'mpe_A', 'onset_B', 'offset_B', 'mpe_B')):
                dsc.d_prob[i] = b['d.' + nm].data_ptr()
            dsc.d_vel[0], dsc.d_vel[1] = b['d.velocity_A'].data_ptr(), b['d.velocity_B'].data_ptr()
        dsc.loss_out, dsc.ws = b['loss_out'].data_ptr(), b['loss_ws'].data_ptr()
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            if spec is None:
                check(self.lib.hftt_loss(C.byref(dsc), stream), 'loss')
            else:
                if 'loss_w_ws' not in b:
                    b['loss_w_ws'] = torch.empty(self.lib.hftt_loss_w_ws_bytes(n) // 4, dtype=torch.float32, device=self.device)
                spec.fill(wdsc, b['loss_w_ws'])
                check(self.lib.hftt_loss_w(C.byref(wdsc), stream), 'loss_w')
        return b['loss_out'][:9]
