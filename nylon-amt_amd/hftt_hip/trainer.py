"""Fast training step over the HIP engine (no per-parameter autograd): forward plan -> fused loss kernel ->
backward plan -> fused Adam on the flat parameter buffer.  Mirrors the body of the reference's hot loop
(training/train.py:89-160: zero_grad, forward, 8 criteria, weighted sum, backward, optimizer.step) and
m_training.py:146-147 (Adam defaults, ReduceLROnPlateau on top).  Gradients are exposed as ``p.grad`` views into the flat
gradient buffer.
"""
from __future__ import annotations

import contextlib
import math
import weakref

import numpy as np
import torch

from . import ops
from ._capi import ADAM_MAX_GROUPS, HfttError
from .layout import flat_offsets

# the two parameters at which the flat layout changes stage (encoder | frequency decoder + heads A | time decoder + heads B): the offsets
# PlanBuilder.build_backward uses for its marks
STAGE_BORDERS = ('decoder_spec2midi.pos_embedding_freq.weight', 'decoder_spec2midi.pos_embedding_time.weight')
STAGES = ('encoder', 'freq', 'time')

# parameter -> engine whose flat buffer it is a view of (filled by HfttEngine.bind): lets FusedAdam(model.parameters()) find the engine
# although m_training.py:146 builds the optimizer before the first forward has bound anything
# (keyed by id: tensors compare element-wise, so they cannot be keys of a WeakKeyDictionary; the weak reference to the parameter
# guards against a recycled id)
_ENGINE_OF = {}


def register_binding(engine, params):
    eref = weakref.ref(engine)
    for p in params:
        key = id(p)
        _ENGINE_OF[key] = (weakref.ref(p, lambda _r, key=key: _ENGINE_OF.pop(key, None)), eref)


def engine_of(p):
    ent = _ENGINE_OF.get(id(p))
    if ent is None or ent[0]() is not p:
        return None
    return ent[1]()


def stage_groups(model, encoder=None, freq=None, time=None, no_decay_1d=False):
    """Parameter groups for ``FusedAdam`` split by the three stages of the flat layout: the encoder, the frequency decoder with heads A, the
    time decoder with heads B (borders: ``STAGE_BORDERS``, in ``model.named_parameters()`` order, which is the flat order).  Each stage
    argument is a dict of group options, e.g. ``encoder=dict(frozen=True)``, ``time=dict(lr=1e-3)``; what it leaves out comes from the
    optimizer's defaults.  ``no_decay_1d=True`` splits every stage once more: biases and LayerNorm parameters (every tensor with at most one
    dimension) go into a twin group with ``weight_decay=0`` -- at most 6 groups.  Every group carries its name as ``'stage'``."""
    named = list(model.named_parameters())
    names = [n for n, _ in named]
    if any(b not in names for b in STAGE_BORDERS):
        raise HfttError('stage_groups: the model has no %s / %s (not an hFT-Transformer?)' % STAGE_BORDERS)
    cut = [names.index(b) for b in STAGE_BORDERS]
    groups = []
    for stage, opts, lo, hi in zip(STAGES, (encoder, freq, time), [0] + cut, cut + [len(named)]):
        opts = dict(opts or {})
        ps = [p for _, p in named[lo:hi]]
        if not no_decay_1d:
            groups.append(dict(opts, params=ps, stage=stage))
            continue
        groups.append(dict(opts, params=[p for p in ps if p.dim() > 1], stage=stage))
        groups.append(dict(opts, params=[p for p in ps if p.dim() <= 1], stage=stage + '.no_decay', weight_decay=0.0))
    return [g for g in groups if g['params']]


class FusedAdam(torch.optim.Optimizer):
    """torch.optim.Adam(params, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0) as ONE kernel over the engine's flat buffers.

    Drop-in at m_training.py:146: ``optimizer = FusedAdam(model.parameters(), lr=args.lr)`` (a model is accepted too).  It is a real
    ``torch.optim.Optimizer``: ``ReduceLROnPlateau(optimizer)`` (:147) and ``scheduler.step`` (:437) drive ``param_groups[0]['lr']``,
    ``state_dict()`` / ``load_state_dict()`` (:374-392, :268-299) have torch Adam's layout (per-parameter ``step`` / ``exp_avg`` /
    ``exp_avg_sq``, here views into two flat moment buffers), so a reference ``.dat`` checkpoint's ``optimizer_dict`` loads.

    The guarded step (opt-in; with the three options at their defaults ``step()`` launches exactly the one Adam kernel above):

    ``max_grad_norm``  global-norm clipping, ``torch.nn.utils.clip_grad_norm_(model.parameters(), max_grad_norm)`` in front of the step: the
                     L2 norm of the whole flat gradient (fp64 accumulation on the device, ``grad_scale`` folded in), factor
                     ``min(1, max_grad_norm / (norm + 1e-6))``.  Unlike ``clip_grad_norm_``, which scales the gradients in place, the factor
                     is applied INSIDE the Adam kernel: ``p.grad`` keeps the UNCLIPPED gradient.
    ``guard``          a step whose gradient norm is not finite (some element is Inf / NaN) is skipped: parameters and both moments keep
                     their bits.  Any of the three options turns the guard on.  ``state[p]['step']`` counts calls, so a skipped step still
                     advances it (``GradScaler`` does not count skipped steps; here the bias correction is slightly smaller for the first few
                     hundred steps after a skip, and checkpoints keep their layout).
    ``weight_decay``   decoupled (``torch.optim.AdamW``: ``p *= 1 - lr * weight_decay`` before the update; the group then says
                     ``decoupled_weight_decay=True``).  It is a per-group option: ``stage_groups(model, no_decay_1d=True)`` keeps biases and
                     LayerNorm parameters in zero-decay groups, as AdamW recipes do.  The L2 form (decay added to the gradient) is not
                     implemented and a state that asks for it is refused.

    Parameter groups (fine-tuning): ``FusedAdam([{'params': ..., 'lr': ..., 'weight_decay': ..., 'frozen': True}, ...], lr=...)``, torch's
    ordinary form, 1 to 8 groups which together hold exactly the bound model's parameters, each once (``stage_groups`` builds the usual
    split).  ``lr``, ``weight_decay`` and ``frozen`` are per group; ``betas``, ``eps``, ``max_grad_norm`` and ``guard`` are shared and groups
    that disagree on them are refused.  A frozen group's parameters and moments keep every bit: the kernel neither loads nor stores them.  A
    parameter with ``requires_grad == False`` is frozen whatever its group says.  The step stays one launch (norm + step when guarded): a
    per-quad group map in device memory says which constants a quad takes.  The map is rebuilt when a ``frozen`` option or a
    ``requires_grad`` flag changes (a host-side signature is compared per step); learning rates travel in the launch descriptor, so a
    scheduler's write to ``param_groups[i]['lr']`` costs nothing.  The guarded norm leaves frozen ranges out (``clip_grad_norm_`` over the
    parameters that have a gradient), so an Inf in a frozen range does not skip the step.  ``frozen_stages()`` says how much of the flat
    layout's front is frozen; ``TrainStep`` hands it to the engine, whose backward then stops where nothing trainable remains.  One group
    with nothing frozen launches exactly the kernels described above.  ``state_dict()`` keeps torch's layout with several ``param_groups``
    (``frozen`` is a group option like any other); a state whose group structure differs from the optimizer's is refused by torch
    (``ValueError``), as for any torch optimizer.

    The decision is taken on the device: ``grad_norm`` and ``clip_coef`` are 0-dim device views of the kernel's record (reading them does
    not synchronise); ``skipped_steps`` and ``clipped_steps`` are Python ints, and reading them DOES synchronise.  ``state_dict()`` carries
    the two counters as ``hftt_guard``; a state without that key (older checkpoints, the reference's ``.dat``) loads.

    Averaged weights (opt-in; ``ema_decay=None`` allocates nothing and launches exactly the kernels described above):

    ``ema_decay``      the exponential moving average of the parameters, ``torch.optim.swa_utils.get_ema_multi_avg_fn(ema_decay)`` after every
                     step, carried INSIDE the Adam launch (``hftt_adam_step_ema``: all three configurations -- plain, guarded, grouped -- go
                     through it, the guarded norm in front as before) as a compensated fp32 sum, because the plain fp32 ``lerp_`` stops moving
                     when the weights only jitter round a mean.  Parameters and moments keep the bits of the step without the average; a
                     skipped step and frozen ranges leave the average alone.  Shared by all groups like ``betas``.  The average starts as a
                     copy of the parameters at ``attach`` (right for fine-tuning from trained weights).
    ``ema_warmup``     from scratch: the decay of call ``t`` (0-based; calls count as for ``step``, skipped ones included) is
                     ``min(ema_decay, (1 + t) / (10 + t))``, so the random initialisation is forgotten quickly.  The decay travels in the
                     launch descriptor: a schedule costs nothing.

    ``state[p]['ema']`` and ``state[p]['ema_c']`` (the running compensation) are views into two flat buffers, like the moments, and travel
    through ``state_dict()`` with them; ``hftt_ema = {'decay', 'warmup', 'updates'}`` rides along.  A state without them loaded into an
    optimizer with the option restarts the average from the parameters; a state with them turns the option on.
    ``with opt.averaged_weights():`` puts the average into the model for evaluation (contents are swapped, so every launch plan keeps its
    addresses) and restores every bit on exit; ``step()`` inside is refused and the context does not nest.  ``opt.averaged_model()`` is a
    CPU copy of the model that holds the average, for pickling.  Under DDP every rank applies the same update to the same bits, so the
    averages agree without communication."""

    def __init__(self, params, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None, guard=False, weight_decay=0.0, model=None,
                 ema_decay=None, ema_warmup=False):
        """model: the module whose parameters the groups hold -- needed only where the group map is wanted before an engine has bound them
        (``frozen_stages()`` on a host without a GPU); with a bound engine the layout is the engine's."""
        if hasattr(params, 'hftt_engine'):
            model = params
            params = model.parameters()
        params = list(params)
        if params and isinstance(params[0], dict):
            if not 1 <= len(params) <= ADAM_MAX_GROUPS:
                raise HfttError('FusedAdam takes 1 to %d parameter groups, got %d' % (ADAM_MAX_GROUPS, len(params)))
            params = [dict(g, params=list(g['params'])) for g in params]
            seen = set()
            for g in params:
                for p in g['params']:
                    if id(p) in seen:
                        raise HfttError('FusedAdam: a parameter appears in more than one group (or twice in one)')
                    seen.add(id(p))
                if not float(g.get('weight_decay', weight_decay)) >= 0.0:
                    raise HfttError('FusedAdam: weight_decay=%r must be >= 0' % (g.get('weight_decay', weight_decay),))
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise HfttError('FusedAdam: max_grad_norm=%r must be positive (None: no clipping)' % (max_grad_norm,))
        if not float(weight_decay) >= 0.0:
            raise HfttError('FusedAdam: weight_decay=%r must be >= 0' % (weight_decay,))
        for d in [ema_decay] + [g.get('ema_decay') for g in params if isinstance(g, dict)]:
            self._check_ema_decay(d)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None, capturable=False,
                                      differentiable=False, fused=None, decoupled_weight_decay=weight_decay != 0,
                                      max_grad_norm=None if max_grad_norm is None else float(max_grad_norm), guard=bool(guard), frozen=False,
                                      ema_decay=None if ema_decay is None else float(ema_decay), ema_warmup=bool(ema_warmup)))
        for g in self.param_groups:
            g['decoupled_weight_decay'] = g['weight_decay'] != 0
        self._check_shared()
        self._model = model
        self._map = None                          # the group map and what it was built from (_group_map)
        self.engine = None
        self.step_count = 0
        self.exp_avg = self.exp_avg_sq = None
        self._ctl = self._ws = None               # the guarded step's device record and workspace (attach)
        self._pending_guard = None                # counters of a checkpoint loaded before any engine existed
        self.ema = self.ema_c = None              # the averaged weights and their running compensation (attach, with ema_decay)
        self.ema_updates = 0                      # calls the average has seen (the t of ema_warmup)
        self._averaged = False                    # inside averaged_weights()

    # ---- binding to the engine's flat buffers (lazy: the engine binds at the model's first forward)
    def _params(self):
        if len(self.param_groups) == 1:
            return self.param_groups[0]['params']
        return [p for g in self.param_groups for p in g['params']]

    def _check_shared(self):
        g0 = self.param_groups[0]
        for g in self.param_groups[1:]:
            for k in ('betas', 'eps', 'max_grad_norm', 'guard', 'ema_decay', 'ema_warmup'):
                a, b = g0.get(k), g.get(k)
                if (tuple(a) != tuple(b)) if k == 'betas' else (a != b):
                    raise HfttError('FusedAdam: parameter groups disagree on %s (%r against %r): it is shared by all groups' % (k, a, b))

    # ---- parameter groups: the per-quad map of the grouped kernels
    def _layout(self):
        """[(name, parameter, flat offset, numel)] and the flat length: the bound engine's, or the model's by the same rule"""
        if self.engine is not None:
            return self.engine._bound, self.engine.flat_params.numel()
        if self._model is None:
            raise HfttError('FusedAdam: the group map needs the flat layout: bind the parameters to an engine (a forward on the GPU) or pass model=')
        named = list(self._model.named_parameters())
        offs, total = flat_offsets((n, p.numel()) for n, p in named)
        return [(n, p, o, p.numel()) for (n, p), o in zip(named, offs)], total

    def _signature(self, layout):
        return (id(self.engine), tuple(bool(g.get('frozen', False)) for g in self.param_groups), tuple(p.requires_grad for _, p, _, _ in layout))

    def _group_map(self):
        """The map state, rebuilt when a group's ``frozen`` or a parameter's ``requires_grad`` changed: dict(trivial, qmap (device uint8 or None
        without an engine), frozen (one flag per kernel group), mask, stages).  trivial: one group, nothing frozen -- today's kernels run."""
        layout, total = self._layout()
        sig = self._signature(layout)
        if self._map is not None and self._map['sig'] == sig:
            return self._map
        groups = self.param_groups
        gi_of = {id(p): i for i, g in enumerate(groups) for p in g['params']}
        if len(gi_of) != len(layout) or any(id(p) not in gi_of for _, p, _, _ in layout):
            raise HfttError('FusedAdam: the parameter groups must together hold exactly the parameters of the bound model, each once '
                            '(%d in the groups, %d in the model)' % (len(gi_of), len(layout)))
        frozen = [bool(g.get('frozen', False)) for g in groups]
        no_grad = [not p.requires_grad for _, p, _, _ in layout]
        sink = None
        if any(ng and not frozen[gi_of[id(p)]] for ng, (_, p, _, _) in zip(no_grad, layout)):
            # requires_grad == False inside a trainable group: such a tensor moves to a frozen group -- a frozen quad reads none of its
            # group's constants, so any frozen group serves, and a new one is opened only when there is none
            sink = frozen.index(True) if True in frozen else len(frozen)
            if sink == len(frozen):
                if sink >= ADAM_MAX_GROUPS:
                    raise HfttError('FusedAdam: %d groups and parameters with requires_grad=False inside trainable groups: no group index is '
                                    'left for them (mark one of the groups frozen)' % len(groups))
                frozen.append(True)
        entries = [(o, n, sink if (ng and not frozen[gi_of[id(p)]]) else gi_of[id(p)]) for ng, (_, p, o, n) in zip(no_grad, layout)]
        host = ops.adam_group_map(entries, total)
        fq = np.asarray(frozen, dtype=bool)[host.numpy()]
        off = {name: o for name, _, o, _ in layout}
        borders = [off.get(b) for b in STAGE_BORDERS]
        stages = 0
        if None not in borders:
            if fq[:borders[0] // 4].all():
                stages = 2 if fq[borders[0] // 4:borders[1] // 4].all() else 1
        self._map = dict(sig=sig, trivial=len(groups) == 1 and not any(frozen), frozen=frozen, mask=sum(1 << i for i, f in enumerate(frozen) if f),
                         qmap=None if self.engine is None else host.to(self.engine.flat_params.device), stages=stages,
                         borders=(0,) + tuple(b or 0 for b in borders), frozen_elements=int(fq.sum()) * 4, host=host)
        return self._map

    def frozen_stages(self):
        """How many leading stages of the flat layout (encoder | frequency decoder + heads A | time decoder + heads B) are frozen as a whole:
        0, 1 (the whole encoder range) or 2 (encoder and frequency decoder).  Derived from the group map; no device work."""
        return self._group_map()['stages']

    def attach(self, engine):
        if (self.engine is engine and self.exp_avg is not None and self.exp_avg.numel() == engine.flat_params.numel()
                and (self.ema is not None) == (self.param_groups[0].get('ema_decay') is not None)):
            return
        ps = self._params()
        bound = [p for _, p, _, _ in engine._bound]
        if len(self.param_groups) == 1:
            if len(ps) != len(bound) or any(a is not b for a, b in zip(ps, bound)):
                raise HfttError('FusedAdam must hold exactly model.parameters() of the bound model, in order')
        elif len(ps) != len(bound) or {id(p) for p in ps} != {id(p) for p in bound}:
            raise HfttError('FusedAdam: the parameter groups must together hold exactly the parameters of the bound model, each once '
                            '(%d in the groups, %d in the model)' % (len(ps), len(bound)))
        ps = bound
        old = {p: dict(self.state[p]) for p in ps if p in self.state and 'exp_avg' in self.state[p]}
        self.engine = engine
        self.exp_avg = torch.zeros_like(engine.flat_params)
        self.exp_avg_sq = torch.zeros_like(engine.flat_params)
        for (name, p, o, n) in engine._bound:
            st = self.state[p]
            m, v = self.exp_avg[o:o + n].view(p.shape), self.exp_avg_sq[o:o + n].view(p.shape)
            if p in old:                          # state loaded (load_state_dict) or carried over a re-bind: copy into the flat moments
                m.copy_(old[p]['exp_avg']); v.copy_(old[p]['exp_avg_sq'])
                self.step_count = int(old[p]['step'])
            st['step'] = torch.tensor(float(self.step_count))
            st['exp_avg'], st['exp_avg_sq'] = m, v
        self._attach_ema(engine, old)
        self._ctl, self._ws = ops.guard_buffers(engine.flat_params.numel(), engine.flat_params.device)
        if self._pending_guard is not None:
            self._set_guard_counts(*self._pending_guard)
            self._pending_guard = None
        ctr = getattr(self, '_pending_counter', None)
        if ctr is not None:                       # a checkpoint loaded before any engine existed: resume its dropout stream position
            engine.step_counter = int(ctr)
            self._pending_counter = None

    def _attach_ema(self, engine, old):
        """the flat average and its compensation, with per-parameter views in the state: carried over where the old state has them (every
        parameter's, or none: a partial average restarts), else the average starts from the parameters"""
        for st in self.state.values():
            st.pop('ema', None); st.pop('ema_c', None)
        if self.param_groups[0].get('ema_decay') is None:
            self.ema = self.ema_c = None
            return
        self.ema = engine.flat_params.clone()
        self.ema_c = torch.zeros_like(engine.flat_params)
        carried = all(p in old and 'ema' in old[p] and 'ema_c' in old[p] for _, p, _, _ in engine._bound)
        if not carried:
            self.ema_updates = 0
        for (name, p, o, n) in engine._bound:
            e, c = self.ema[o:o + n].view(p.shape), self.ema_c[o:o + n].view(p.shape)
            if carried:
                e.copy_(old[p]['ema']); c.copy_(old[p]['ema_c'])
            self.state[p]['ema'], self.state[p]['ema_c'] = e, c

    def _find_engine(self):
        if self._model is not None:
            return self._model.hftt_engine()
        eng = engine_of(self._params()[0])
        if eng is None or not eng.is_bound():
            raise HfttError('FusedAdam.step: the parameters are not bound to a HIP engine yet (run a forward of the model on the GPU first)')
        return eng

    @torch.no_grad()
    def step(self, closure=None, grad_scale=1.0):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self._averaged:
            raise HfttError('FusedAdam.step inside averaged_weights(): the model holds the averaged weights, leave the context first')
        self.attach(self._find_engine())
        g = self.param_groups[0]
        mp = self._group_map()
        self.step_count += 1
        if g.get('ema_decay') is not None:
            self._step_ema(mp, grad_scale)
        elif not mp['trivial']:
            self._step_groups(mp, grad_scale)
        elif self._guarded(g):
            mg = g.get('max_grad_norm')
            ops.grad_norm(self.engine.flat_grads, self._ctl, self._ws, grad_scale=grad_scale, max_norm=math.inf if mg is None else float(mg))
            ops.adam_step_guarded(self.engine.flat_params, self.engine.flat_grads, self.exp_avg, self.exp_avg_sq, self.step_count, self._ctl,
                                  lr=float(g['lr']), beta1=g['betas'][0], beta2=g['betas'][1], eps=g['eps'], grad_scale=grad_scale,
                                  weight_decay=float(g.get('weight_decay', 0)))
        else:
            ops.adam_step(self.engine.flat_params, self.engine.flat_grads, self.exp_avg, self.exp_avg_sq, self.step_count,
                          lr=float(g['lr']), beta1=g['betas'][0], beta2=g['betas'][1], eps=g['eps'], grad_scale=grad_scale)
        self.engine._prepared_frozen = False          # (a frozen-weights inference engine must prepare its operands again)
        for p in self._params():
            self.state[p]['step'].fill_(self.step_count)
        return loss

    def _step_groups(self, mp, grad_scale):
        """the grouped kernels: one launch unguarded, norm + step guarded"""
        self._check_shared()
        groups, g0, eng = self.param_groups, self.param_groups[0], self.engine
        extra = len(mp['frozen']) - len(groups)     # (the group opened for requires_grad == False tensors: its constants are never read)
        ctl = None
        if any(self._guarded(g) for g in groups):
            mg = g0.get('max_grad_norm')
            ops.grad_norm_groups(eng.flat_grads, mp['qmap'], mp['mask'], self._ctl, self._ws, grad_scale=grad_scale,
                                 max_norm=math.inf if mg is None else float(mg))
            ctl = self._ctl
        ops.adam_step_groups(eng.flat_params, eng.flat_grads, self.exp_avg, self.exp_avg_sq, self.step_count, mp['qmap'],
                             lr=[float(g['lr']) for g in groups] + [0.0] * extra,
                             weight_decay=[float(g.get('weight_decay', 0)) for g in groups] + [0.0] * extra, frozen=mp['frozen'], ctl=ctl,
                             beta1=g0['betas'][0], beta2=g0['betas'][1], eps=g0['eps'], grad_scale=grad_scale)

    # ---- the averaged weights: the same three configurations through the one launch that also carries the average
    @staticmethod
    def _check_ema_decay(d):
        if d is not None and not 0.0 <= float(d) < 1.0:           # (false for NaN too)
            raise HfttError('FusedAdam: ema_decay=%r must be in [0, 1) (None: no averaged weights)' % (d,))

    @staticmethod
    def ema_decay_at(ema_decay, t, warmup=False):
        """the decay of call t (0-based): ema_decay, or with warmup min(ema_decay, (1 + t) / (10 + t))"""
        return min(float(ema_decay), (1.0 + t) / (10.0 + t)) if warmup else float(ema_decay)

    def _step_ema(self, mp, grad_scale):
        self._check_shared()
        groups, g0, eng = self.param_groups, self.param_groups[0], self.engine
        self._check_ema_decay(g0['ema_decay'])
        extra = len(mp['frozen']) - len(groups)
        ctl = None
        if any(self._guarded(g) for g in groups):
            mg = g0.get('max_grad_norm')
            max_norm = math.inf if mg is None else float(mg)
            if mp['trivial']:
                ops.grad_norm(eng.flat_grads, self._ctl, self._ws, grad_scale=grad_scale, max_norm=max_norm)
            else:
                ops.grad_norm_groups(eng.flat_grads, mp['qmap'], mp['mask'], self._ctl, self._ws, grad_scale=grad_scale, max_norm=max_norm)
            ctl = self._ctl
        beta = self.ema_decay_at(g0['ema_decay'], self.ema_updates, g0.get('ema_warmup', False))
        ops.adam_step_ema(eng.flat_params, eng.flat_grads, self.exp_avg, self.exp_avg_sq, self.ema, self.ema_c, self.step_count, beta,
                          lr=[float(g['lr']) for g in groups] + [0.0] * extra, quad_group=None if mp['trivial'] else mp['qmap'],
                          weight_decay=[float(g.get('weight_decay', 0)) for g in groups] + [0.0] * extra, frozen=mp['frozen'], ctl=ctl,
                          beta1=g0['betas'][0], beta2=g0['betas'][1], eps=g0['eps'], grad_scale=grad_scale)
        self.ema_updates += 1

    def _need_ema(self, what):
        if self.ema is None:
            raise HfttError('FusedAdam.%s: no averaged weights (build the optimizer with ema_decay= and attach it to an engine: a step, or a '
                            'TrainStep)' % what)

    @contextlib.contextmanager
    def averaged_weights(self):
        """The model holds the averaged weights inside the context and its own, bit for bit, after it.  The CONTENTS of the flat parameter
        buffer and of the average are swapped (launch plans and descriptors hold device addresses), and the engine is told to prepare its
        operands again on both sides.  ``step()`` inside is refused; the context does not nest."""
        self._need_ema('averaged_weights')
        if self._averaged:
            raise HfttError('FusedAdam.averaged_weights does not nest')
        self._swap_average()
        self._averaged = True
        try:
            yield self
        finally:
            self._swap_average()
            self._averaged = False

    @torch.no_grad()
    def _swap_average(self):
        tmp = self.engine.flat_params.clone()
        self.engine.flat_params.copy_(self.ema)
        self.ema.copy_(tmp)
        self.engine._prepared_frozen = False

    def averaged_model(self, model=None):
        """A CPU deep copy of the model (``model``, or the one given to the constructor) that holds the averaged weights: what
        ``pickle.dump(model.cpu(), fh, protocol=4)`` would write had training ended on the average.  One device-to-host copy of the
        average; the model on the device is not touched."""
        self._need_ema('averaged_model')
        model = self._model if model is None else model
        if model is None or not hasattr(model, 'hftt_state'):
            raise HfttError('FusedAdam.averaged_model: pass the model (the optimizer was built from its parameters alone)')
        if self._averaged:
            raise HfttError('FusedAdam.averaged_model inside averaged_weights(): the buffers are swapped, leave the context first')
        bound = self.engine._bound
        if any(a is not b for a, (_, b, _, _) in zip(model.parameters(), bound)):
            raise HfttError('FusedAdam.averaged_model: the model is not the one whose parameters the optimizer holds')
        avg = self.ema.cpu()
        memo = {id(p): torch.nn.Parameter(avg[o:o + n].clone().view(p.shape), requires_grad=p.requires_grad) for _, p, o, n in bound}
        twin = type(model).__new__(type(model))
        twin.__setstate__(model.hftt_state(memo))
        return twin.cpu()

    # ---- the guarded step: options in the parameter groups, the verdict and the counters in the device record
    @staticmethod
    def _guarded(g):
        return bool(g.get('guard', False)) or g.get('max_grad_norm') is not None or g.get('weight_decay', 0) != 0

    def _ctl_word(self, i, dtype=None):
        if self._ctl is None:
            raise HfttError('FusedAdam: not attached to an engine yet (the record of the guarded step lives on its device)')
        return (self._ctl if dtype is None else self._ctl.view(dtype))[i]

    @property
    def grad_norm(self):
        """|| grad_scale * g ||_2 of the last guarded step: a 0-dim fp32 DEVICE view (no sync; inf / nan when the step was skipped)"""
        return self._ctl_word(0, torch.float32)

    @property
    def clip_coef(self):
        """the factor the last guarded step applied on top of grad_scale (1: not clipped, 0: skipped): a 0-dim fp32 DEVICE view (no sync)"""
        return self._ctl_word(1, torch.float32)

    def _guard_counts(self):
        if self._ctl is None:
            return self._pending_guard or (0, 0)
        sk, cl = self._ctl[3:5].tolist()
        return int(sk) & 0xFFFFFFFF, int(cl) & 0xFFFFFFFF

    def _set_guard_counts(self, skipped, clipped):
        to_i32 = lambda x: ((int(x) & 0xFFFFFFFF) ^ 0x80000000) - 0x80000000      # noqa: E731  (the record's words are uint32)
        self._ctl[3:5] = torch.tensor([to_i32(skipped), to_i32(clipped)], dtype=torch.int32)

    @property
    def skipped_steps(self):
        """steps skipped so far because the gradient norm was not finite (a Python int: reading it synchronises with the device)"""
        return self._guard_counts()[0]

    @property
    def clipped_steps(self):
        """applied steps whose clip factor was below 1 (a Python int: reading it synchronises with the device)"""
        return self._guard_counts()[1]

    def state_dict(self):
        if self._averaged:
            raise HfttError('FusedAdam.state_dict inside averaged_weights(): parameters and average are swapped, leave the context first')
        sd = super().state_dict()
        sd['hftt_step_counter'] = None if self.engine is None else int(self.engine.step_counter)      # dropout stream position (resume)
        skipped, clipped = self._guard_counts()
        sd['hftt_guard'] = {'skipped': skipped, 'clipped': clipped}
        g0 = self.param_groups[0]
        sd['hftt_ema'] = {'decay': g0.get('ema_decay'), 'warmup': bool(g0.get('ema_warmup', False)), 'updates': int(self.ema_updates)}
        return sd

    def load_state_dict(self, state_dict):
        state_dict = dict(state_dict)
        ctr = state_dict.pop('hftt_step_counter', None)
        guard = state_dict.pop('hftt_guard', None)   # absent in older checkpoints and in the reference's .dat
        ema = state_dict.pop('hftt_ema', None)       # absent in checkpoints written before the averaged weights existed
        if self._averaged:
            raise HfttError('FusedAdam.load_state_dict inside averaged_weights(): leave the context first')
        super().load_state_dict(state_dict)          # torch's layout: state tensors are fresh copies, param_groups restored
        steps = [int(s['step']) for s in self.state.values() if 'step' in s]
        self.step_count = max(steps) if steps else 0
        for g in self.param_groups:                  # what the fused kernel does not implement must not be dropped silently
            l2 = g.get('weight_decay', 0) != 0 and not g.get('decoupled_weight_decay', False)       # (the decoupled form is the guarded kernel's)
            if l2 or g.get('amsgrad', False) or g.get('maximize', False):
                raise HfttError('FusedAdam: the loaded state asks for weight_decay / amsgrad / maximize, which the fused Adam kernel does not do '
                                '(reference: optim.Adam(model.parameters(), lr), m_training.py:146)')
            for k in ('max_grad_norm', 'guard', 'frozen'):     # a state written without the options keeps the ones this optimizer was built with
                g.setdefault(k, self.defaults[k])
            # the averaged weights: a state that carries no average (no option, or the option unset) leaves the option as this optimizer was
            # built -- the average then restarts from the parameters at attach; a state that carries one brings its option along
            if g.get('ema_decay') is None:
                g['ema_decay'], g['ema_warmup'] = self.defaults['ema_decay'], self.defaults['ema_warmup']
            g.setdefault('ema_warmup', False)
            self._check_ema_decay(g['ema_decay'])
        has_avg = bool(self.state) and all('ema' in s and 'ema_c' in s for s in self.state.values())
        self.ema_updates = int(ema['updates']) if (ema is not None and has_avg) else 0
        self._map = None
        eng, self.engine, self.exp_avg = self.engine, None, None
        self.ema = self.ema_c = None
        self._pending_counter = None
        self._pending_guard = None if guard is None else (int(guard['skipped']), int(guard['clipped']))
        if eng is not None:
            self.attach(eng)                         # copy the loaded moments into the flat buffers
            if ctr is not None:
                eng.step_counter = int(ctr)          # applied now: a TrainStep built later must not rewind the dropout stream again
        else:
            self._pending_counter = ctr              # no engine yet: applied when one is attached (attach / TrainStep)


class TrainStep:
    """One object per (model, optimizer): ``loss = step(spec, onset, offset, mpe, velocity)``."""

    def __init__(self, model, lr=1e-4, weight_A=1.0, weight_B=1.0, grad_sync=None, optimizer=None, loss_spec=None):
        self.model = model
        self.engine = model.hftt_engine()
        self.opt = optimizer if optimizer is not None else FusedAdam(model, lr=lr)
        self.opt.attach(self.engine)
        ctr = getattr(self.opt, '_pending_counter', None)
        if ctr is not None:
            self.engine.step_counter = int(ctr)
            self.opt._pending_counter = None
        self.weight_A, self.weight_B = weight_A, weight_B
        self.grad_sync = grad_sync          # callable(flat_grads) -> None (DDP all-reduce), or None
        self.loss_spec = loss_spec          # hftt_hip.criteria.LossSpec: the fused loss with its options (hftt_loss_w); None: the reference's criteria
        self._prune = 0                     # frozen stages of the last backward (flat_grads below its border was zeroed when it changed)

    def forward_backward(self, spec, label_onset, label_offset, label_mpe, label_velocity):
        eng = self.model.hftt_engine()
        if eng is not self.engine:
            raise HfttError('model was moved / re-bound after the TrainStep was created')
        B = spec.shape[0]
        with torch.cuda.device(eng.device):
            eng.forward(spec, training=self.model.training, save=True)
            loss = eng.loss(B, (label_onset, label_offset, label_mpe, label_velocity), self.weight_A, self.weight_B, with_grad=True, spec=self.loss_spec)
            # fine-tuning: the backward stops where nothing trainable remains (FusedAdam.frozen_stages; other optimizers: the whole backward).
            # The pruned backward does not write flat_grads below the border: zeroed once per change, so that p.grad views read zeros
            k = self.opt.frozen_stages() if hasattr(self.opt, 'frozen_stages') else 0
            lo = eng.frozen_border(k)
            if k != self._prune:
                eng.flat_grads[:lo].zero_()
                self._prune = k
            if self.grad_sync is not None:
                if lo:
                    self.grad_sync.begin_step(lo=lo)
                else:
                    self.grad_sync.begin_step()
            eng.backward(B, on_ready=getattr(self.grad_sync, 'bucket_ready', None), frozen_stages=k)
        return loss

    def __call__(self, spec, label_onset, label_offset, label_mpe, label_velocity):
        loss = self.forward_backward(spec, label_onset, label_offset, label_mpe, label_velocity)
        scale = 1.0
        if self.grad_sync is not None:
            scale = self.grad_sync(self.engine.flat_grads) or 1.0     # all-reduce(sum); the 1/world factor goes into Adam
        with torch.cuda.device(self.engine.device):
            self.opt.step(grad_scale=scale)
        return loss            # [9] device tensor: total + 8 terms (no host sync here)

    def expose_grads(self):
        for (name, p, o, n), g in zip(self.engine._bound, self.engine.grad_views()):
            p.grad = g
