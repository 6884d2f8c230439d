"""Criteria the fused loss launch takes besides the reference's (training/train.py:141-153: 6x nn.BCELoss + 2x nn.CrossEntropyLoss, plain
means): a positive-class weight and a soft-label focal modulation on the BCE heads, and class weights, ignore_index and label smoothing on
the velocity cross-entropy -- the remedies for targets where positives are well under 1 % of the elements.  Definitions:
include/hftt_hip.h (hftt_loss_w).

  BalancedBCELoss   an nn.Module with the value definition in torch ops: it runs on the CPU and on the compatibility path as it is;
  LossSpec          what the eight criteria of a training call become for hftt_loss_w: device tables and scalars.
                    LossSpec.from_criteria -> None (the reference's eight: hftt_loss runs as ever), a LossSpec, or False (a criterion the
                    fused launch does not do: the compatibility path runs as ever).
"""
import torch
import torch.nn as nn

from ._capi import HfttError

BCE_HEADS = ('onset_A', 'offset_A', 'mpe_A', 'onset_B', 'offset_B', 'mpe_B')      # the order of hftt_loss_desc.prob[6]
_BCE_AT = (0, 1, 2, 4, 5, 6)          # where they sit in train()'s eight criteria; the velocity cross-entropies are at 3 and 7
_CE_AT = (3, 7)


def _check_gamma(gamma):
    gamma = float(gamma)
    if not (gamma == 0.0 or 1.0 <= gamma <= 4.0):
        raise ValueError('gamma=%g must be 0 or in [1, 4]' % gamma)
    return gamma


class BalancedBCELoss(nn.Module):
    """mean_i m_i * -(a_j y_i log p_i + (1 - y_i) log(1 - p_i)),  m_i = |y_i - p_i|^gamma,  j = i mod Nn  (logs clamped at -100 as nn.BCELoss)

    pos_weight: a float, or a [Nn] tensor (one weight per pitch: the inputs' last dimension); it weighs the positive part only, which is
    BCEWithLogitsLoss(pos_weight=)'s definition.  gamma: 0 (no modulation), or in [1, 4]: the soft-label form of focal loss (quality focal
    loss) -- |y - p| rather than 1 - p_t, because onset and offset targets are ramps.  Deliberately NOT a subclass of nn.BCELoss: code that
    asks isinstance(c, nn.BCELoss) means the plain mean."""

    def __init__(self, pos_weight=1.0, gamma=0.0):
        super().__init__()
        self.gamma = _check_gamma(gamma)
        if torch.is_tensor(pos_weight):
            if pos_weight.dim() != 1 or pos_weight.numel() < 1:
                raise ValueError('pos_weight must be a float or a 1-D tensor [Nn]')
            t = pos_weight.detach().clone().to(torch.float32)
        else:
            t = torch.tensor([float(pos_weight)], dtype=torch.float32)
        if not bool((t > 0).all()):
            raise ValueError('pos_weight must be positive')
        self.scalar = not torch.is_tensor(pos_weight)
        self.register_buffer('pos_weight', t)

    def extra_repr(self):
        return 'pos_weight=%s, gamma=%g' % ('%g' % float(self.pos_weight[0]) if self.scalar else '[%d]' % self.pos_weight.numel(), self.gamma)

    def forward(self, p, y):
        p = p.reshape(-1)
        y = y.reshape(-1).to(p.dtype)
        a = self.pos_weight.to(device=p.device, dtype=p.dtype)
        if a.numel() > 1:
            if p.numel() % a.numel() != 0:
                raise ValueError('BalancedBCELoss: %d elements are no multiple of the %d pitches of pos_weight' % (p.numel(), a.numel()))
            a = a.repeat(p.numel() // a.numel())
        base = -(a * y * torch.log(p).clamp_min(-100.0) + (1.0 - y) * torch.log1p(-p).clamp_min(-100.0))
        if self.gamma != 0.0:
            base = (y - p).abs().pow(self.gamma) * base
        return base.mean()


def _plain_bce(c):
    return isinstance(c, nn.BCELoss) and c.reduction == 'mean' and c.weight is None


def _plain_ce(c):
    return (isinstance(c, nn.CrossEntropyLoss) and c.reduction == 'mean' and c.weight is None and c.label_smoothing == 0.0
            and c.ignore_index == -100)


def reference_criteria(crits):
    """the reference's eight (training/train.py:141-153): what hftt_loss computes"""
    return len(crits) == 8 and all(_plain_bce(crits[i]) for i in _BCE_AT) and all(_plain_ce(crits[i]) for i in _CE_AT)


class LossSpec:
    """The options of one hftt_loss_w call: per BCE head (BCE_HEADS order) a device table [Nn] or None and a gamma; per velocity side a device
    table [V] or None, a smoothing and an ignore_index."""

    def __init__(self, Nn, V, pos_weight, gamma, class_weight, smoothing, ignore_index):
        self.Nn, self.V = int(Nn), int(V)
        self.pos_weight, self.gamma = list(pos_weight), [_check_gamma(g) for g in gamma]
        self.class_weight, self.smoothing, self.ignore_index = list(class_weight), [float(e) for e in smoothing], [int(k) for k in ignore_index]
        if len(self.pos_weight) != 6 or len(self.gamma) != 6 or len(self.class_weight) != 2 or len(self.smoothing) != 2 or len(self.ignore_index) != 2:
            raise HfttError('LossSpec: six BCE heads and two velocity sides')
        for t, k in [(t, self.Nn) for t in self.pos_weight] + [(t, self.V) for t in self.class_weight]:
            if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != k):
                raise HfttError('LossSpec: tables are contiguous fp32 tensors of [Nn] resp. [V] elements')
        for e in self.smoothing:
            if not 0.0 <= e < 1.0:
                raise HfttError('LossSpec: smoothing=%g must be in [0, 1)' % e)

    @property
    def needs_prepass(self):
        """a side's divisor W is summed from the labels when they can weigh other than 1 (include/hftt_hip.h)"""
        return any(t is not None or 0 <= k < self.V for t, k in zip(self.class_weight, self.ignore_index))

    @classmethod
    def from_criteria(cls, crits, Nn, V, device):
        """None: the reference's eight criteria.  A LossSpec: every BCE criterion is a plain nn.BCELoss() or a BalancedBCELoss, every velocity
        criterion an nn.CrossEntropyLoss(weight=?, ignore_index=?, label_smoothing=?, reduction='mean').  False: anything else (an
        nn.BCELoss(weight=), another reduction, another class)."""
        crits = tuple(crits)
        if reference_criteria(crits):
            return None
        if len(crits) != 8:
            return False
        pos_weight, gamma = [], []
        for i in _BCE_AT:
            c = crits[i]
            if _plain_bce(c):
                pos_weight.append(None); gamma.append(0.0)
            elif isinstance(c, BalancedBCELoss):
                a = c.pos_weight.detach()
                if a.numel() == 1:
                    a = None if float(a[0]) == 1.0 else a.expand(Nn)
                elif a.numel() != Nn:
                    raise HfttError('BalancedBCELoss.pos_weight has %d entries, the model %d pitches' % (a.numel(), Nn))
                pos_weight.append(None if a is None else a.to(device=device, dtype=torch.float32).contiguous())
                gamma.append(c.gamma)
            else:
                return False
        class_weight, smoothing, ignore_index = [], [], []
        for i in _CE_AT:
            c = crits[i]
            if not (isinstance(c, nn.CrossEntropyLoss) and c.reduction == 'mean' and 0.0 <= c.label_smoothing < 1.0):
                return False
            w = c.weight
            if w is not None:
                if w.dim() != 1 or w.numel() != V:
                    return False
                w = w.detach().to(device=device, dtype=torch.float32).contiguous()
            class_weight.append(w); smoothing.append(c.label_smoothing); ignore_index.append(c.ignore_index)
        return cls(Nn, V, pos_weight, gamma, class_weight, smoothing, ignore_index)

    def fill(self, dsc, ws_w):
        """write the options into a LossWDesc (dsc.base is the caller's); ws_w: the pre-pass workspace, a device tensor or None"""
        dsc.Nn = self.Nn
        for i in range(6):
            dsc.pos_weight[i] = None if self.pos_weight[i] is None else self.pos_weight[i].data_ptr()
            dsc.gamma[i] = self.gamma[i]
        for s in range(2):
            dsc.class_weight[s] = None if self.class_weight[s] is None else self.class_weight[s].data_ptr()
            dsc.smoothing[s] = self.smoothing[s]
            dsc.ignore_index[s] = self.ignore_index[s]
        dsc.ws_w = None if ws_w is None else ws_w.data_ptr()
