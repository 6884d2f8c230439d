"""Host side of the class-balanced and focal criteria, without a GPU: which criteria tuples stay on the fused path
(hftt_hip.criteria.LossSpec.from_criteria: None / a spec / False), what the spec holds, BalancedBCELoss's argument checks, how
training.train picks its path, and the criterion flags of tools/train_config5.py."""
import argparse
import importlib.util
import os
import types

import pytest
import torch
import torch.nn as nn

import util

NN, V = 88, 128


def _reference():
    return [nn.BCELoss(), nn.BCELoss(), nn.BCELoss(), nn.CrossEntropyLoss()] * 2


def _with(**at):
    c = _reference()
    for i, v in at.items():
        c[int(i[1:])] = v
    return tuple(c)


def test_the_reference_criteria_give_none():
    from hftt_hip.criteria import LossSpec, reference_criteria
    assert LossSpec.from_criteria(_reference(), NN, V, 'cpu') is None
    assert reference_criteria(tuple(_reference()))

    class MyBCE(nn.BCELoss):          # a subclass of the plain mean is the plain mean, as training.train has always read it
        pass
    assert LossSpec.from_criteria(_with(c0=MyBCE()), NN, V, 'cpu') is None


def test_supported_criteria_give_a_spec():
    from hftt_hip.criteria import BalancedBCELoss, LossSpec
    ramp = torch.linspace(0.5, 8.0, NN)
    cw = torch.ones(V)
    cw[0] = 0.1
    crits = _with(c0=BalancedBCELoss(pos_weight=4.0), c1=BalancedBCELoss(pos_weight=ramp, gamma=2.0), c3=nn.CrossEntropyLoss(weight=cw),
                  c5=BalancedBCELoss(gamma=1.5), c7=nn.CrossEntropyLoss(ignore_index=0, label_smoothing=0.1))
    s = LossSpec.from_criteria(crits, NN, V, 'cpu')
    assert isinstance(s, LossSpec) and (s.Nn, s.V) == (NN, V)
    # heads in prob[6]'s order: onset_A, offset_A, mpe_A, onset_B, offset_B, mpe_B
    assert s.gamma == [0.0, 2.0, 0.0, 0.0, 1.5, 0.0]
    assert torch.equal(s.pos_weight[0], torch.full((NN,), 4.0)) and torch.equal(s.pos_weight[1], ramp)
    assert all(s.pos_weight[h] is None for h in (2, 3, 4, 5))          # (a scalar 1 needs no table)
    assert torch.equal(s.class_weight[0], cw) and s.class_weight[1] is None
    assert s.smoothing == [0.0, 0.1] and s.ignore_index == [-100, 0] and s.needs_prepass
    for t in (s.pos_weight[0], s.pos_weight[1], s.class_weight[0]):
        assert t.dtype == torch.float32 and t.is_contiguous()
    # no class weights and no label that could be ignored: W = n, the pre-pass is skipped
    s2 = LossSpec.from_criteria(_with(c0=BalancedBCELoss(pos_weight=4.0), c7=nn.CrossEntropyLoss(ignore_index=V, label_smoothing=0.1)), NN, V, 'cpu')
    assert isinstance(s2, LossSpec) and not s2.needs_prepass
    # a neutral BalancedBCELoss is still a spec (hftt_loss_w produces hftt_loss's bits for it)
    s3 = LossSpec.from_criteria(_with(c2=BalancedBCELoss()), NN, V, 'cpu')
    assert isinstance(s3, LossSpec) and s3.pos_weight == [None] * 6 and s3.gamma == [0.0] * 6


@pytest.mark.parametrize('name', ['bce_weight', 'bce_sum', 'ce_sum', 'ce_none', 'mse', 'bce_logits', 'ce_weight_shape', 'seven'])
def test_other_criteria_stay_false(name):
    from hftt_hip.criteria import LossSpec
    crits = {
        'bce_weight': _with(c0=nn.BCELoss(weight=torch.ones(NN))),                 # a per-element weight is not the positive-class weight
        'bce_sum': _with(c1=nn.BCELoss(reduction='sum')), 'ce_sum': _with(c3=nn.CrossEntropyLoss(reduction='sum')),
        'ce_none': _with(c7=nn.CrossEntropyLoss(reduction='none')), 'mse': _with(c2=nn.MSELoss()),
        'bce_logits': _with(c4=nn.BCEWithLogitsLoss(pos_weight=torch.ones(NN))),   # takes logits: another function of the model's output
        'ce_weight_shape': _with(c3=nn.CrossEntropyLoss(weight=torch.ones(V + 1))), 'seven': tuple(_reference()[:7]),
    }[name]
    assert LossSpec.from_criteria(crits, NN, V, 'cpu') is False


def test_balanced_bce_arguments_and_value():
    from hftt_hip import HfttError
    from hftt_hip.criteria import BalancedBCELoss, LossSpec
    assert not isinstance(BalancedBCELoss(), nn.BCELoss)
    for bad in (dict(gamma=0.5), dict(gamma=4.5), dict(gamma=-1.0), dict(gamma=float('nan')), dict(pos_weight=0.0), dict(pos_weight=-1.0),
                dict(pos_weight=torch.tensor([1.0, 0.0])), dict(pos_weight=torch.ones(2, 2))):
        with pytest.raises(ValueError):
            BalancedBCELoss(**bad)
    with pytest.raises(HfttError, match='87 entries, the model 88 pitches'):
        LossSpec.from_criteria(_with(c0=BalancedBCELoss(pos_weight=torch.ones(87))), NN, V, 'cpu')
    g = torch.Generator().manual_seed(3)
    p, y = torch.rand(4, NN, generator=g, dtype=torch.float64), torch.rand(4, NN, generator=g, dtype=torch.float64)
    # neutral: nn.BCELoss; a weight: BCEWithLogitsLoss(pos_weight=) on the logits of p
    assert torch.allclose(BalancedBCELoss().double()(p, y), nn.BCELoss()(p, y), rtol=1e-14)
    w = torch.linspace(0.5, 8.0, NN, dtype=torch.float64)
    ref = nn.BCEWithLogitsLoss(pos_weight=w)(torch.log(p) - torch.log1p(-p), y)
    assert torch.allclose(BalancedBCELoss(pos_weight=w).double()(p, y), ref, rtol=1e-12)
    # the focal factor |y - p|^gamma, element by element
    foc = ((y - p).abs() ** 2 * -(y * torch.log(p) + (1 - y) * torch.log1p(-p))).mean()
    assert torch.allclose(BalancedBCELoss(gamma=2.0).double()(p, y), foc, rtol=1e-14)
    with pytest.raises(ValueError, match='no multiple'):
        BalancedBCELoss(pos_weight=torch.ones(3))(torch.rand(10), torch.rand(10))


def test_train_picks_its_path_from_the_criteria():
    """training.train._loss_spec: the reference's criteria never ask the model for an engine; a spec is built for the engine's Nn and V"""
    from hftt_hip.criteria import BalancedBCELoss, LossSpec
    from training import train as T

    class NoEngine:
        def hftt_engine(self):
            raise AssertionError('the reference criteria need no engine')
    assert T._loss_spec(NoEngine(), tuple(_reference()), 'cpu') == (True, None)
    model = types.SimpleNamespace(hftt_engine=lambda: types.SimpleNamespace(N=NN, V=V))
    fast, spec = T._loss_spec(model, _with(c0=BalancedBCELoss(pos_weight=4.0, gamma=2.0)), 'cpu')
    assert fast and isinstance(spec, LossSpec) and spec.gamma[0] == 2.0
    assert T._loss_spec(model, _with(c0=nn.BCELoss(weight=torch.ones(NN))), 'cpu') == (False, None)
    assert 'hftt_loss_w' in T.__doc__ and 'BalancedBCELoss' in T.__doc__


@pytest.fixture(scope='module')
def tool():
    spec = importlib.util.spec_from_file_location('train_config5_tool', os.path.join(util.ROOT, 'tools', 'train_config5.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _args(tool, argv):
    ap = argparse.ArgumentParser()
    tool.add_loss_arguments(ap)
    return ap.parse_args(argv)


def test_tool_flags_default_to_the_reference_criteria(tool):
    from hftt_hip.criteria import LossSpec
    crits = tool.build_criteria(_args(tool, []))
    assert len(crits) == 8 and LossSpec.from_criteria(crits, NN, V, 'cpu') is None
    assert [type(c) for c in crits] == [nn.BCELoss, nn.BCELoss, nn.BCELoss, nn.CrossEntropyLoss] * 2


def test_tool_flags_build_the_expected_criteria(tool):
    from hftt_hip.criteria import BalancedBCELoss, LossSpec
    crits = tool.build_criteria(_args(tool, ['--onset-pos-weight', '4', '--focal-gamma', '2', '--velocity-silence-weight', '0.1']))
    for i in (0, 1, 2, 4, 5, 6):
        assert isinstance(crits[i], BalancedBCELoss) and crits[i].gamma == 2.0
        assert float(crits[i].pos_weight[0]) == (4.0 if i in (0, 4) else 1.0)
    for i in (3, 7):
        w = crits[i].weight
        assert isinstance(crits[i], nn.CrossEntropyLoss) and w.shape == (V,) and abs(float(w[0]) - 0.1) < 1e-7 and bool((w[1:] == 1).all())
        assert crits[i].label_smoothing == 0.0
    s = LossSpec.from_criteria(crits, NN, V, 'cpu')
    assert isinstance(s, LossSpec) and s.gamma == [2.0] * 6 and s.needs_prepass
    assert torch.equal(s.pos_weight[0], torch.full((NN,), 4.0)) and s.pos_weight[1] is None and torch.equal(s.pos_weight[3], s.pos_weight[0])
    # one flag at a time: only what it names changes
    crits = tool.build_criteria(_args(tool, ['--offset-pos-weight', '3', '--mpe-pos-weight', '2']))
    assert [type(c) for c in crits[:4]] == [nn.BCELoss, BalancedBCELoss, BalancedBCELoss, nn.CrossEntropyLoss]
    assert float(crits[1].pos_weight[0]) == 3.0 and float(crits[2].pos_weight[0]) == 2.0 and crits[1].gamma == 0.0
    crits = tool.build_criteria(_args(tool, ['--label-smoothing', '0.1']))
    assert crits[3].label_smoothing == 0.1 and crits[3].weight is None and type(crits[0]) is nn.BCELoss
    assert not LossSpec.from_criteria(crits, NN, V, 'cpu').needs_prepass
    with pytest.raises(ValueError):
        tool.build_criteria(_args(tool, ['--focal-gamma', '0.5']))
