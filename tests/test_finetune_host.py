"""Host half of fine-tuning (no GPU): the per-quad group map, stage_groups, FusedAdam's group handling and frozen_stages() on a CPU-built
tiny model with offsets from layout.flat_offsets."""
import numpy as np
import pytest
import torch

import util
from hftt_hip import HfttError, ops
from hftt_hip.layout import flat_offsets
from hftt_hip.trainer import STAGE_BORDERS, FusedAdam, stage_groups


@pytest.fixture()
def model():
    return util.build_model(util.MINI, 3)


def _layout(model):
    named = list(model.named_parameters())
    offs, total = flat_offsets((n, p.numel()) for n, p in named)
    return named, offs, total


def test_group_map_covers_parameters_and_gaps(model):
    named, offs, total = _layout(model)
    assert total % 8 == 0 and all(o % 8 == 0 for o in offs)
    assert any((o + p.numel()) % 8 for (_, p), o in zip(named, offs))            # the tiny model does have alignment gaps
    entries = [(o, p.numel(), i % 3) for i, ((_, p), o) in enumerate(zip(named, offs))]
    qmap = ops.adam_group_map(entries, total)
    assert qmap.dtype == torch.uint8 and qmap.numel() == total // 4
    q = qmap.numpy()
    for i, (o, k, gi) in enumerate(entries):
        end = entries[i + 1][0] if i + 1 < len(entries) else total
        assert (q[o // 4:end // 4] == gi).all()              # the parameter's quads and the gap quads behind it
    with pytest.raises(HfttError):
        ops.adam_group_map([(0, 8, 0), (4, 8, 1)], 16)       # overlap
    with pytest.raises(HfttError):
        ops.adam_group_map([(0, 8, 8)], 8)                   # group index beyond 7
    with pytest.raises(HfttError):
        ops.adam_group_map([(0, 8, 0)], 10)                  # total not a multiple of 4


def test_stage_groups_split_at_the_backward_marks(model):
    named, offs, total = _layout(model)
    off = {n: o for (n, _), o in zip(named, offs)}
    groups = stage_groups(model, encoder=dict(frozen=True), time=dict(lr=1e-3))
    assert [g['stage'] for g in groups] == ['encoder', 'freq', 'time']
    assert groups[0]['frozen'] is True and groups[2]['lr'] == 1e-3 and 'lr' not in groups[1]
    opt = FusedAdam(groups, lr=1e-4, model=model)
    mp = opt._group_map()
    q = mp['host'].numpy()
    b0, b1 = (off[b] for b in STAGE_BORDERS)
    change = (np.nonzero(np.diff(q.astype(int)))[0] + 1) * 4
    assert list(change) == [b0, b1] and mp['borders'] == (0, b0, b1)
    assert (q[:b0 // 4] == 0).all() and (q[b0 // 4:b1 // 4] == 1).all() and (q[b1 // 4:] == 2).all()
    gi_of = {id(p): i for i, g in enumerate(opt.param_groups) for p in g['params']}
    for (n, p), o in zip(named, offs):
        assert (q[o // 4:(o + p.numel() + 3) // 4] == gi_of[id(p)]).all(), n
    assert opt.param_groups[1]['lr'] == 1e-4 and opt.param_groups[1]['frozen'] is False
    assert mp['frozen'] == [True, False, False] and mp['mask'] == 1 and not mp['trivial']


def test_no_decay_1d_twins_hold_exactly_the_1d_tensors(model):
    groups = stage_groups(model, no_decay_1d=True)
    assert [g['stage'] for g in groups] == ['encoder', 'encoder.no_decay', 'freq', 'freq.no_decay', 'time', 'time.no_decay']
    opt = FusedAdam(groups, lr=1e-3, weight_decay=0.01, model=model)
    n1 = 0
    for g in opt.param_groups:
        twin = g['stage'].endswith('.no_decay')
        assert g['weight_decay'] == (0.0 if twin else 0.01) and g['decoupled_weight_decay'] is (not twin)
        assert all((p.dim() <= 1) == twin for p in g['params'])
        n1 += len(g['params']) if twin else 0
    assert n1 == sum(1 for p in model.parameters() if p.dim() <= 1) > 0
    assert sum(len(g['params']) for g in opt.param_groups) == len(list(model.parameters()))
    assert opt.frozen_stages() == 0


def test_frozen_stages(model):
    named = list(model.named_parameters())
    names = [n for n, _ in named]
    cut = [names.index(b) for b in STAGE_BORDERS]
    mk = lambda **kw: FusedAdam(stage_groups(model, **kw), lr=1e-3, model=model)          # noqa: E731
    assert mk().frozen_stages() == 0
    assert mk(encoder=dict(frozen=True)).frozen_stages() == 1
    assert mk(encoder=dict(frozen=True), freq=dict(frozen=True)).frozen_stages() == 2
    assert mk(freq=dict(frozen=True)).frozen_stages() == 0                                # not a prefix
    assert mk(encoder=dict(frozen=True), freq=dict(frozen=True), time=dict(frozen=True)).frozen_stages() == 2
    # one plain group: the requires_grad flags alone freeze, and the map follows them
    opt = FusedAdam(model.parameters(), lr=1e-3, model=model)
    assert opt.frozen_stages() == 0 and opt._group_map()['trivial']
    for _, p in named[:cut[0] - 1]:
        p.requires_grad_(False)
    assert opt.frozen_stages() == 0 and not opt._group_map()['trivial']                   # part of the encoder only
    named[cut[0] - 1][1].requires_grad_(False)
    assert opt.frozen_stages() == 1
    named[cut[0]][1].requires_grad_(False)
    named[cut[0] + 3][1].requires_grad_(False)
    assert opt.frozen_stages() == 1                                                       # encoder and part of the frequency decoder
    for _, p in named[cut[0]:cut[1]]:
        p.requires_grad_(False)
    assert opt.frozen_stages() == 2
    assert opt._group_map()['frozen'] == [False, True]                                    # the flagged tensors live in a group of their own
    for _, p in named:
        p.requires_grad_(True)
    assert opt.frozen_stages() == 0 and opt._group_map()['trivial']
    # a group's option changes under the optimizer: the signature notices
    opt = mk()
    assert opt.frozen_stages() == 0
    opt.param_groups[0]['frozen'] = True
    assert opt.frozen_stages() == 1


def test_refusals(model):
    ps = list(model.parameters())
    with pytest.raises(HfttError, match='exactly the parameters'):
        FusedAdam([dict(params=ps[:10]), dict(params=ps[11:])], lr=1e-3, model=model).frozen_stages()          # one missing
    with pytest.raises(HfttError, match='more than one group'):
        FusedAdam([dict(params=ps[:10]), dict(params=ps[9:])], lr=1e-3, model=model)                           # one repeated
    with pytest.raises(HfttError, match='1 to 8 parameter groups'):
        FusedAdam([dict(params=[p]) for p in ps[:8]] + [dict(params=ps[8:])], lr=1e-3, model=model)
    with pytest.raises(HfttError, match='disagree on betas'):
        FusedAdam([dict(params=ps[:10]), dict(params=ps[10:], betas=(0.8, 0.999))], lr=1e-3, model=model)
    with pytest.raises(HfttError, match='disagree on guard'):
        FusedAdam([dict(params=ps[:10], guard=True), dict(params=ps[10:])], lr=1e-3, model=model)
    with pytest.raises(HfttError, match='weight_decay'):
        FusedAdam([dict(params=ps[:10], weight_decay=-1.0), dict(params=ps[10:])], lr=1e-3, model=model)
    with pytest.raises(HfttError, match='needs the flat layout'):
        FusedAdam(stage_groups(model), lr=1e-3).frozen_stages()
    # eight groups are fine
    assert FusedAdam([dict(params=[p]) for p in ps[:7]] + [dict(params=ps[7:])], lr=1e-3, model=model).frozen_stages() == 0


def test_state_dict_carries_groups_and_refuses_another_structure(model):
    a = FusedAdam(stage_groups(model, encoder=dict(frozen=True, lr=1e-5)), lr=1e-3, model=model)
    sd = a.state_dict()
    assert [g['frozen'] for g in sd['param_groups']] == [True, False, False] and sd['param_groups'][0]['lr'] == 1e-5
    b = FusedAdam(stage_groups(model), lr=1e-4, model=model)
    assert b.frozen_stages() == 0
    b.load_state_dict(sd)
    assert [g['frozen'] for g in b.param_groups] == [True, False, False] and b.param_groups[0]['lr'] == 1e-5
    assert b.frozen_stages() == 1
    with pytest.raises(ValueError):
        FusedAdam(model.parameters(), lr=1e-4).load_state_dict(sd)
