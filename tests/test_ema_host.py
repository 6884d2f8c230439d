"""Host half of the averaged weights: FusedAdam's ema_decay / ema_warmup options, what the parameter groups and the state dict carry, and
load_state_dict's rules -- all without an engine, on the CPU."""
import math

import pytest
import torch

import util


def _model():
    return util.build_model(util.MINI, 3)


def test_the_options_default_to_off_and_live_in_the_parameter_group():
    from hftt_hip.trainer import FusedAdam
    opt = FusedAdam(_model().parameters(), lr=1e-3)
    g = opt.param_groups[0]
    assert g['ema_decay'] is None and g['ema_warmup'] is False
    assert opt.ema is None and opt.ema_c is None and opt.ema_updates == 0
    assert not FusedAdam._guarded(g)                                        # the average does not turn the guard on
    opt = FusedAdam(_model().parameters(), lr=1e-3, ema_decay=0.9999, ema_warmup=True)
    g = opt.param_groups[0]
    assert g['ema_decay'] == 0.9999 and g['ema_warmup'] is True and not FusedAdam._guarded(g)
    assert FusedAdam(_model().parameters(), ema_decay=0).param_groups[0]['ema_decay'] == 0.0          # beta = 0: the average is the last iterate
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt)                 # still a real torch Optimizer
    assert sched.optimizer is opt


@pytest.mark.parametrize('bad', [1.0, 1.5, -0.1, math.nan, math.inf])
def test_a_decay_outside_0_1_is_refused(bad):
    from hftt_hip import HfttError
    from hftt_hip.trainer import FusedAdam
    with pytest.raises(HfttError, match='ema_decay'):
        FusedAdam(_model().parameters(), ema_decay=bad)
    model = _model()
    ps = list(model.parameters())
    with pytest.raises(HfttError, match='ema_decay'):
        FusedAdam([{'params': ps[:2], 'ema_decay': bad}, {'params': ps[2:]}], model=model)


def test_groups_that_disagree_on_the_average_are_refused():
    from hftt_hip import HfttError
    from hftt_hip.trainer import FusedAdam
    model = _model()
    ps = list(model.parameters())
    with pytest.raises(HfttError, match='disagree on ema_decay'):
        FusedAdam([{'params': ps[:2], 'ema_decay': 0.999}, {'params': ps[2:]}], lr=1e-3, ema_decay=0.9999, model=model)
    with pytest.raises(HfttError, match='disagree on ema_decay'):
        FusedAdam([{'params': ps[:2], 'ema_decay': 0.999}, {'params': ps[2:]}], lr=1e-3, model=model)
    with pytest.raises(HfttError, match='disagree on ema_warmup'):
        FusedAdam([{'params': ps[:2], 'ema_warmup': True}, {'params': ps[2:]}], lr=1e-3, ema_decay=0.9999, model=model)
    opt = FusedAdam([{'params': ps[:2], 'lr': 1e-4}, {'params': ps[2:]}], lr=1e-3, ema_decay=0.9999, model=model)
    assert [g['ema_decay'] for g in opt.param_groups] == [0.9999, 0.9999]


def test_the_state_dict_key_is_present_without_an_engine():
    from hftt_hip.trainer import FusedAdam
    sd = FusedAdam(_model().parameters(), lr=1e-3).state_dict()
    assert sd['hftt_ema'] == {'decay': None, 'warmup': False, 'updates': 0}
    sd = FusedAdam(_model().parameters(), lr=1e-3, ema_decay=0.999, ema_warmup=True).state_dict()
    assert sd['hftt_ema'] == {'decay': 0.999, 'warmup': True, 'updates': 0}
    assert sd['param_groups'][0]['ema_decay'] == 0.999 and sd['param_groups'][0]['ema_warmup'] is True


def test_without_an_engine_the_averaged_views_are_refused():
    from hftt_hip import HfttError
    from hftt_hip.trainer import FusedAdam
    model = _model()
    for opt in (FusedAdam(model.parameters(), ema_decay=0.99, model=model), FusedAdam(model.parameters(), model=model)):
        with pytest.raises(HfttError, match='no averaged weights'):
            with opt.averaged_weights():
                pass
        with pytest.raises(HfttError, match='no averaged weights'):
            opt.averaged_model()


def _state_with_average(model, decay=0.99, updates=7):
    """what an optimizer with the option writes after `updates` calls, built by hand (no engine here): torch Adam's state plus ema / ema_c"""
    ref = torch.optim.Adam(model.parameters(), lr=2e-4)
    for p in model.parameters():
        p.grad = torch.ones_like(p)
    ref.step()
    sd = ref.state_dict()
    for i, p in enumerate(model.parameters()):
        sd['state'][i]['ema'] = p.detach() * 0.5
        sd['state'][i]['ema_c'] = torch.full_like(p, 1e-9)
    sd['param_groups'][0].update(ema_decay=decay, ema_warmup=True)
    sd['hftt_ema'] = {'decay': decay, 'warmup': True, 'updates': updates}
    return sd


def test_load_state_dict_on_the_cpu():
    from hftt_hip.trainer import FusedAdam
    model = _model()
    # a state without the average (a checkpoint of before, or torch Adam's / the reference's) into an optimizer with the option: the option
    # stays, the count restarts; the average itself restarts from the parameters at attach
    old = torch.optim.Adam(model.parameters(), lr=2e-4).state_dict()
    assert 'hftt_ema' not in old and 'ema_decay' not in old['param_groups'][0]
    opt = FusedAdam(model.parameters(), lr=1e-3, ema_decay=0.9999, ema_warmup=True)
    opt.ema_updates = 5
    opt.load_state_dict(old)
    g = opt.param_groups[0]
    assert g['lr'] == 2e-4 and g['ema_decay'] == 0.9999 and g['ema_warmup'] is True and opt.ema_updates == 0
    # ... the same when the state was written by a FusedAdam without the option (its groups say ema_decay None)
    plain = FusedAdam(model.parameters(), lr=3e-4).state_dict()
    assert plain['param_groups'][0]['ema_decay'] is None
    opt = FusedAdam(model.parameters(), lr=1e-3, ema_decay=0.999)
    opt.load_state_dict(plain)
    assert opt.param_groups[0]['ema_decay'] == 0.999 and opt.param_groups[0]['lr'] == 3e-4
    # a state WITH the average into an optimizer without the option: kept, and the option is on
    sd = _state_with_average(model)
    opt = FusedAdam(model.parameters(), lr=1e-3)
    opt.load_state_dict(sd)
    g = opt.param_groups[0]
    assert g['ema_decay'] == 0.99 and g['ema_warmup'] is True and opt.ema_updates == 7
    for p in model.parameters():
        assert torch.equal(opt.state[p]['ema'], p.detach() * 0.5) and torch.equal(opt.state[p]['ema_c'], torch.full_like(p, 1e-9))
    out = opt.state_dict()
    assert out['hftt_ema'] == {'decay': 0.99, 'warmup': True, 'updates': 7}
    assert all('ema' in s and 'ema_c' in s for s in out['state'].values())
    # a broken decay in a state is refused like one in the constructor
    from hftt_hip import HfttError
    sd = _state_with_average(model, decay=1.0)
    with pytest.raises(HfttError, match='ema_decay'):
        FusedAdam(model.parameters(), lr=1e-3).load_state_dict(sd)
