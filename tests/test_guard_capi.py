"""C ABI and host half of the guarded optimizer step (hftt_grad_norm, hftt_adam_step_guarded, FusedAdam's options): the record's layout
against the C compiler, every host-side refusal with its message (they run before the device guard and the launch, so a box without a GPU
tests them), and FusedAdam.load_state_dict on the CPU.  No compute calls."""
import ctypes as C
import math
import os
import subprocess

import pytest
import torch

import util

HDR = os.path.join(util.ROOT, 'include', 'hftt_hip.h')


@pytest.fixture(scope='module')
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location('hftt_build', os.path.join(util.ROOT, 'nylon-amt_amd', 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build(verbose=False)
    from hftt_hip import _capi
    return _capi.lib()


def test_record_layout_matches_the_c_compiler(lib, tmp_path):
    from hftt_hip import _capi
    cls, cname = _capi.GuardCtl, 'hftt_guard_ctl'
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % HDR, 'int main(void) {',
             'printf("%s %%zu\\n", sizeof(%s));' % (cname, cname)]
    for f in cls._fields_:
        lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f[0], cname, f[0]))
    lines += ['printf("HFTT_ABI_VERSION %d\\n", HFTT_ABI_VERSION);', 'return 0; }']
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'layout'
    subprocess.run(['gcc', '-std=c99', str(src), '-o', str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split('\n') if l)
    assert int(got[cname]) == C.sizeof(cls) == 32
    for f in cls._fields_:
        assert int(got['%s.%s' % (cname, f[0])]) == getattr(cls, f[0]).offset, f[0]
    assert [getattr(cls, f).offset for f in ('norm', 'coef', 'apply', 'skipped', 'clipped')] == [0, 4, 8, 12, 16]      # the words ops / FusedAdam read
    assert int(got['HFTT_ABI_VERSION']) == 8 == lib.hftt_abi_version() == _capi.ABI_VERSION          # the symbols were added AT version 8
    for name in ('hftt_grad_norm_ws_bytes', 'hftt_grad_norm', 'hftt_adam_step_guarded'):
        assert name in _capi.SIGNATURES and hasattr(lib, name)


def test_workspace_size(lib):
    for n in (1, 5, 1025, 2048 * 256 * 4 + 5, 1 << 33):
        b = lib.hftt_grad_norm_ws_bytes(n)
        assert b > 0 and b % 16 == 0
    # one fp64 partial per workgroup of the capped grid
    assert lib.hftt_grad_norm_ws_bytes(1 << 33) >= 2048 * 8


P = 0x1000          # a non-null, 16-byte aligned "device pointer": every case below is refused before anything dereferences it

NORM_OK = dict(g=P, n=1024, grad_scale=1.0, max_norm=1.0, ws=P, ctl=P)
NORM_REJECTS = [({'g': None}, b'null operand'), ({'ws': None}, b'null operand'), ({'ctl': None}, b'null operand'),
                ({'n': 0}, b'n=0'), ({'n': -3}, b'n=-3'),
                ({'g': P + 4}, b'16-byte aligned'), ({'ws': P + 8}, b'16-byte aligned'), ({'ctl': P + 4}, b'16-byte aligned'),
                ({'grad_scale': math.inf}, b'grad_scale must be finite'), ({'grad_scale': -math.inf}, b'grad_scale must be finite'),
                ({'grad_scale': math.nan}, b'grad_scale must be finite'),
                ({'max_norm': math.nan}, b'max_norm must be positive'), ({'max_norm': 0.0}, b'max_norm must be positive'),
                ({'max_norm': -1.0}, b'max_norm must be positive')]


@pytest.mark.parametrize('kw,msg', NORM_REJECTS, ids=['-'.join('%s=%s' % kv for kv in k.items()) for k, _ in NORM_REJECTS])
def test_grad_norm_rejects_before_any_launch(lib, kw, msg):
    a = dict(NORM_OK, **kw)
    assert lib.hftt_grad_norm(a['g'], a['n'], a['grad_scale'], a['max_norm'], a['ws'], a['ctl'], None) not in (0, 2, 3)
    err = lib.hftt_last_error()
    assert err.startswith(b'grad_norm: ') and msg in err, err


ADAM_OK = dict(p=P, g=P, m=P, v=P, n=1024, step=1, lr=1e-3, weight_decay=0.01, ctl=P)
ADAM_REJECTS = [({'p': None}, b'bad arguments'), ({'g': None}, b'bad arguments'), ({'m': None}, b'bad arguments'), ({'v': None}, b'bad arguments'),
                ({'n': 0}, b'bad arguments'), ({'step': 0}, b'bad arguments'),
                ({'p': P + 4}, b'buffers must be 16-byte aligned'), ({'g': P + 8}, b'buffers must be 16-byte aligned'),
                ({'m': P + 4}, b'buffers must be 16-byte aligned'), ({'v': P + 12}, b'buffers must be 16-byte aligned'),
                ({'ctl': None}, b'ctl is null'), ({'ctl': P + 8}, b'ctl must be 16-byte aligned'),
                ({'weight_decay': math.nan}, b'weight_decay must be >= 0'), ({'weight_decay': -0.01}, b'weight_decay must be >= 0'),
                ({'lr': 0.5, 'weight_decay': 2.0}, b'lr * weight_decay must be below 1'), ({'lr': 10.0, 'weight_decay': 0.5}, b'lr * weight_decay must be below 1')]


@pytest.mark.parametrize('kw,msg', ADAM_REJECTS, ids=['-'.join('%s=%s' % kv for kv in k.items()) for k, _ in ADAM_REJECTS])
def test_adam_step_guarded_rejects_before_any_launch(lib, kw, msg):
    a = dict(ADAM_OK, **kw)
    rc = lib.hftt_adam_step_guarded(a['p'], a['g'], a['m'], a['v'], a['n'], a['step'], a['lr'], 0.9, 0.999, 1e-8, 1.0, a['weight_decay'], a['ctl'], None)
    assert rc not in (0, 2, 3)
    err = lib.hftt_last_error()
    assert err.startswith(b'adam_step_guarded: ') and msg in err, err


def test_python_entry_points_refuse_cpu_tensors(lib):
    from hftt_hip import HfttError, ops
    g, p, m, v = (torch.zeros(16) for _ in range(4))
    ctl, ws = torch.zeros(8, dtype=torch.int32), torch.zeros(2048, dtype=torch.float64)
    with pytest.raises(HfttError, match='no CPU fallback'):
        ops.grad_norm(g, ctl, ws)
    with pytest.raises(HfttError, match='no CPU fallback'):
        ops.adam_step_guarded(p, g, m, v, 1, ctl)


def _model():
    return util.build_model(util.MINI, 3)


def test_options_live_in_the_parameter_group_and_the_state_dict():
    from hftt_hip import HfttError
    from hftt_hip.trainer import FusedAdam
    opt = FusedAdam(_model().parameters(), lr=1e-3)
    g = opt.param_groups[0]
    assert g['max_grad_norm'] is None and g['guard'] is False and g['weight_decay'] == 0 and g['decoupled_weight_decay'] is False
    assert not FusedAdam._guarded(g)                                        # defaults: today's single-kernel step
    opt = FusedAdam(_model().parameters(), lr=1e-3, max_grad_norm=1.0, guard=True, weight_decay=0.01)
    g = opt.param_groups[0]
    assert g['max_grad_norm'] == 1.0 and g['guard'] is True and g['weight_decay'] == 0.01 and g['decoupled_weight_decay'] is True
    for kw in (dict(guard=True), dict(max_grad_norm=0.5), dict(weight_decay=0.01)):
        assert FusedAdam._guarded(FusedAdam(_model().parameters(), **kw).param_groups[0]), kw
    sd = opt.state_dict()
    assert sd['hftt_guard'] == {'skipped': 0, 'clipped': 0} and sd['param_groups'][0]['max_grad_norm'] == 1.0
    assert opt.skipped_steps == 0 and opt.clipped_steps == 0               # (no engine yet: nothing to read)
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt)                 # still a real torch Optimizer
    assert sched.optimizer is opt
    for kw in (dict(max_grad_norm=0.0), dict(max_grad_norm=-1.0), dict(max_grad_norm=math.nan), dict(weight_decay=-0.1), dict(weight_decay=math.nan)):
        with pytest.raises(HfttError):
            FusedAdam(_model().parameters(), **kw)


def test_load_state_dict_on_the_cpu():
    from hftt_hip import HfttError
    from hftt_hip.trainer import FusedAdam
    model = _model()
    # an old state: no hftt_guard key, a parameter group without the new options (what a checkpoint of the parent commit or the reference's
    # .dat holds)
    old = torch.optim.Adam(model.parameters(), lr=2e-4).state_dict()
    assert 'hftt_guard' not in old and 'max_grad_norm' not in old['param_groups'][0]
    opt = FusedAdam(model.parameters(), lr=1e-3, max_grad_norm=2.0)
    opt.load_state_dict(old)
    g = opt.param_groups[0]
    assert g['lr'] == 2e-4 and g['max_grad_norm'] == 2.0 and g['guard'] is False          # the options it was built with survive
    assert opt.state_dict()['hftt_guard'] == {'skipped': 0, 'clipped': 0}
    # the counters and the decoupled decay travel
    src = FusedAdam(model.parameters(), lr=1e-3, weight_decay=0.01, guard=True)
    sd = src.state_dict()
    sd['hftt_guard'] = {'skipped': 3, 'clipped': 41}
    dst = FusedAdam(model.parameters(), lr=5e-4)
    dst.load_state_dict(sd)
    g = dst.param_groups[0]
    assert g['weight_decay'] == 0.01 and g['decoupled_weight_decay'] is True and g['guard'] is True and g['lr'] == 1e-3
    assert (dst.skipped_steps, dst.clipped_steps) == (3, 41) and dst.state_dict()['hftt_guard'] == {'skipped': 3, 'clipped': 41}
    assert FusedAdam._guarded(g)
    # torch.optim.AdamW's own state is the decoupled form when it says so
    adamw = torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=0.05).state_dict()
    adamw['param_groups'][0]['decoupled_weight_decay'] = True
    dst = FusedAdam(model.parameters())
    dst.load_state_dict(adamw)
    assert dst.param_groups[0]['weight_decay'] == 0.05
    # what the kernels do not do is still refused, with the existing message
    for kw in (dict(weight_decay=0.01), dict(amsgrad=True), dict(maximize=True)):
        bad = torch.optim.Adam(model.parameters(), lr=1e-3, **kw).state_dict()
        bad['param_groups'][0]['decoupled_weight_decay'] = False
        with pytest.raises(HfttError, match='which the fused Adam kernel does not do'):
            FusedAdam(model.parameters()).load_state_dict(bad)
