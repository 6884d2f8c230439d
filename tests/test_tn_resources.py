"""Registers, scratch and occupancy of csrc/gemm_tn.hip from the compiler's own remarks (no GPU): the five forms of the paper-size step and
their reference twins (kernel form 100 + npass: the reference step schedule, HFTT_TN_PIPE=0) stay free of scratch at two waves per SIMD, and
no form of the file spills more than it did before the pipelined schedules."""
import re

import pytest

from hipcc_remarks import get, resources

# (TM, TN, npass, dY bf16, X bf16) of the main kernel at the paper-size x3 step
PAPER_FORMS = ['2, 4, 4, false, false', '1, 4, 6, false, false', '2, 4, 6, false, true', '2, 4, 4, true, false', '1, 4, 4, false, false']
# forms that spilled before (bytes per lane), none of them in the paper step; every other form had none
SCRATCH_BEFORE = {'2, 4, 3, false, false': 76, '2, 4, 6, false, false': 20, '2, 4, 1, true, false': 32}


def _kernels():
    res = {k: v for k, v in resources('gemm_tn.hip').items() if k.startswith('gemm_tn_kernel<')}
    assert len(res) >= 40, sorted(res)
    return {re.sub(r'^gemm_tn_kernel<|>$', '', k): v for k, v in res.items()}


def _twin(form):
    tm, tn, npass, rest = form.split(', ', 3)
    return '%s, %s, %d, %s' % (tm, tn, 100 + int(npass), rest)


# the paper forms that run the split loop, each with a reference twin; the masked 256 x 256 form with a bf16 X keeps the reference loop
SPLIT_FORMS = [f for f in PAPER_FORMS if f != '2, 4, 6, false, true']


@pytest.mark.parametrize('form', PAPER_FORMS)
def test_paper_forms_and_their_reference_twins(form):
    res = _kernels()
    assert (_twin(form) in res) == (form in SPLIT_FORMS), form
    for name in (form, _twin(form)) if form in SPLIT_FORMS else (form,):
        v = res[name]
        assert get(v, 'ScratchSize') == 0, (name, v)
        assert get(v, 'VGPRs') + get(v, 'AGPRs') <= 256, (name, v)
        assert get(v, 'Occupancy') >= 2, (name, v)


def test_no_form_spills_more_than_before():
    for name, v in _kernels().items():
        tm, tn, form, rest = name.split(', ', 3)
        base = '%s, %s, %d, %s' % (tm, tn, int(form) % 100, rest)      # a reference twin is held to its form's figure
        assert get(v, 'ScratchSize') <= SCRATCH_BEFORE.get(base, 0), (name, v)
