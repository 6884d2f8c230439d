"""The compiler's own resource remarks of one source file of csrc/ (hipcc cross-compiles without a GPU), for the tests that pin registers,
scratch, LDS and occupancy: one compile per source file and test session."""
import functools
import os
import re
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'nylon-amt_amd', 'csrc')
HIPCC = '/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else shutil.which('hipcc')


@functools.lru_cache(maxsize=None)
def resources(src):
    """{demangled kernel name, without namespace, return type and arguments: {remark: value}} in the order of the file"""
    if HIPCC is None:
        pytest.skip('hipcc not found')
    out = subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-fPIC', '-std=c++17', '-Wno-unused-result', '-x', 'hip', '-c', os.path.join(CSRC, src),
                          '-o', '/dev/null', '-Rpass-analysis=kernel-resource-usage'], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    rows, cur = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r'Function Name: (\S+)', line)
        if m:
            cur = m.group(1); rows[cur] = {}
            continue
        m = re.search(r'remark:\s+([A-Za-z ]+(?:\[[^\]]*\])?): (\d+)', line)
        if m and cur:
            rows[cur][m.group(1).strip()] = int(m.group(2))
    names = subprocess.run(['c++filt'], input='\n'.join(rows), capture_output=True, text=True).stdout.splitlines()
    return {re.sub(r'\(anonymous namespace\)::|void |\(.*$', '', n): v for n, v in zip(names, rows.values())}


def get(v, key):
    """the remark named `key`, or the first whose name starts with it ('ScratchSize' for 'ScratchSize [bytes/lane]')"""
    if key in v:
        return v[key]
    for k, x in v.items():
        if k.startswith(key):
            return x
    raise KeyError(key)
