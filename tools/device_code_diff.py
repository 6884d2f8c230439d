#!/usr/bin/env python3
"""Is the device code of this tree the same as at another commit?  The check for a host-side change (launchers, validation, the C ABI plumbing).

    python tools/device_code_diff.py [--base REV] [--grad-hi] [--jobs N]

Exports REV (default HEAD) next to the working tree, compiles every HIP source of each side's own build.py SOURCES with this tree's FLAGS, device
side only (`--cuda-device-only --no-gpu-bundle-output`: one gfx950 code object per file), and compares per kernel symbol -- whichever file holds
it on either side (a symbol that one tree holds in several sources is matched file by file); a symbol that moved is reported with where from --
  * the instruction bytes (llvm-objdump -d), symbol by symbol, so that a changed order of instantiation does not matter, and
  * the amdhsa.kernels metadata (llvm-readelf --notes): register counts, spills, scratch, static LDS, kernarg size, workgroup size.
--grad-hi adds -DHFTT_GRAD_HI_BUILD (the HFTT_BUILD_GRAD_HI=1 library).  Exit status 0 = no difference, 1 = differences (listed).
What "0 differences" does NOT cover: constant data outside the symbols' instructions (.rodata tables, device globals), the kernel descriptors
beyond the metadata keys above, and anything on the host side (grids, LDS byte counts, argument order: bench.py --dump-outputs is the check for
those).
"""
import argparse
import hashlib
import importlib.util
import os
import re
import subprocess
import sys
import tarfile
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join('nylon-amt_amd', 'csrc')
META_KEYS = ('.vgpr_count', '.agpr_count', '.sgpr_count', '.vgpr_spill_count', '.sgpr_spill_count', '.private_segment_fixed_size',
             '.group_segment_fixed_size', '.kernarg_segment_size', '.max_flat_workgroup_size', '.uses_dynamic_stack')


def _build_py(root):
    spec = importlib.util.spec_from_file_location('hftt_build', os.path.join(root, 'nylon-amt_amd', 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _llvm(tool):
    for d in (os.environ.get('ROCM_PATH', '/opt/rocm') + '/llvm/bin', '/opt/rocm/llvm/bin'):
        if os.path.exists(os.path.join(d, tool)):
            return os.path.join(d, tool)
    return tool


def _run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError('%s failed:\n%s' % (' '.join(cmd), r.stderr[-4000:]))
    return r.stdout


def kernels_of(tree, src, flags, hipcc, out_dir):
    """{symbol: (sha256 of the instruction bytes, n_bytes, {metadata key: value})} of one source file's code object"""
    co = os.path.join(out_dir, os.path.splitext(src)[0] + '.co')
    _run([hipcc] + flags + ['-x', 'hip', '--cuda-device-only', '--no-gpu-bundle-output', '-c', os.path.join(tree, CSRC, src), '-o', co])
    code, sym = {}, None
    for line in _run([_llvm('llvm-objdump'), '-d', co]).splitlines():
        m = re.match(r'^[0-9a-f]+ <(.+)>:$', line)
        if m:
            sym = m.group(1)
            code[sym] = []
            continue
        m = re.search(r'// [0-9A-F]+: ((?:[0-9A-F]{8} ?)+)', line)
        if m and sym is not None:
            code[sym].append(m.group(1).strip())
    meta, cur = {}, None
    for line in _run([_llvm('llvm-readelf'), '--notes', co]).splitlines():
        if line.startswith('  - '):                      # a new entry of amdhsa.kernels
            cur = {}
            line = '    ' + line[4:]
        m = re.match(r'^    (\.[a-z_]+):\s+(\S+)$', line)
        if m and cur is not None:
            if m.group(1) == '.name':
                meta[m.group(2)] = cur
            elif m.group(1) in META_KEYS:
                cur[m.group(1)] = m.group(2)
    out = {}
    for name, words in code.items():
        text = ' '.join(words)
        out[name] = (hashlib.sha256(text.encode()).hexdigest(), len(text.replace(' ', '')) // 2, meta.get(name))
    for name in meta:
        if name not in out:
            out[name] = (None, 0, meta[name])
    return out


def _keyed(got, side, sources):
    """{key: (source file, kernels_of value)}: key = the symbol, or (file, symbol) for a symbol that `dup` names"""
    return {((src, name) if name in got['dup'] else name): (src, v) for src in sources for name, v in got[(side, src)].items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--base', default='HEAD')
    ap.add_argument('--grad-hi', action='store_true')
    ap.add_argument('--jobs', type=int, default=8)
    a = ap.parse_args()
    b = _build_py(ROOT)
    flags = [f for f in b.FLAGS if f != '-DHFTT_GRAD_HI_BUILD'] + (['-DHFTT_GRAD_HI_BUILD'] if a.grad_hi else [])
    with tempfile.TemporaryDirectory() as tmp:
        base = os.path.join(tmp, 'base')
        os.makedirs(base)
        tar = os.path.join(tmp, 'base.tar')
        _run(['git', '-C', ROOT, 'archive', '-o', tar, a.base, CSRC, 'include', os.path.join('nylon-amt_amd', 'build.py')])
        with tarfile.open(tar) as t:
            t.extractall(base)
        # each side compiles the sources its own build.py names: a kernel may have moved to another file, or its file may be gone
        sources = {side: [s for s in _build_py(tree).SOURCES if s.endswith('.hip')] for side, tree in (('base', base), ('tree', ROOT))}
        jobs = []
        for side, tree in (('base', base), ('tree', ROOT)):
            os.makedirs(os.path.join(tmp, 'co_' + side))
            jobs += [(side, tree, s) for s in sources[side]]
        with ThreadPoolExecutor(max_workers=a.jobs) as ex:
            res = list(ex.map(lambda j: kernels_of(j[1], j[2], flags, b._hipcc(), os.path.join(tmp, 'co_' + j[0])), jobs))
    got = {(j[0], j[2]): r for j, r in zip(jobs, res)}
    # matched by symbol across files; by (file, symbol) only where one tree holds the symbol in more than one source
    got['dup'] = {name for side in sources for name in set().union(*(got[(side, s)] for s in sources[side]))
                  if sum(name in got[(side, s)] for s in sources[side]) > 1}
    old, new = _keyed(got, 'base', sources['base']), _keyed(got, 'tree', sources['tree'])
    n_diff = n_moved = 0
    for s in sources['tree']:
        mine = {k: v for k, (src, v) in new.items() if src == s}
        bad, moved = [], {}
        for k in sorted(mine, key=str):
            name = k if isinstance(k, str) else k[1]
            if k not in old:
                bad.append('  %s: only in the working tree' % name)
                continue
            was, o = old[k]
            if was != s:
                moved.setdefault(was, []).append(name)
            if o[:2] != mine[k][:2]:
                bad.append('  %s: instruction bytes differ (%d -> %d bytes)' % (name, o[1], mine[k][1]))
            elif o[2] != mine[k][2]:
                bad.append('  %s: metadata differs: %s -> %s' % (name, o[2], mine[k][2]))
        n_diff += len(bad)
        n_moved += sum(len(v) for v in moved.values())
        print('%-18s %4d symbols %9d code bytes  %s%s' % (s, len(mine), sum(v[1] for v in mine.values()), 'identical' if not bad else '%d DIFFER' % len(bad),
                                                       ''.join('  (%d moved here from %s)' % (len(v), f) for f, v in sorted(moved.items()))))
        for line in bad:
            print(line)
    for k in sorted(set(old) - set(new), key=str):
        print('%-18s %s: only in the base' % (old[k][0], k if isinstance(k, str) else k[1]))
        n_diff += 1
    print('%s against %s%s: %d symbols, %d code bytes, %d moved to another file, %d differences' % (
        'working tree', a.base, ' (-DHFTT_GRAD_HI_BUILD)' if a.grad_hi else '', len(new), sum(v[1] for _, v in new.values()), n_moved, n_diff))
    return 1 if n_diff else 0


if __name__ == '__main__':
    sys.exit(main())
