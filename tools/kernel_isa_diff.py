#!/usr/bin/env python
"""Compare the gfx950 code of every kernel in two sets of HIP sources, kernel by kernel.

    python tools/kernel_isa_diff.py --old OLD/csrc/gemm.hip --new csrc/gemm*.hip ... [-- -DFLAG ...]

Each source is compiled with the project's CFLAGS (forwardtacotron_amd.build) plus
`--cuda-device-only -S` and whatever follows `--`; a path that ends in `.s` is read as is.
The assembly is cut at its kernel labels; a kernel is keyed by its demangled name without the
namespace prefixes, its label numbering and symbol names normalised.  Two kernels are identical
when their whole instruction text and their .amdhsa_ resource directives are equal.  Prints one
line per kernel and a verdict; exit status 1 when a kernel is missing, extra or different.
No GPU needed.
"""
from __future__ import annotations

import argparse
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from forwardtacotron_amd import build  # noqa: E402

CXXFILT = Path(build.HIPCC).resolve().parent.parent / 'lib' / 'llvm' / 'bin' / 'llvm-cxxfilt'
NAMESPACES = ('(anonymous namespace)::', 'ftmi_gemm::')
MANGLED_NAMESPACES = ('12_GLOBAL__N_1', '9ftmi_gemm')  # the same prefixes in a name left mangled


def assembly(path: Path, flags, tmp: Path) -> str:
    if path.suffix == '.s':
        return path.read_text()
    out = tmp / (f'{abs(hash(str(path.resolve())))}_{path.stem}.s')
    cmd = [build.HIPCC, *build.CFLAGS, *flags, '--cuda-device-only', '-S', str(path), '-o', str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(f'hipcc failed for {path}:\n{r.stderr}')
    return out.read_text()


def demangle(names):
    names = sorted(names)
    if not names:
        return {}
    exe = str(CXXFILT) if CXXFILT.exists() else 'c++filt'
    out = subprocess.run([exe], input='\n'.join(names), capture_output=True, text=True,
                         check=True).stdout.split('\n')
    table = {}
    for m, d in zip(names, out):
        for ns in NAMESPACES + (MANGLED_NAMESPACES if d == m else ()):  # d == m: not demangled
            d = d.replace(ns, '')
        table[m] = d
    return table


def kernels(text: str):
    """{name: (instruction lines, resource directives)} of one assembly file."""
    names = demangle(set(re.findall(r'\b_Z\w+', text)))
    entry = set(re.findall(r'^\s*\.amdhsa_kernel\s+(\S+)', text, re.M))
    lines = text.split('\n')
    found = {}
    i = 0
    while i < len(lines):
        m = re.match(r'^(\w+):', lines[i])
        if not (m and m.group(1) in entry):
            i += 1
            continue
        sym, body, res = m.group(1), [], []
        i += 1
        while i < len(lines) and not lines[i].startswith('.Lfunc_end'):
            s = lines[i].split(';')[0].strip()
            i += 1
            if not s:
                continue
            s = re.sub(r'\.LBB\d+_', '.LBB_', s)
            s = re.sub(r'\b_Z\w+', lambda q: names.get(q.group(0), q.group(0)), s)
            s = re.sub(r'\s+', ' ', s)
            if s.startswith('.amdhsa_') or s == '.end_amdhsa_kernel':
                res.append(s)
            elif not s.startswith(('.section', '.p2align', '.text')):
                body.append(s)
        found[names.get(sym, sym)] = (body, res)
    return found


def directive(res, key):
    for s in res:
        if s.startswith(key + ' '):
            return s.split()[-1]
    return '-'


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument('--old', nargs='+', required=True, type=Path)
    ap.add_argument('--new', nargs='+', required=True, type=Path)
    ap.add_argument('flags', nargs='*', help='extra compile flags, after --')
    a = ap.parse_args()
    sides = []
    with tempfile.TemporaryDirectory() as tmp:
        with ThreadPoolExecutor(max_workers=8) as ex:
            texts = dict(zip(a.old + a.new,
                             ex.map(lambda p: assembly(p, a.flags, Path(tmp)), a.old + a.new)))
        for paths in (a.old, a.new):
            side = {}
            for p in paths:
                for k, v in kernels(texts[p]).items():
                    if k in side:
                        raise SystemExit(f'kernel defined twice: {k}')
                    side[k] = v
            sides.append(side)
    old, new = sides
    bad = 0
    print(f'# flags: {" ".join(a.flags) or "(default)"}')
    print('# verdict    instr  vgpr  sgpr    lds  scratch  accum  kernel')
    for k in sorted(set(old) | set(new)):
        if k not in new or k not in old:
            verdict = 'MISSING' if k not in new else 'EXTRA'
        else:
            verdict = 'identical' if old[k] == new[k] else 'DIFFERS'
        bad += verdict != 'identical'
        body, res = new.get(k) or old[k]
        print(f'{verdict:<10} {len(body):>6} {directive(res, ".amdhsa_next_free_vgpr"):>5} '
              f'{directive(res, ".amdhsa_next_free_sgpr"):>5} '
              f'{directive(res, ".amdhsa_group_segment_fixed_size"):>6} '
              f'{directive(res, ".amdhsa_private_segment_fixed_size"):>8} '
              f'{directive(res, ".amdhsa_accum_offset"):>6}  {k}')
    same = sum(1 for k in old if k in new and old[k] == new[k])
    print(f'# {same} of {len(old)} kernels present and identical; '
          f'{len(new)} kernels in the new sources; {bad} missing, extra or different')
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
