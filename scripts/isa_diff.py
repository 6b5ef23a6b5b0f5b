#!/usr/bin/env python
"""Device-ISA identity check for kernel experiments and refactors: compile .hip files of two source trees (git revisions,
or directories holding a tree) to gfx950 assembly and compare every kernel's instruction stream (labels and comments
normalised).  Used to prove that an experimental template variant behind a default-off switch, or a move of kernels
between files, leaves the kernels' code untouched, so it can be committed without a GPU run.

    python scripts/isa_diff.py <rev_a> <rev_b> [file.hip ...] [--b file.hip ...] [--rename old=new ...] [--work dir]
    e.g.  isa_diff.py HEAD~1 HEAD                                   (the default files: the cluster recurrence family)
          isa_diff.py HEAD~1 . csrc/gemm.hip --b csrc/gemm.hip csrc/conv.hip --rename conv3x5_nt_kernel=conv_nt_kernel
          isa_diff.py HEAD~1 . --rename 'lstm_bwd_cluster_f32s_kernel<([^>]*)>=lstm_bwd_cluster_f32_kernel<\1, OpSplit3>'
(file paths from the repository root).  Every file is compiled with the flags that build.py OF ITS OWN TREE gives it -- FLAGS
and the file's FILE_FLAGS entry, ASR_BUILD_ABLATE=1 in the environment included -- so a file that exists only on side b
takes tree b's flags and the verdict is about the code each tree ships.
Kernels are matched by demangled name over ALL files of a side (they may move between files), with
`(anonymous namespace)::` dropped and the --rename substitutions (re.sub) applied to side a's names.  Template arguments appended
with a default (kernel<256, false> -> kernel<256, false, false>) are matched by trying the old name with `, false` appended
to the argument list.  --work keeps the trees and their assembly in a directory (and reuses what is there).  Kernels that differ are listed with their registers, scratch and LDS on both sides."""
import os
import re
import runpy
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = 'tensorflow_end2end_speech_recognition_amd/csrc/'
DEFAULT = [CSRC + f for f in ('lstm_cluster.hip', 'lstm_cluster_f32.hip', 'gru_cluster.hip', 'cluster_host.hip')]
CXXFILT = 'c++filt'
RES = ('.vgpr_count', '.agpr_count', '.sgpr_count', '.private_segment_fixed_size', '.group_segment_fixed_size')


def build_flags(tree, rel):
    """What build.py of the SAME tree compiles `rel` with (FLAGS + its FILE_FLAGS entry, ASR_BUILD_ABLATE included), so that
    the verdict is about the code that ships; only the switches that stop at device assembly are added."""
    build = runpy.run_path(os.path.join(tree, os.path.dirname(os.path.dirname(rel)), 'build.py'))
    return build['FLAGS'] + build['FILE_FLAGS'].get(os.path.basename(rel), []) + ['--cuda-device-only', '-S']


def asm_of(rev, rels, tmp, tag):
    """{mangled kernel name: (body, resources)} over the files `rels` of revision (or directory) `rev`."""
    tree = os.path.join(tmp, tag)
    fresh = not os.path.isdir(tree)
    os.makedirs(tree, exist_ok=True)
    dirs = sorted({'include'} | {os.path.dirname(r) for r in rels} |
                  {os.path.join(os.path.dirname(os.path.dirname(r)), 'build.py') for r in rels})
    if not fresh:
        pass
    elif os.path.isdir(rev):
        for d in dirs:
            subprocess.run(['cp', '-r', '--parents', d, tree], cwd=os.path.abspath(rev), check=True)
    else:
        subprocess.run('git -C %s archive %s %s | tar -x -C %s' % (ROOT, rev, ' '.join(dirs), tree), shell=True, check=True)
    fns = {}
    for i, rel in enumerate(rels):
        out = os.path.join(tree, 'out%d.s' % i)
        if not os.path.exists(out):
            subprocess.run(['/opt/rocm/bin/hipcc'] + build_flags(tree, rel) + ['-I', os.path.join(tree, 'include'), '-o', out,
                                                                               os.path.join(tree, rel)], check=True, capture_output=True)
        txt = open(out).read()
        res = resources(txt)
        for name, body in functions(txt).items():
            fns[name] = (body, res.get(name, {}))
    return fns


def functions(txt):
    parts = re.split(r'\n\t\.(?:globl|protected|weak)\t(\S+)\s*; -- Begin function \S+\n', txt)   # (comdat templates: .protected)
    return {parts[i]: parts[i + 1][:parts[i + 1].find('; -- End function')] for i in range(1, len(parts), 2)}


def resources(txt):
    """{kernel: {field: value}} from the .amdgpu_metadata note."""
    out = {}
    for entry in re.split(r'\n  - \.agpr_count:', txt[txt.find('amdhsa.kernels:'):])[1:]:
        entry = '    .agpr_count:' + entry
        name = re.search(r'\n\s+\.name:\s+(\S+)', entry)
        if name:
            out[name.group(1)] = {k: int(m.group(1)) for k in RES for m in [re.search(r'%s:\s+(\d+)' % re.escape(k), entry)] if m}
    return out


def normalise(body, name):
    b = body.replace(name, 'FN')
    b = re.sub(r'\.Lfunc_end\d+', '.Lfunc_end', b)
    b = re.sub(r'\.LBB\d+_', '.LBB_', b)
    b = re.sub(r';.*', '', b)
    # (symbol binding is not code: a template kernel moved into an anonymous namespace loses its .globl / .weak line)
    return [line.rstrip() for line in b.splitlines() if line.strip() and not re.match(r'\s*\.(globl|weak|protected|hidden)\s', line)]


def demangled(names, renames=()):
    """{readable name: mangled name}"""
    if not names:
        return {}
    names = list(names)
    out = subprocess.run([CXXFILT], input='\n'.join(names), capture_output=True, text=True, check=True).stdout.split('\n')
    table = {}
    for mangled, d in zip(names, out):
        d = re.sub(r'^void ', '', d.replace('(anonymous namespace)::', '').replace('> >', '>>').replace('> >', '>>'))
        for old, new in renames:
            d = re.sub(old, new, d)
        table[d] = mangled
    return table


def main():
    args = sys.argv[1:]
    if len(args) < 2:
        sys.exit(__doc__)
    rev_a, rev_b, files_a, files_b, renames, work = args[0], args[1], [], None, [], []
    dest = files_a
    for a in args[2:]:
        if a == '--b':
            files_b = dest = []
        elif a == '--rename':
            dest = renames
        elif a == '--work':
            dest = work
        else:
            dest.append(a)
    files_a = files_a or DEFAULT
    files_b = files_b or files_a
    renames = [tuple(r.split('=', 1)) for r in renames]
    with tempfile.TemporaryDirectory() as tmp:
        tmp = work[0] if work else tmp
        a, b = asm_of(rev_a, files_a, tmp, 'a'), asm_of(rev_b, files_b, tmp, 'b')
    da, db = demangled(a, renames), demangled(b)
    same = True
    matched = set()
    for name in sorted(da):
        other = name if name in db else re.sub(r'>\(', ', false>(', name, count=1)
        if other not in db:
            print('MISSING   %s' % name[:160])
            same = False
            continue
        matched.add(other)
        (body_a, res_a), (body_b, res_b) = a[da[name]], b[db[other]]
        ok = normalise(body_a, da[name]) == normalise(body_b, db[other])
        same &= ok
        print('%s %s' % ('IDENTICAL' if ok else 'DIFFERENT', name[:160]))
        if not ok:
            print('            ' + '  '.join('%s %s -> %s' % (k[1:], res_a.get(k), res_b.get(k)) for k in RES))
    for name in sorted(db):
        if name not in matched:
            print('NEW       %s' % name[:160])
    print('kernels unchanged' if same else 'KERNELS CHANGED')
    return 0 if same else 1


if __name__ == '__main__':
    sys.exit(main())
