#!/usr/bin/env python
"""Kernel-by-kernel comparison of the device code of two builds of the library (CPU only).

    python -m hual_amd.build --out A/parent.so     # at the parent commit
    python -m hual_amd.build --out B/this.so       # at this commit
    python scripts/isa_diff.py A/parent.so.obj B/this.so.obj [--show KERNEL] [--pair 'NAME_IN_A=NAME_IN_B' ...]

For every kernel symbol of every device object: the instruction count of each side and whether the instruction streams are equal once
the addresses, the encodings and the symbols of branch targets (objdump's trailing comment) are taken off; every operand, literal
constants included, is compared.  --show prints a unified diff of one kernel's stream.  Kernels are paired by demangled name; --pair
(repeatable) pairs a kernel that was renamed: the one kernel of A whose name holds the first substring with the one kernel of B, in the
same object file, whose name holds the second, e.g. --pair 'AlScoreMcArgs=AlSource)1>'.  The script names no instruction and searches
for nothing: it only diffs.
"""
import difflib
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get('HUAL_LLVM_BIN', '/opt/rocm/lib/llvm/bin')


def code_objects(obj, tmp):
    o = os.path.join(tmp, os.path.basename(obj))
    shutil.copy(obj, o)
    subprocess.run([os.path.join(LLVM, 'llvm-objdump'), '--offloading', o], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=True)
    return sorted(f for f in glob.glob(o + '.*') if 'amdgcn' in f)


def normalise(line):
    """the instruction text alone: the address and the encoding ride in the trailing comment, and so does the symbol + offset that
    objdump resolves a branch to (the operand itself is a relative offset).  Literal operands stay as they are"""
    return line.split('//')[0].strip()


def kernels_of(obj_dir):
    """{(object file, demangled kernel): normalised stream}"""
    res = {}
    tmp = tempfile.mkdtemp(prefix='hual_isa_')
    try:
        for obj in sorted(glob.glob(os.path.join(obj_dir, '*.hip.o'))):
            for co in code_objects(obj, tmp):
                dis = subprocess.run([os.path.join(LLVM, 'llvm-objdump'), '-d', '-C', co], stdout=subprocess.PIPE, check=True).stdout.decode()
                cur, streams = None, {}
                for l in dis.splitlines():
                    m = re.match(r'^[0-9a-f]+ <(.+)>:$', l)
                    if m:
                        cur = m.group(1)
                        streams[cur] = []
                    elif cur is not None and l.startswith('\t'):
                        streams[cur].append(normalise(l))
                for k, st in streams.items():
                    res[(os.path.basename(obj), k)] = st
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return res


def rename(a, b, pair):
    """the kernel of B that `pair` = 'x=y' names by y takes the key of the kernel of A named by x, shown as 'A name => B name'"""
    x, y = pair.split('=', 1)
    ka, kb = [k for k in a if x in k[1]], [k for k in b if y in k[1]]
    if len(ka) != 1 or len(kb) != 1 or ka[0][0] != kb[0][0]:
        sys.exit('--pair %s: needs one kernel of A and one of B in the same object file, found %s and %s' % (pair, ka, kb))
    key = (ka[0][0], '%s => %s' % (ka[0][1], kb[0][1]))
    a[key], b[key] = a.pop(ka[0]), b.pop(kb[0])


def main():
    argv = sys.argv[1:]
    opts = {'--show': [], '--pair': []}
    args = []
    while argv:
        x = argv.pop(0)
        if x in opts:
            opts[x].append(argv.pop(0))
        else:
            args.append(x)
    show = opts['--show'][-1] if opts['--show'] else None
    a, b = kernels_of(args[0]), kernels_of(args[1])
    for pair in opts['--pair']:
        rename(a, b, pair)
    ndiff = 0
    print('%-16s %8s %8s  %-9s %s' % ('object', 'insns A', 'insns B', 'stream', 'kernel'))
    for key in sorted(set(a) | set(b)):
        sa, sb = a.get(key, []), b.get(key, [])
        same = key in a and key in b and sa == sb
        ndiff += not same
        print('%-16s %8d %8d  %-9s %s' % (key[0], len(sa), len(sb), 'equal' if same else 'DIFFERENT', key[1]))
        if not same:
            if show is not None and show in key[1]:
                print('\n'.join(difflib.unified_diff(sa, sb, 'A', 'B', lineterm='', n=2)))
    print('%d kernels, %d with a different stream' % (len(set(a) | set(b)), ndiff))
    return 0


if __name__ == '__main__':
    sys.exit(main())
