"""python scripts/input_forms_parity.py [--out FILE] (on the GPU) writes profiles/input_forms_parity.txt: every run of
tests/test_gpu_input_forms.py at three data seeds (the test's own and two more: batch and d_x0) - the kernels that ran, asserted against
the test's restatement of the dispatch, the 1e-3 gate, and per tensor d_hip = max|hip - f64|, d_32 = max|f32 oracle - f64|, s and the
ratio d_hip / max(d_32, 2^-23 s), the quantity the test's M constants bound; one line per (run, tensor, seed), closed by the worst
ratio per class of case.  python scripts/input_forms_parity.py --summary FILE prints those closing lines from a table's own rows (no
GPU needed)."""
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import test_gpu_input_forms as t      # noqa: E402

SEEDS = 3
HEAD = '# class | run | seed | seconds | tensor | d_hip | d_32 | s | ratio'


def measure(out, cls, sp):
    for k in range(SEEDS):
        t0 = time.time()
        blk = t.make_block(dict(sp, seed=sp['seed'] + 1000 * k))
        rows = t.run_input(blk, xseed=9 + 10 * k)
        sec = time.time() - t0
        for name, d_hip, d_32, s, ratio in rows:
            print('%-8s|%s|%d|%.1f|%s|%.3e|%.3e|%.3e|%.2f' % (cls, t._id(sp), k, sec, name.replace('grad ', ''), d_hip, d_32, s, ratio), file=out, flush=True)


def summary(lines, out=sys.stdout):
    """per class of case: the worst row, the worst at the test's own data (seed 0), M by the rule (twice the worst ratio, rounded up to
    a power of two) beside the cap and the test's constant, and the slowest run"""
    by = {}
    for ln in lines:
        f = [c.strip() for c in ln.split('|')]
        if len(f) == 9 and not ln.startswith('#'):
            by.setdefault(f[0], []).append((float(f[8]), int(f[2]), float(f[3]), f))
    for cls in t.M:
        if cls in by:
            w = max(by[cls])
            f = w[3]
            print('# class %-8s: worst ratio %.2f (%s seed %s, %s, d_hip %s against d_32 %s; seed 0, the test\'s own data: %.2f) -> twice that, rounded '
                  'up to a power of two: %g; cap %g; the test has M = %g; slowest run %.1f s'
                  % (cls, w[0], f[1], f[2], f[4], f[5], f[6], max(r[0] for r in by[cls] if r[1] == 0), 2.0 ** math.ceil(math.log2(2.0 * w[0])),
                     t.CAP, t.M[cls], max(r[2] for r in by[cls])), file=out)


def main(path):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    failed = []
    with open(path, 'w') as out:
        print(HEAD, file=out, flush=True)
        for cls, sp in t.IN_RUNS:
            try:
                measure(out, cls, sp)
            except AssertionError as e:      # the launched symbols or the 1e-3 gate: reported, the other runs still go
                failed.append((cls, t._id(sp)))
                print('# FAILED %s %s: %s' % (cls, t._id(sp), str(e)[:3000]), file=out, flush=True)
    with open(path) as f:
        lines = f.read().splitlines()
    with open(path, 'a') as out:
        summary(lines, out)
    summary(lines)
    assert not failed, failed


if __name__ == '__main__':
    if '--summary' in sys.argv:
        summary(open(sys.argv[-1]).read().splitlines())
    else:
        main(sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else os.path.join(ROOT, 'profiles', 'input_forms_parity.txt'))
