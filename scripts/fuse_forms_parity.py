"""python scripts/fuse_forms_parity.py [--out FILE] (on the GPU) writes profiles/fuse_forms_parity.txt: every case of
tests/test_gpu_fuse_forms.py at three data seeds (the test's own and two more: masks, labels, cq.feats, d outputs, loc_part; logits and
soft labels of the localizing cases) - the kernels that ran, asserted against the test's restatement of the dispatch, the 1e-3 gate, and
per tensor d_hip = max|hip - f64|, d_32 = max|f32 oracle - f64|, s and the ratio d_hip / max(d_32, 2^-23 s), the quantity the test's M
constants bound; one line per (case, tensor, seed), closed by the worst ratio per class of case.  python scripts/fuse_forms_parity.py
--summary FILE prints those closing lines from a table's own rows (no GPU needed)."""
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import test_gpu_fuse_forms as t      # noqa: E402

SEEDS = 3
HEAD = '# class | case | seed | seconds | tensor | d_hip | d_32 | s | ratio'


def _emit(out, cls, name, k, sec, rows):
    for tensor, d_hip, d_32, s, ratio in rows:
        print('%-6s|%s|%d|%.1f|%s|%.3e|%.3e|%.3e|%.2f' % (cls, name, k, sec, tensor.replace('grad ', ''), d_hip, d_32, s, ratio), file=out, flush=True)


def measure(out, cls, sp):
    for k in range(SEEDS):
        t0 = time.time()
        rows, _ = t.run_fuse(t.make_block(dict(sp, seed=sp['seed'] + 1000 * k)), xseed=9 + 10 * k)
        _emit(out, cls, t._id(sp), k, time.time() - t0, rows)


def measure_loc(out, T):
    for k in range(SEEDS):
        t0 = time.time()
        rows = t.run_loc(T, seed=31 + 100 * k)
        _emit(out, 'loc', 'B%d_T%d' % (t.LOC_B, T), k, time.time() - t0, rows)


def summary(lines, out=sys.stdout):
    """per class of case: the worst row, the worst at the test's own data (seed 0), M by the rule (twice the worst ratio, rounded up to
    a power of two) beside the cap and the test's constant, and the slowest case"""
    by = {}
    for ln in lines:
        f = [c.strip() for c in ln.split('|')]
        if len(f) == 9 and not ln.startswith('#'):
            by.setdefault(f[0], []).append((float(f[8]), int(f[2]), float(f[3]), f))
    for cls in t.M:
        if cls in by:
            w = max(by[cls])
            f = w[3]
            rule = 2.0 ** math.ceil(math.log2(2.0 * w[0])) if w[0] > 0 else 1.0
            print('# class %-6s: worst ratio %.2f (%s seed %s, %s, d_hip %s against d_32 %s, s %s; seed 0, the test\'s own data: %.2f) -> twice that, '
                  'rounded up to a power of two: %g; cap %g; the test has M = %g; slowest case %.1f s'
                  % (cls, w[0], f[1], f[2], f[4], f[5], f[6], f[7], max(r[0] for r in by[cls] if r[1] == 0), rule, t.CAP, t.M[cls],
                     max(r[2] for r in by[cls])), file=out)


def main(path):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    failed = []
    with open(path, 'w') as out:
        print(HEAD, file=out, flush=True)
        for cls, sp in t.FUSE_CASES:
            try:
                measure(out, cls, sp)
            except AssertionError as e:      # the launched symbols or the 1e-3 gate: reported, the other cases still go
                failed.append((cls, t._id(sp)))
                print('# FAILED %s %s: %s' % (cls, t._id(sp), str(e)[:3000]), file=out, flush=True)
        for T in t.LOC_T:
            try:
                measure_loc(out, T)
            except AssertionError as e:
                failed.append(('loc', T))
                print('# FAILED loc T%d: %s' % (T, str(e)[:3000]), file=out, flush=True)
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
        main(sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else os.path.join(ROOT, 'profiles', 'fuse_forms_parity.txt'))
