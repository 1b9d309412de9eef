"""python scripts/cq_forms_parity.py > TABLE (on the GPU); python scripts/cq_forms_parity.py --summary TABLE: its closing lines (no GPU needed);
both together are profiles/cq_forms_parity.txt.  Every case of tests/test_gpu_cq_forms.py at three data seeds (the
test's own and two more: batch and activations) - the form that ran, and per tensor max|hip - f64|, max|f32 oracle - f64| and their
ratio d_hip / max(d_32, 2^-23 s), the quantity the test's M constants bound.  The shapes under HUAL_CQ_NO_WIDE=1 run in a child process."""
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import test_gpu_cq_forms as t      # noqa: E402
from test_gpu_blocks import Block      # noqa: E402

SEEDS = 3
CAP = {'f16': 16.0, 'f32': 4.0}      # the most M may be, whatever is measured: 22-bit operands are 4 float32 rounding units, x 4 for lost subnormal
                                    # residuals; the float32 forms differ from the oracle in summation order only
FMT = '%-7s|%-12s|B%d T%d L%d|drop %.1f|%-52s|d_hip %.3e|d_32 %.3e|ratio %s|max %6.2f'


def measure(label, make):
    """make(k) -> the block of data seed k; one line per (dropout, tensor): d_hip and d_32 at the seed of the largest ratio, the ratio at each seed"""
    res = {}
    for k in range(SEEDS):
        blk = make(k)
        for drop in (0.2, 0.0):
            x, dy, feats, dx, got = t._launch(blk, drop, xseed=5 + 10 * k)
            form = t._form_of(blk, got)
            for name, d_hip, d_32, s, ratio in t._floor_rows(blk, x, dy, feats, dx, drop):
                res.setdefault((form, drop, name), []).append((ratio, d_hip, d_32))
    for (form, drop, name), v in res.items():
        w = max(v)
        print(FMT % (form, label, blk.B, blk.T, blk.L, drop, name, w[1], w[2], ' '.join('%6.2f' % r[0] for r in v), w[0]), flush=True)


def summary(lines):
    """per form: the worst line; per class of form: the worst ratio, M by the rule (twice the worst ratio, rounded up to a power of two) and the
    seed-to-seed spread (a line's largest ratio / its smallest)"""
    by, spread = {}, {}
    for ln in lines:
        f = [c.strip() for c in ln.split('|')]
        if len(f) != 9:
            continue
        ratios = [float(v) for v in f[7].split()[1:]]
        by.setdefault(f[0], []).append((max(ratios), ln))
        spread.setdefault(t.FORMS[f[0]][3], []).append(max(ratios) / max(min(ratios), 1e-30))
    print('# the worst line of each form')
    for form, v in by.items():
        print('# ' + max(v)[1] + '   (of %d lines)' % len(v))
    for cls in ('f16', 'f32'):
        w = max(max(v)[0] for f, v in by.items() if t.FORMS[f][3] == cls)
        w0 = max(float(ln.split('|')[7].split()[1]) for f, v in by.items() if t.FORMS[f][3] == cls for _, ln in v)
        print('# class %s: worst ratio %.2f (seed 0, the test\'s own data: %.2f) -> twice that, rounded up to a power of two: %g; cap %g; the test has M = %g.  '
              'Over the three seeds a line\'s largest / smallest ratio is at most %.2f, median %.2f'
              % (cls, w, w0, 2.0 ** math.ceil(math.log2(2.0 * w)), CAP[cls], t.M[cls], max(spread[cls]), statistics.median(spread[cls])))


def main():
    if '--no-wide' in sys.argv:
        for shape in t.NO_WIDE_SHAPES:
            measure('no wide', lambda k: Block(**dict(shape, seed=shape['seed'] + 1000 * k)))
        return
    print('# form | case | shape | dropout | tensor | d_hip, d_32 at the seed of the largest ratio | ratio at seeds 0 1 2 | largest', flush=True)
    for form, shape in t.CASES:
        measure('', lambda k: Block(**dict(shape, seed=shape['seed'] + 1000 * k)))
    for form, T, L in t.MASK_CASES:
        measure('mask paths', lambda k: t._mask_block(T, L, seed=71 + 1000 * k))


if __name__ == '__main__':
    if '--summary' in sys.argv:          # ... --summary FILE: the table's closing lines from its own rows
        summary(open(sys.argv[-1]).read().splitlines())
    elif '--no-wide' in sys.argv:
        main()
    else:
        main()
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--no-wide'], env=dict(os.environ, HUAL_CQ_NO_WIDE='1'))
        assert r.returncode == 0
