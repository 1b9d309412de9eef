"""python scripts/da_forms_parity.py [--out FILE] (on the GPU) writes profiles/da_forms_parity.txt: every case of tests/test_gpu_da_forms.py
at three data seeds (the test's own and two more: batch and activations) - the kernels that ran, asserted against the test's restatement of
the dispatch, and per tensor the ratio d_hip / max(d_32, 2^-23 s) of max|hip - f64| to max|f32 oracle - f64|, the quantity the test's M
constants bound; one line per (case, dropout), closed by the worst ratio per class of case and per attention kernel.
python scripts/da_forms_parity.py --summary FILE prints those closing lines from a table's own rows, and
python scripts/da_forms_parity.py --table the map of DESIGN.md section 3 from the same restatement (neither needs a GPU)."""
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import test_gpu_da_forms as t      # noqa: E402

SEEDS = 3
CLASSES = ('fwd', 'chain', 'plain', 'big', 'tiles')
HEAD = '# class | attention kernels | shape | layer | dropout | s per case | largest ratio | its tensor, d_hip and d_32 | ratio at seeds 0/1/2 per tensor, in the order:'


def _short(name, layer):
    return name.replace('grad d_attn_%d/' % layer, '').replace('dual_multihead_attention/', 'mha/')      # (the layer has its own column)


def measure(out, cls, layer, shape, legend):
    """one line per dropout setting: the largest ratio with its tensor, d_hip and d_32, and every tensor's ratio at each seed"""
    res, form, t0 = {}, None, time.time()
    for k in range(SEEDS):
        blk = t.make_block(dict(shape, seed=shape['seed'] + 1000 * k))
        for drop in ((t.DROP, 0.0) if layer == 0 else (t.DROP,)):
            want, rows = t.run_case(blk, layer, drop, xseed=3 + 10 * k)
            form = t._form_name(want)
            for name, d_hip, d_32, s, ratio in rows:
                res.setdefault(drop, {}).setdefault(_short(name, layer), []).append((ratio, d_hip, d_32))
    sec = (time.time() - t0) / (SEEDS * len(res))
    for drop, v in res.items():
        if not legend:
            legend.extend(v)
            print(HEAD + ' ' + ' '.join(legend), file=out, flush=True)
        assert list(v) == legend
        w, name = max((max(r), n) for n, r in v.items())
        print('%-5s|%-33s|B%d T%d L%d|layer %d|drop %.1f|%.1f s|max %.2f|%s d_hip %.3e d_32 %.3e|%s'
              % (cls, form, blk.B, blk.T, blk.L, layer, drop, sec, w[0], name, w[1], w[2],
                 ' '.join('/'.join('%.2f' % r[0] for r in v[n]) for n in legend)), file=out, flush=True)


def summary(lines, out=sys.stdout):
    """per attention kernel and per class of case: the worst line (without its last column); per class M by the rule (twice the worst
    ratio, rounded up to a power of two, at most the cap) and the seed-to-seed spread (a tensor's largest ratio / its smallest)"""
    by, kern, spread = {}, {}, {}
    for ln in lines:
        f = [c.strip() for c in ln.split('|')]
        if len(f) != 9 or ln.startswith('#'):
            continue
        per = [[float(x) for x in c.split('/')] for c in f[8].split()]
        w, head = max(max(p) for p in per), ln[:ln.rindex('|')]
        by.setdefault(f[0], []).append((w, max(p[0] for p in per), head))
        for k in f[1].split():
            kern.setdefault(k, []).append((w, head))
        spread.setdefault(f[0], []).extend(max(p) / max(min(p), 1e-30) for p in per)
    print('# the worst line of each attention kernel', file=out)
    for k in sorted(kern):
        print('# %-18s %s   (of %d lines)' % (k, max(kern[k])[1], len(kern[k])), file=out)
    for cls in CLASSES:
        if cls not in by:
            continue
        w, w0 = max(v[0] for v in by[cls]), max(v[1] for v in by[cls])
        print('# class %-5s: worst ratio %.2f (%s; seed 0, the test\'s own data: %.2f) -> twice that, rounded up to a power of two: %g; cap %g; the '
              'test has M = %g.  Over the three seeds a tensor\'s largest / smallest ratio is at most %.2f, median %.2f'
              % (cls, w, ' '.join(max(by[cls])[2].split('|')[2:5] + max(by[cls])[2].split('|')[7:]), w0, 2.0 ** math.ceil(math.log2(2.0 * w)), t.CAP,
                 t.M[cls], max(spread[cls]), statistics.median(spread[cls])), file=out)


# ---------------------------------------------------------------------------------------------------- DESIGN.md section 3
RULES = {      # kernel -> (its region in words, the same as a predicate)
    'attn_fwd_kernel<2, 256>': ('max(T, L) <= 32 and cdiv(T, 16) + cdiv(L, 16) <= 3', lambda T, L: max(T, L) <= 32 and t._cdiv(T, 16) + t._cdiv(L, 16) <= 3),
    'attn_fwd_kernel<2, 512>': ('max(T, L) <= 32 and cdiv(T, 16) + cdiv(L, 16) = 4', lambda T, L: max(T, L) <= 32 and t._cdiv(T, 16) + t._cdiv(L, 16) == 4),
    'attn_fwd_kernel<4, 512>': ('33 <= max(T, L) <= 64', lambda T, L: 33 <= max(T, L) <= 64),
    'attn_fwd_kernel<8, 512>': ('65 <= max(T, L) <= 128', lambda T, L: 65 <= max(T, L) <= 128),
    'attn_fwd_kernel<16, 512>': ('129 <= max(T, L) <= 256', lambda T, L: 129 <= max(T, L) <= 256),
    'attn_bwd_chain_kernel': ('L <= 32 and T <= 128', lambda T, L: L <= 32 and T <= 128),
    'attn_bwd_big_kernel': ('max(T, L) > 128 and min(T, L) <= 128', lambda T, L: max(T, L) > 128 and min(T, L) <= 128),
    'attn_bwd_kernel': ('the rest: L >= 33 with max(T, L) <= 128, or both beyond 128', lambda T, L: (L >= 33 and max(T, L) <= 128) or min(T, L) > 128),
}


def table(out=sys.stdout):
    """which attention kernel and how many row tiles per workgroup serve which (T, L, B): the regions in words, checked here against the
    restatement over every T, L <= 256, and the cases of tests/test_gpu_da_forms.py that run them"""
    rng = range(1, 257)
    served = {(T, L): [t.attn_fwd_form(T, L), t.attn_bwd_form(T, L)] for T in rng for L in rng}
    for (T, L), fb in served.items():
        assert [k for k, (_, pred) in RULES.items() if pred(T, L)] == fb, (T, L, fb)
    shapes = sorted({(sh['B'], sh['T'], sh['L']) for _, _, sh in t.CASES})
    fmt = lambda cs: ' '.join('(%d,%d,%d)' % c for c in cs)
    print('| kernel | region (T frames, L words, both at most 256) | shapes | cases of `test_gpu_da_forms.py` (B, T, L) |\n|---|---|---|---|', file=out)
    for k, (words, _) in RULES.items():
        print('| `%s` | %s | %d | %s |' % (k, words, sum(k in fb for fb in served.values()), fmt(c for c in shapes if k in t.dispatch(*c))), file=out)
    print('\n| row tiles per workgroup | rows R = B (T + L) | kernels | cases (B, T, L) |\n|---|---|---|---|', file=out)
    for nt in (1, 2, 3, 4):
        cs = [c for c in shapes if nt in t.row_tiles(*c)]
        rows = 'R <= 4096' if nt == 1 else '%d < R <= %d' % (4096 * (nt - 1), 4096 * nt) if nt < 4 else 'R > 12288'
        kern = '`ln_proj_kernel<%d, true>`' % nt
        if nt < 4:
            kern += ', `da_post_kernel<{0}>`, `ln_proj_bwd_kernel<false, {0}>`, `da_mid_bwd_kernel<{0}>`, `ln_proj_bwd_kernel<false, {0}, true>`'.format(nt)
        if nt == 3:
            rows += ' (R > 8192 for the kernels of at most 48 rows)'
        print('| %d | %s | %s | %s |' % (nt, rows, kern, 'every other case (%d shapes)' % len(cs) if nt == 1 else fmt(cs)), file=out)


def main(path):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    failed, legend = [], []
    with open(path, 'w') as out:
        for cls, layer, shape in t.CASES:
            try:
                measure(out, cls, layer, shape, legend)
            except AssertionError as e:      # the launched symbols or the 1e-3 gate: reported, the other cases still run
                failed.append((cls, layer, shape))
                print('# FAILED %s layer %d %s: %s' % (cls, layer, t._id(shape), str(e)[:2000]), file=out, flush=True)
    with open(path) as f:
        lines = f.read().splitlines()
    with open(path, 'a') as out:
        summary(lines, out)
    summary(lines)
    assert not failed, failed


if __name__ == '__main__':
    if '--summary' in sys.argv:
        summary(open(sys.argv[-1]).read().splitlines())
    elif '--table' in sys.argv:
        table()
    else:
        main(sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else os.path.join(ROOT, 'profiles', 'da_forms_parity.txt'))
