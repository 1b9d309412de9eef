"""python scripts/cb_forms_parity.py [--out FILE] (on the GPU) writes profiles/cb_forms_parity.txt: every case of tests/test_gpu_cb_forms.py
at three data seeds (the test's own and two more: batch and activations) - the kernels that ran, asserted against the test's restatement of
the dispatch, the 1e-3 gate, and per tensor the ratio d_hip / max(d_32, 2^-23 s) of max|hip - f64| to max|f32 oracle - f64|, the quantity
the test's M constants bound; one line per (case, dropout), closed by the worst ratio per class of case.
python scripts/cb_forms_parity.py --summary FILE prints those closing lines from a table's own rows (no GPU needed)."""
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import test_gpu_cb_forms as t      # noqa: E402

SEEDS = 3
HEAD = '# class | block | shape | MT fwd/bwd, tiles per layer fwd / bwd, grids | dropout | s per case | largest ratio | its tensor, d_hip and d_32 | ratio at seeds 0/1/2 per tensor, in the order:'
SHORT = (('grad conv_block/', 'cb/'), ('grad predictor/feature_encoder/', 'fe/'), ('grad predictor/', 'p/'), ('multihead_attention_block/', 'mab/'),
         ('depthwise_conv_layers_', 'dw'), ('layer_norm', 'ln'), ('top_self_attention/', 'tsa/'))


def _short(name):
    for a, b in SHORT:
        name = name.replace(a, b)
    return name


def _form_txt(kind, sh):
    f = t.cb_form(sh['B'], sh['T'], sh['L']) if kind == 'conv_block' else t.pred_form(sh['B'], sh['T'])
    return 'MT %d/%d tiles %s / %s grids %d/%d' % (f['mt'] + (''.join(map(str, f['fwd_tiles'])), ''.join(map(str, f['bwd_tiles'])), f['grid'][0][0], f['grid'][1][0]))


def measure(out, kind, cls, shape, drops, legends):
    """one line per dropout setting: the largest ratio with its tensor, d_hip and d_32, and every tensor's ratio at each seed"""
    res, t0 = {}, time.time()
    run = t.run_cb if kind == 'conv_block' else t.run_pred
    for k in range(SEEDS):
        blk = t.make_block(dict(shape, seed=shape['seed'] + 1000 * k))
        for drop in drops:
            t.set_drop(blk, drop)
            for name, d_hip, d_32, s, ratio in run(blk, xseed=(1 if kind == 'conv_block' else 7) + 10 * k):
                res.setdefault(drop, {}).setdefault(_short(name), []).append((ratio, d_hip, d_32))
    sec = (time.time() - t0) / (SEEDS * len(res))
    legend = legends.setdefault(kind, [])
    for drop, v in res.items():
        if not legend:
            legend.extend(v)
            print(HEAD + ' ' + ' '.join(legend), file=out, flush=True)
        assert list(v) == legend
        w, name = max((max(r), n) for n, r in v.items())
        print('%-8s|%-10s|B%d T%d L%d|%s|drop %.1f|%.1f s|max %.2f|%s d_hip %.3e d_32 %.3e|%s'
              % (cls, kind, blk.B, blk.T, blk.L, _form_txt(kind, shape), drop, sec, w[0], name, w[1], w[2],
                 ' '.join('/'.join('%.2f' % r[0] for r in v[n]) for n in legend)), file=out, flush=True)


def summary(lines, out=sys.stdout):
    """per class of case: the worst line (without its last column), M by the rule (twice the worst ratio, rounded up to a power of two, at
    most the cap) and the seed-to-seed spread (a tensor's largest ratio / its smallest, over the tensors whose ratio stays above 0.1)"""
    by, spread = {}, {}
    for ln in lines:
        f = [c.strip() for c in ln.split('|')]
        if len(f) != 9 or ln.startswith('#'):
            continue
        per = [[float(x) for x in c.split('/')] for c in f[8].split()]
        by.setdefault(f[0], []).append((max(max(p) for p in per), max(p[0] for p in per), ln[:ln.rindex('|')]))
        spread.setdefault(f[0], []).extend(max(p) / min(p) for p in per if min(p) >= 0.1)      # (gradients that are zero on both sides: ratio 0)
    for cls in t.M:
        if cls not in by:
            continue
        w, w0 = max(v[0] for v in by[cls]), max(v[1] for v in by[cls])
        f = [c.strip() for c in max(by[cls])[2].split('|')]
        print('# class %-8s: worst ratio %.2f (%s; seed 0, the test\'s own data: %.2f) -> twice that, rounded up to a power of two: %g; cap %g; the '
              'test has M = %g.  Over the three seeds a tensor\'s largest / smallest ratio is at most %.2f, median %.2f; %s per case'
              % (cls, w, ' '.join([f[2], f[4], f[7]]), w0, 2.0 ** math.ceil(math.log2(2.0 * w)), t.CAP, t.M[cls], max(spread[cls]),
                 statistics.median(spread[cls]), ' .. '.join(sorted({v[2].split('|')[5].strip() for v in by[cls]}))), file=out)


def main(path):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    failed, legends = [], {}
    with open(path, 'w') as out:
        for kind, runs, cases in (('conv_block', t.CB_RUNS, t.CB_CASES), ('predictor', t.PRED_RUNS, t.PRED_CASES)):
            for cls, shape in cases:
                drops = [d for c, sh, d in runs if sh is shape]
                try:
                    measure(out, kind, cls, shape, drops, legends)
                except AssertionError as e:      # the launched symbols or the 1e-3 gate: reported, the other cases still run
                    failed.append((kind, cls, shape))
                    print('# FAILED %s %s %s: %s' % (kind, cls, t._id(shape), str(e)[:3000]), file=out, flush=True)
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
        main(sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else os.path.join(ROOT, 'profiles', 'cb_forms_parity.txt'))
