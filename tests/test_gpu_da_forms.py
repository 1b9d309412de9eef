"""GPU: every kernel form of the dual attention block - csrc/attn.hip launch_attn_fwd / launch_attn_bwd choose five forward instantiations
and three backward kernels by (T, L), csrc/dablock.hip the row tiles per workgroup of ln_proj / da_post / ln_proj_bwd / da_mid_bwd by the
row count - against the oracle, each case proving in the same test which kernels it ran (hual_prof_get), so a change of the dispatch
cannot take a shape off a form without a failing test.  The dispatch is restated below (`dispatch`); tests/test_da_dispatch.py (no GPU)
holds the case table to every instantiation that restatement can return.

Two gates per case.  The 1e-3 contract of test_gpu_blocks.test_dual_attn_fwd_bwd (_close, _check_param_grads), and a gate at the float32
noise floor: the block has no ReLU, so it is compared with R.dual_attn_block in float64 (parameters and inputs cast, the same dropout
masks), next to the float32 oracle's own distance to float64:  d_hip = max|hip - f64|  <=  M max(d_32, 2^-23 s),  d_32 = max|f32 - f64|,
s = max|f64| of the tensor (y, dx) or the block's largest parameter gradient (the parameter gradients, as _check_param_grads scales them:
the key-bias gradients are zero in exact arithmetic).

M per class of case (the rows of the table below): twice the worst ratio d_hip / max(d_32, 2^-23 s) measured on an MI355X over every
case and tensor here at three data seeds (profiles/da_forms_parity.txt, scripts/da_forms_parity.py), rounded up to a power of two, and
never above 16 - a condition, not a measurement: 22-bit operands are 4 float32 rounding units, the other factor 4 is for subnormal
residuals under the fixed attention scales 2^4 / 2^10.  The factor two is the spread of a maximum norm from seed
to seed, as argued in test_gpu_cq_forms.py.
  fwd (the cases listed for a forward instantiation): worst 1.87 (B1 T64 L64, no dropout, gradient of dense_1/bias, d_hip 1.1e-5 against
    d_32 6.1e-6) -> M = 4.
  chain: worst 1.50 (B8 T128 L32, dropout on, gradient of layer_norm_1/layer_norm_bias, 4.8e-5 against 3.2e-5) -> M = 4.
  plain (attn_bwd_kernel with four jobs): worst 1.57 (B8 T129 L129, dropout on, the same gradient, 6.5e-5 against 4.1e-5) -> M = 4.
  big: worst 1.75 (B8 T129 L32, no dropout, gradient of layer_norm_2/layer_norm_bias, 3.9e-5 against 2.2e-5) -> M = 4.
  tiles (two to four row tiles per workgroup): worst 3.07 (B171 T64 L8, no dropout, gradient of f_value/bias, 1.6e-4 against 4.6e-5:
    a sum over 12312 rows) -> M = 8.
No (case, tensor) comes near the cap.  Over the three seeds a tensor's largest ratio is 1.3 times its smallest in the median, 3.2 times
at most; at the data the cases below use (seed 0) the worst ratios are 1.43, 1.49, 1.57, 1.75 and 2.65.  The gradient sums use float
atomics, so a gradient's ratio moves from run to run: three runs of the table gave 1.57 .. 1.68 (plain), 1.65 .. 1.75 (big) and
3.03 .. 3.07 (tiles) as the worst.  A case takes 0.1 .. 0.3 s, the row-tile cases of 4104 / 8208 / 12312 rows 0.2 / 0.4 / 0.5 s.
What the gate sees: with the lo.hi pass of dS.K taken out of the second and third job of attn_bwd_chain (a scratch build), the 29 cases
here that run the chain kernel fail it with ratios of 80 .. 265 (dx, the query and layer_norm_1 gradients) after passing the 1e-3 gate,
which test_gpu_blocks.test_dual_attn_fwd_bwd passes too.
"""
import os

import pytest
import torch

import parity_util as pu
from oracle import philox as px
from oracle import seqpan_ref as R
from test_gpu_blocks import DROP, OFFSET, SEED, Block, _check_param_grads, _close
from test_gpu_da_bwd_fused import _grid, _prof

pytestmark = pytest.mark.gpu


def _flag(name):
    """csrc/attn.hip getenv_flag"""
    v = os.environ.get(name)
    if v is None:
        return False
    v = v.strip()
    k = 1 if v[:1] in ('+', '-') else 0
    while k < len(v) and v[k].isdigit():
        k += 1
    return v[:k] not in ('', '+', '-') and int(v[:k]) != 0


if _flag('HUAL_ATTN_NO_BIG'):
    raise RuntimeError('HUAL_ATTN_NO_BIG takes attn_bwd_big_kernel out of the dispatch: test_gpu_da_forms.py states which kernel serves '
                       'which shape and cannot run under it')

M = {'fwd': 4.0, 'chain': 4.0, 'plain': 4.0, 'big': 4.0, 'tiles': 8.0}
CAP = 16.0


# ---------------------------------------------------------------------------------------------------- the dispatch, restated
def _cdiv(a, b):
    return (a + b - 1) // b


def attn_jobs(T, L):
    """(Tq, Tk) of the four attentions of a layer in launch order (csrc/seqpan.hip da_bufs): video self, video -> query, query self,
    query -> video"""
    return [(T, T), (T, L), (L, L), (L, T)]


def attn_fwd_form(T, L):
    """csrc/attn.hip launch_attn_fwd: key tiles of the longest key side -> NK; eight waves when the launch has eight (job, 16-query tile)
    units, i.e. cdiv(T, 16) + cdiv(L, 16) >= 4"""
    nkt = _cdiv(max(T, L), 16)
    nk = 2 if nkt <= 2 else 4 if nkt <= 4 else 8 if nkt <= 8 else 16
    units = sum(_cdiv(tq, 16) for tq, _ in attn_jobs(T, L))
    return 'attn_fwd_kernel<%d, %d>' % (nk, 512 if units >= 8 else 256)


def attn_bwd_form(T, L):
    """csrc/attn.hip launch_attn_bwd: the jobs stable-sorted by Tq Tk, largest first; chain iff the two smallest have <= 32 queries and
    <= 128 keys; else the eight-wave kernel iff the largest job alone has more than 128 queries AND keys"""
    j = sorted(attn_jobs(T, L), key=lambda q: -q[0] * q[1])
    if all(tq <= 32 and tk <= 128 for tq, tk in j[2:]):
        return 'attn_bwd_chain_kernel'
    large = [tq > 128 and tk > 128 for tq, tk in j]
    if large[0] and not any(large[1:]):
        return 'attn_bwd_big_kernel'
    return 'attn_bwd_kernel'


def tile_rows(R_, Nv, cap):
    """csrc/common.h xcd_clip_rows(R, Nv, 16, cap): rows per workgroup of a row-local launch"""
    mt = max(_cdiv(R_, 256), 16)
    while mt < cap and _grid(R_, Nv, mt) > 256:
        mt += 1
    return min(mt, cap)


LP_ROWS, DP_ROWS = 64, 48      # csrc/lnproj_body.h, csrc/dablock.hip (= LB_ROWS): ln_proj takes up to four 16-row tiles per workgroup, every other row-local kernel three


def row_tiles(B, T, L):
    """(NT of ln_proj, NT of da_post / ln_proj_bwd / da_mid_bwd)"""
    R_, Nv = B * (T + L), B * T
    return _cdiv(tile_rows(R_, Nv, LP_ROWS), 16), _cdiv(tile_rows(R_, Nv, DP_ROWS), 16)


def dispatch(B, T, L):
    """{kernel symbol: launches} of hual_dual_attn_fwd + hual_dual_attn_bwd of one layer - the families attn_*, da_*, ln_proj*, ln2_mid*
    (a per-block call runs the unfused backward pair, tests/test_gpu_da_bwd_fused.py)"""
    nt4, nt3 = row_tiles(B, T, L)
    return {'ln_proj_kernel<%d, true>' % nt4: 1, attn_fwd_form(T, L): 1, 'da_post_kernel<%d>' % nt3: 1,
            'ln_proj_bwd_kernel<false, %d>' % nt3: 1, 'da_mid_bwd_kernel<%d>' % nt3: 1, attn_bwd_form(T, L): 1,
            'ln_proj_bwd_kernel<false, %d, true>' % nt3: 1}


FAMILY = ('attn_', 'da_', 'ln_proj', 'ln2_mid')


def _tile_B(rows, T=64, L=8):
    """the smallest clip count that puts B (T + L) rows over `rows`"""
    return rows // (T + L) + 1


# (class of the noise-floor gate, what the case is there for, B, T, L).  B from {1, 3, 8, 9}: every backward kernel once with whole XCD
# groups (B % 8 == 0) and once on its interleaved fallback; B = 9 leaves workgroups of the forward grid (xcd_round8) idle
TABLE = [
    ('fwd', 'fwd <2,256>', [(3, 5, 3), (9, 16, 16), (1, 32, 16)]),
    ('fwd', 'fwd <2,512>', [(3, 32, 17), (8, 32, 32)]),
    ('fwd', 'fwd <4,512>', [(9, 33, 1), (3, 48, 49), (1, 64, 64)]),
    ('fwd', 'fwd <8,512>', [(3, 65, 9), (8, 128, 128)]),
    ('fwd', 'fwd <16,512>, nkt_pad 16 and 2 in one launch', [(9, 129, 9), (1, 256, 20)]),
    ('chain', 'chain at its edges', [(8, 128, 32), (3, 20, 32), (1, 32, 32)]),                      # (20, 32): L > T
    ('plain', 'one word past chain: attn_bwd_kernel, four jobs', [(3, 128, 33), (8, 40, 36)]),
    ('big', 'one frame past chain: big', [(8, 129, 32), (3, 131, 12), (9, 256, 20)]),            # (131, 12): odd query pairs
    ('big', 'big with the query side as the large job', [(3, 3, 129)]),
    ('plain', 'two large jobs: attn_bwd_kernel at 8 key blocks', [(8, 129, 129), (1, 256, 256)]),
    ('tiles', 'row tiles NT = 1, ragged last tile', [(5, 50, 11)]),
    ('tiles', 'row tiles NT = 2, 3 and 4 (ln_proj)', [(_tile_B(4096), 64, 8), (_tile_B(8192), 64, 8), (_tile_B(12288), 64, 8)]),
]
# layer 1 once per backward kernel
LAYER1 = [('chain', (3, 20, 32)), ('plain', (8, 40, 36)), ('big', (3, 131, 12))]


def _shape(B, T, L, seed):
    # (vdim: the block never reads the clip features; 64 keeps the batches of the row-tile cases small)
    return dict(B=B, T=T, L=L, C=4, seed=seed, max_vlen=max(T, L), vdim=64)


CASES = [(cls, 0, _shape(B, T, L, 700 + 10 * i + k)) for i, (cls, _, shapes) in enumerate(TABLE) for k, (B, T, L) in enumerate(shapes)]
CASES += [(cls, 1, _shape(B, T, L, 900 + i)) for i, (cls, (B, T, L)) in enumerate(LAYER1)]
# every (case, dropout) the tests run: layer 0 with and without dropout, layer 1 with
RUNS = [(cls, layer, shape, drop) for cls, layer, shape in CASES for drop in ((DROP, 0.0) if layer == 0 else (DROP,))]


def _id(v):
    return 'B%d_T%d_L%d' % (v['B'], v['T'], v['L']) if isinstance(v, dict) else str(v)


def covered_symbols():
    """every symbol some case of the table is predicted to launch (tests/test_da_dispatch.py)"""
    return {s for _, _, sh in CASES for s in dispatch(sh['B'], sh['T'], sh['L'])}


# ---------------------------------------------------------------------------------------------------- one case
def _launch(blk, layer, drop, xseed=3):
    """hual_dual_attn_fwd + hual_dual_attn_bwd on random activations (xseed 3: those of test_gpu_blocks.test_dual_attn_fwd_bwd) between
    hual_prof_begin and hual_prof_end; returns x, dy, y, dx on the host and {kernel symbol: launches}"""
    lib, l = blk.lib, blk.l
    blk.opts = blk.m._opts(drop)
    x, dy = blk.rand(blk.R, xseed), blk.rand(blk.R, xseed + 1)
    xd, dyd = x.to(blk.dev), dy.to(blk.dev)
    y, dx = torch.empty_like(xd), torch.empty_like(xd)

    def call():
        lib.check(l.hual_dual_attn_fwd(*blk.args(), layer, lib.ptr(xd), lib.ptr(y), *blk.tail()))
        lib.check(l.hual_dual_attn_bwd(*blk.args(), layer, lib.ptr(dyd), lib.ptr(dx), lib.ptr(blk.grads), *blk.tail()))
    got = _prof(lib, l, call)
    return x, dy, y.cpu(), dx.cpu(), got


def _assert_form(blk, got):
    """exactly the predicted symbols of the attn_ / da_ / ln_proj / ln2_mid families, at the predicted launch counts"""
    ran = {k: c for k, c in got.items() if k.startswith(FAMILY)}
    want = dispatch(blk.B, blk.T, blk.L)
    assert ran == want, ('launched', ran, 'predicted', want)
    return want


def _oracle(blk, layer, x, dy, drop, dt):
    """R.dual_attn_block in both directions at dtype dt -> (parameters with .grad, y, dx)"""
    rng = px.DropoutRNG(SEED, OFFSET, drop)
    pr = {k: t.detach().clone().to(dt).requires_grad_(True) for k, t in blk.p.items()}
    xr = x.clone().to(dt).requires_grad_(True)
    v, q = blk.split(xr)
    n, site, H = 'd_attn_%d' % layer, px.SITE_DA + 8 * layer, blk.cfg.num_heads
    v_ = R.dual_attn_block(v, q, pr, n, H, blk.v_mask, blk.q_mask, rng, site, blk.rows_v)
    q_ = R.dual_attn_block(q, v, pr, n, H, blk.q_mask, blk.v_mask, rng, site, blk.rows_q)
    out = torch.cat([v_.reshape(blk.Nv, 128), q_.reshape(blk.Nq, 128)])
    out.backward(dy.to(dt))
    return pr, out.detach(), xr.grad


def _floor_rows(blk, layer, y, dx, o64, o32):
    """[(tensor, d_hip, d_32, s, d_hip / max(d_32, 2^-23 s))] for y, dx and every parameter gradient of the layer"""
    ref = {}
    for dt, (pr, out, xg) in (('f64', o64), ('f32', o32)):
        ref[dt] = dict({'grad ' + k: t.grad.double() for k, t in pr.items() if t.grad is not None}, y=out.double(), dx=xg.double())
    f64, f32 = ref['f64'], ref['f32']
    hg = blk.params_grad()
    hip = dict({k: torch.from_numpy(hg[k[5:]]).double().reshape(f64[k].shape) for k in f64 if k.startswith('grad ')}, y=y.double(), dx=dx.double())
    assert sorted(f32) == sorted(f64) and len(hip) > 2 and all(k in ('y', 'dx') or k[5:].startswith('d_attn_%d/' % layer) for k in hip), sorted(hip)
    gmax = max(float(t.abs().max()) for k, t in f64.items() if k.startswith('grad '))
    rows = []
    for k in sorted(f64):
        d_hip, d_32 = float((hip[k] - f64[k]).abs().max()), float((f32[k] - f64[k]).abs().max())
        s = gmax if k.startswith('grad ') else float(f64[k].abs().max())
        rows.append((k, d_hip, d_32, s, d_hip / max(d_32, 2.0 ** -23 * s)))
    return rows


def run_case(blk, layer, drop, xseed=3):
    """launch, (a) the form and (b) the 1e-3 gate asserted; returns the predicted symbols and the rows of the noise-floor gate"""
    x, dy, y, dx, got = _launch(blk, layer, drop, xseed)
    want = _assert_form(blk, got)
    o32 = _oracle(blk, layer, x, dy, drop, torch.float32)
    _close('y', y, o32[1])
    _close('dx', dx, o32[2])
    _check_param_grads(blk, o32[0], lambda k: k.startswith('d_attn_%d/' % layer))
    return want, _floor_rows(blk, layer, y, dx, _oracle(blk, layer, x, dy, drop, torch.float64), o32)


def make_block(shape):
    """Block(**shape); R.synthetic_batch draws queries of at least three words, so a shorter L takes the first L word columns of an
    L = 3 batch (every query keeps all its L words)"""
    if shape['L'] >= 3:
        return Block(**shape)
    cfg, p, wv, b, labels = pu.make_case(**dict(shape, L=3))
    b['word_ids'], b['char_ids'] = b['word_ids'][:, :shape['L']].contiguous(), b['char_ids'][:, :shape['L']].contiguous()
    make, pu.make_case = pu.make_case, lambda **kw: (cfg, p, wv, b, labels)
    try:
        blk = Block()
    finally:
        pu.make_case = make
    assert (blk.B, blk.T, blk.L) == (shape['B'], shape['T'], shape['L']) and int(blk.q_mask.sum()) == blk.Nq
    return blk


def _form_name(want):
    return ' '.join(sorted(s.replace('_kernel', '').replace(', ', ',') for s in want if s.startswith('attn_')))


def _case(cls, layer, shape, drop):
    """one parity case: (a) the kernels that ran, (b) the 1e-3 gate, (c) the gate at the noise floor"""
    blk = make_block(shape)
    want, rows = run_case(blk, layer, drop)
    for r in rows:
        print('%-5s %s B%d T%d L%d layer %d drop %.1f  %-70s d_hip %.3e  d_32 %.3e  s %.3e  ratio %6.2f'
              % ((cls, _form_name(want), blk.B, blk.T, blk.L, layer, drop) + r))
    assert M[cls] <= CAP
    bad = [r for r in rows if not r[4] <= M[cls]]
    assert not bad, (cls, 'M = %g' % M[cls], bad)


# ---------------------------------------------------------------------------------------------------- block parity per form
@pytest.mark.parametrize('cls,layer,shape,drop', RUNS, ids=_id)
def test_dual_attn_fwd_bwd_by_form(cls, layer, shape, drop):
    assert drop in (0.0, DROP)
    _case(cls, layer, shape, drop)
