"""GPU: every tile form of the fused conv block (csrc/convblock.hip conv_block_fwd_kernel / conv_block_bwd_kernel) and of the conditioned
predictor around it (csrc/seqpan.hip fwd_fe / fwd_heads / bwd_heads / bwd_fe) against the oracle, each case proving in the same test which
kernels it ran (hual_prof_get), so a change of the dispatch cannot take a shape off a form without a failing test.  The dispatch is
restated below; tests/test_cb_dispatch.py (no GPU) holds the case table to every class of form named here.

What chooses a form.  Rows per workgroup MT = xcd_clip_rows(R, Nv, 16, cap) (csrc/common.h; `tile_rows`), cap 46 forward and 40 backward,
over the unified row space (Nv video rows, then the query rows) for the shared encoder and over the one row space of the video rows
(Nv = 0) for the predictor's two encoder passes.  Per layer the matrix phase takes tf_mma_lean<4> instead of <3> when its rows need a
fourth 16-row tile: forward layer l works on nout = MT + 2 (9 - 3 l) rows (four tiles from MT 31 / 37 / 43 for l = 0 / 1 / 2, never
for l = 3), backward layer i on nG = MT + 6 (i + 1) rows (from MT 25 / 31 / 37 for i = 3 / 2 / 1, never for i = 0).  Beyond 256
workgroups at the capped MT the launch takes a second round; beyond the backward cap the backward reads statistics, relu bits and keep
bits that forward tiles of another height wrote.  The predictor adds heads_kernel<8 | 16> (T <= 128 or not), the single-job
attn_fwd_kernel<NK, 256 | 512> (eight waves from eight 16-query tiles on: T > 112), attn_bwd_kernel or - beyond 128 frames - the
eight-wave attn_bwd_big_kernel, ln_proj_kernel<NT, plain> at ln_proj_rows (cap 64), ln_proj_pair_kernel<NT> at ln_proj_pair_rows
(both problems in one round: 2 grid <= 256, cap 64) and ln_proj_bwd_kernel<pre, NT> at ln_proj_bwd_rows (cap 48).

Two gates per case.  (a) The 1e-3 contract of test_gpu_blocks.test_conv_block_fwd_bwd / test_predictor_fwd_bwd: _close on y and dx (the
logits and d_outputs), _check_param_grads on the block's parameter gradients, assert_pins_ok on the kernel's relu pins, span indices equal
on the kernel's own logits.  (b) A gate at the float32 noise floor: the oracle is evaluated with the kernel's pins and the same dropout
masks in float32 and in float64 (parameters and inputs cast); with the active sets shared all three sides compute z * pin, so the
comparison is smooth.  d_hip = max|hip - f64|  <=  M max(d_32, 2^-23 s),  d_32 = max|f32 - f64|,  s = max|f64| of the tensor or, for
the parameter gradients, the block's largest gradient (as _check_param_grads scales them).

M per class of case (the rows of the tables below): twice the worst ratio d_hip / max(d_32, 2^-23 s) measured on an MI355X over every
case and tensor of the class at three data seeds (profiles/cb_forms_parity.txt, scripts/cb_forms_parity.py), rounded up to a power of
two, never above 16 - a condition, not a measurement (the cap test_gpu_da_forms.py justifies for 22-bit split operands).  The factor two
is the spread of a maximum norm from seed to seed, as argued in test_gpu_cq_forms.py.
Worst ratio per class (case, dropout, tensor, d_hip against d_32) -> M:
  t3      2.15 (B190 T12 L5, no dropout, gradient of depthwise_conv_layers_0/bias, 3.4e-5 against 1.4e-5) -> 8
  b4      3.34 (B410 T12 L5, no dropout, gradient of depthwise_conv_layers_2/bias, 8.5e-5 against 2.1e-5) -> 8
  f1b2    2.40 (B480 T12 L5, no dropout, the same gradient, 7.7e-5 against 3.2e-5) -> 8
  mt37    2.71 (B560 T12 L5, no dropout, gradient of depthwise_conv_layers_3/bias, 9.0e-5 against 2.6e-5) -> 8
  fcap    1.95 (B610 T12 L5, no dropout, gradient of depthwise_conv_layers_2/bias, 7.3e-5 against 3.7e-5) -> 4
  f3      2.12 (B650 T12 L5, no dropout, gradient of depthwise_conv_layers_1/bias, 7.5e-5 against 3.1e-5) -> 8
  round2  1.94 (B860 T12 L5, dropout on, gradient of depthwise_conv_layers_0/bias, 9.0e-5 against 4.7e-5) -> 4
  short   2.93 (B1000 T3 L2, dropout on, gradient of depthwise_conv_layers_3/bias, 8.3e-5 against 2.0e-5) -> 8
  p_tiny  1.48 (B250 T5, dropout on, d_outputs, 5.3e-6 against 3.6e-6) -> 4
  p_four  2.24 (B1000 T8, no dropout, gradient of multihead_attention_block/dense/kernel, 3.7e-5 against 1.6e-5) -> 8
  p_ragged 1.50 (B47 T131, no dropout, gradient of the encoder's depthwise_conv_layers_3/bias, 3.4e-5 against 2.3e-5) -> 4
  p_fcap  1.43 (B80 T129, no dropout, gradient of the encoder's depthwise_conv_layers_2/depthwise_filter, 7.8e-5 against 5.5e-5) -> 4
  p_max   1.72 (B40 T256, dropout on, gradient of the encoder's depthwise_conv_layers_3/bias, 5.6e-5 against 3.3e-5) -> 4
No ratio exceeds 8, so none is a finding about the kernels, and no class comes near the cap.  The worst tensors are pointwise-bias
gradients - sums of dZ over up to 14 620 rows, where the summation order of the weight-gradient launch meets the oracle's; y, dx, the
logits and d_outputs stay below 1.5 everywhere.  At the data the cases below use (seed 0) the worst ratios are 1.37, 1.75, 2.40, 1.81,
1.70, 1.89, 1.88, 2.09 (shared encoder) and 1.17, 2.24, 1.24, 1.43, 1.72 (predictor); over the three seeds a tensor's largest ratio is
1.3 .. 1.5 times its smallest in the median, at most 3.6 times in the shared encoder and 8.9 times in the predictor (tensors whose
ratio stays above 0.1).  A case takes 0.2 .. 1.3 s of test
time in the shared encoder (14 620 rows: 1.0 s) and 0.3 .. 2.5 s in the predictor (B40 T256, whose float64 oracle is most of it).
What the gates see: with the two residual passes (hi.lo, lo.hi) taken out of tf_mma_lean<4> only (a scratch build; arithmetic only), 25
of the 33 cases here fail while test_gpu_blocks.test_conv_block_fwd_bwd / test_predictor_fwd_bwd still pass.  The two b4 cases, where
only the backward's layer 3 runs the four-tile product, pass gate (a) whole and fail gate (b) with ratios of 128 / 147 (dx) and 28 / 40
(depthwise_filter gradients).  The other 23 - every case with a four-tile forward layer, and the predictor cases whose ln_proj_pair
launch takes four row tiles - fail already in gate (a), at assert_pins_ok: relu pins that disagree with the oracle at units of |z| =
1.1e-4 .. 2.2e-4 max|z| against PIN_Z_TOL = 1e-4, which neither block test at 16 rows per workgroup reaches.  The 8 cases that pass
are the ones that never run the four-tile product: t3, p_tiny, and the short-clip cases at MT 16 / 20 / 24.
"""
import pytest
import torch

import parity_util as pu
from oracle import philox as px
from oracle import seqpan_ref as R
from test_gpu_blocks import DROP, OFFSET, SEED, Block, _check_param_grads, _close
from test_gpu_da_bwd_fused import _grid, _prof
from test_gpu_da_forms import _cdiv, tile_rows

pytestmark = pytest.mark.gpu

CAP = 16.0
M = {'t3': 8.0, 'b4': 8.0, 'f1b2': 8.0, 'mt37': 8.0, 'fcap': 4.0, 'f3': 8.0, 'round2': 4.0, 'short': 8.0,
     'p_tiny': 4.0, 'p_four': 8.0, 'p_ragged': 4.0, 'p_fcap': 4.0, 'p_max': 4.0}


# ---------------------------------------------------------------------------------------------------- the dispatch, restated
CB_FWD_CAP, CB_BWD_CAP = 46, 40      # csrc/convblock.h HUAL_CB_MAXMT, HUAL_CB_BWD_MAXMT
LP_ROWS, LB_ROWS = 64, 48            # csrc/lnproj_body.h, csrc/dablock.hip


def cb_rows(R_, Nv):
    """csrc/convblock.hip conv_block_fused_rows / conv_block_fused_rows_bwd: (forward MT, backward MT); Nv = 0: one row space"""
    return tile_rows(R_, Nv, CB_FWD_CAP), tile_rows(R_, Nv, CB_BWD_CAP)


def fwd_tiles(mt):
    """NT of the tf_mma_lean<NT> product of forward layer 0 .. 3: four when the nout = MT + 2 (9 - 3 l) rows need a fourth 16-row tile,
    else the three-tile product (whatever fewer tiles the rows fill)"""
    return [4 if _cdiv(mt + 2 * (9 - 3 * l), 16) > 3 else 3 for l in range(4)]


def bwd_tiles(mt):
    """... of backward layer 0 .. 3: nG = MT + 6 (i + 1) rows"""
    return [4 if _cdiv(mt + 6 * (i + 1), 16) > 3 else 3 for i in range(4)]


def grid_rounds(R_, Nv, mt):
    """(workgroups of the launch, rounds of 256)"""
    g = _grid(R_, Nv, mt)
    return g, _cdiv(g, 256)


def straddles(Nv, mt):
    """a tile holds the last video rows and the first query rows"""
    return Nv % mt != 0


def cb_form(B, T, L):
    """the unified row space of the shared encoder: everything that chooses a code path in the two kernels"""
    R_, Nv = B * (T + L), B * T
    mf, mb = cb_rows(R_, Nv)
    return dict(R=R_, Nv=Nv, mt=(mf, mb), fwd_tiles=fwd_tiles(mf), bwd_tiles=bwd_tiles(mb), grid=(grid_rounds(R_, Nv, mf), grid_rounds(R_, Nv, mb)),
                straddle=(straddles(Nv, mf), straddles(Nv, mb)), ragged=(R_ % mf != 0, R_ % mb != 0))


def ln_proj_pair_rows(R_):
    """csrc/dablock.hip ln_proj_pair_rows"""
    mt = 16
    while mt < LP_ROWS and 2 * _grid(R_, 0, mt) > 256:
        mt += 1
    return mt


def pred_form(B, T):
    """the predictor's one row space"""
    Nv = B * T
    mf, mb = cb_rows(Nv, 0)
    return dict(R=Nv, mt=(mf, mb), fwd_tiles=fwd_tiles(mf), bwd_tiles=bwd_tiles(mb), grid=(grid_rounds(Nv, 0, mf), grid_rounds(Nv, 0, mb)),
                ragged=(Nv % mf != 0, Nv % mb != 0), ln_proj=tile_rows(Nv, 0, LP_ROWS), ln_proj_pair=ln_proj_pair_rows(Nv),
                ln_proj_bwd=tile_rows(Nv, 0, LB_ROWS))


def attn1_fwd_form(T):
    """csrc/attn.hip launch_attn_fwd with the one job (T, T)"""
    nkt = _cdiv(T, 16)
    nk = 2 if nkt <= 2 else 4 if nkt <= 4 else 8 if nkt <= 8 else 16
    return 'attn_fwd_kernel<%d, %d>' % (nk, 512 if nkt >= 8 else 256)


def attn1_bwd_form(T):
    """csrc/attn.hip launch_attn_bwd with one job: no chain; the eight-wave kernel beyond 128 queries and keys"""
    return 'attn_bwd_big_kernel' if T > 128 else 'attn_bwd_kernel'


def cb_dispatch(B, T, L):
    """{kernel symbol: launches} of hual_conv_block_fwd + hual_conv_block_bwd in the conv_block_ family (a per-block call keeps the
    dual attention's ln_proj launch out of the block's own)"""
    return {'conv_block_fwd_kernel': 1, 'conv_block_bwd_kernel': 1}


def pred_dispatch(B, T):
    """{kernel symbol: launches} of hual_predictor_fwd + hual_predictor_bwd in the families conv_block_, ln_proj, attn_, heads_kernel.
    Two encoder passes; a per-block call runs each ln_proj behind its conv block as a launch of its own, and forms the heads' dZ in a
    second heads launch (grad_only) of the same instantiation"""
    f = pred_form(B, T)
    nt, ntp, ntb = _cdiv(f['ln_proj'], 16), _cdiv(f['ln_proj_pair'], 16), _cdiv(f['ln_proj_bwd'], 16)
    return {'conv_block_fwd_kernel': 2, 'ln_proj_kernel<%d, true>' % nt: 2, attn1_fwd_form(T): 2, 'ln_proj_kernel<%d, false>' % nt: 2,
            'ln_proj_pair_kernel<%d>' % ntp: 1, 'heads_kernel<%d>' % (8 if T <= 128 else 16): 2,
            'ln_proj_bwd_kernel<true, %d>' % ntb: 2, attn1_bwd_form(T): 2, 'ln_proj_bwd_kernel<false, %d>' % ntb: 2, 'conv_block_bwd_kernel': 2}


CB_FAMILY = ('conv_block_',)
PRED_FAMILY = ('conv_block_', 'ln_proj', 'attn_', 'heads_kernel')

# (class of the noise-floor gate, what the class is there for, [(B, T, L)]): the shared encoder, unified rows.  Every class runs with
# dropout 0.2, its first case without dropout as well
CB_TABLE = [
    ('t3', 'three tiles everywhere', [(190, 12, 5)]),
    ('b4', 'one four-tile layer in the backward only (MT 25..30)', [(410, 12, 5)]),
    ('f1b2', 'forward layer 0 plus two backward layers (MT 31..36)', [(480, 12, 5)]),
    ('mt37', 'MT 37..40; long clips with 3-word queries', [(560, 12, 5), (37, 256, 3)]),
    ('fcap', 'forward above the backward cap (41..42); one-word queries', [(610, 12, 5), (40, 256, 1)]),
    ('f3', 'forward with three four-tile layers (43..46)', [(650, 12, 5)]),
    ('round2', 'forward cap with a second round of workgroups', [(860, 12, 5)]),
    ('short', 'clips shorter than the window at MT > 16', [(1000, 5, 1), (1000, 3, 2), (1000, 1, 1), (1000, 6, 3), (1024, 8, 3)]),
]
# the predictor, one row space, position embeddings: [(B, T)]
PRED_TABLE = [
    ('p_tiny', 'tiny clips', [(250, 5)]),
    ('p_four', 'four-tile forward at T <= 128: short clips, bench clips', [(1000, 8), (64, 128)]),
    ('p_ragged', 'T just above 128, ragged last tile', [(47, 131)]),
    ('p_fcap', 'forward above the backward cap at T > 128', [(80, 129)]),
    ('p_max', 'both maxima', [(40, 256)]),
]
PRED_L = 3      # the predictor never reads the query rows: the shortest query the synthetic batches draw


def _shape(B, T, L, seed):
    # (vdim: neither block reads the clip features; 64 keeps the batches of a thousand clips small)
    return dict(B=B, T=T, L=L, C=4, seed=seed, max_vlen=max(T, L, 8), vdim=64)


CB_CASES = [(cls, _shape(B, T, L, 1100 + 10 * i + k)) for i, (cls, _, shapes) in enumerate(CB_TABLE) for k, (B, T, L) in enumerate(shapes)]
PRED_CASES = [(cls, _shape(B, T, PRED_L, 1300 + 10 * i + k)) for i, (cls, _, shapes) in enumerate(PRED_TABLE) for k, (B, T) in enumerate(shapes)]


def _runs(table, cases):
    first = {cls: shapes[0][:2] for cls, _, shapes in table}
    return [(cls, sh, drop) for cls, sh in cases for drop in ((DROP, 0.0) if (sh['B'], sh['T']) == first[cls] else (DROP,))]


CB_RUNS, PRED_RUNS = _runs(CB_TABLE, CB_CASES), _runs(PRED_TABLE, PRED_CASES)


def _id(v):
    return 'B%d_T%d_L%d' % (v['B'], v['T'], v['L']) if isinstance(v, dict) else str(v)


# ---------------------------------------------------------------------------------------------------- one case
MIN_T, MIN_L = 8, 3


def make_block(shape, drop=DROP):
    """Block(**shape).  R.synthetic_batch draws queries of at least three words and needs clips long enough to hold a labelled span, so a
    shorter T or L takes the first T frames / L word columns of a batch of MIN_T frames / MIN_L words (the clip lengths cut to T: every
    query keeps all its L words, and some clip still fills its T frames)"""
    T, L = shape['T'], shape['L']
    if T >= MIN_T and L >= MIN_L:
        return Block(drop=drop, **shape)
    cfg, p, wv, b, labels = pu.make_case(**dict(shape, T=max(T, MIN_T), L=max(L, MIN_L)))
    b = dict(b, video=b['video'][:, :T].contiguous(), lens=b['lens'].clamp(max=T), word_ids=b['word_ids'][:, :L].contiguous(),
             char_ids=b['char_ids'][:, :L].contiguous())
    blk = Block(drop=drop, case=(cfg, p, wv, b, labels))
    assert (blk.B, blk.T, blk.L) == (shape['B'], T, L) and (L >= MIN_L or int(blk.q_mask.sum()) == blk.Nq) and int(b['lens'].max()) == T
    return blk


def set_drop(blk, drop):
    """the same block at another dropout rate (scripts/cb_forms_parity.py)"""
    blk.drop, blk.opts, blk.rng = drop, blk.m._opts(drop), px.DropoutRNG(SEED, OFFSET, drop)


def _assert_form(got, family, want):
    """exactly the predicted symbols of the families, at the predicted launch counts"""
    ran = {k: c for k, c in got.items() if k.startswith(family)}
    assert ran == want, ('launched', ran, 'predicted', want)


def _floor_rows(blk, prefix, hip, o64, o32):
    """[(tensor, d_hip, d_32, s, d_hip / max(d_32, 2^-23 s))] for the output tensors and every parameter gradient of the block.
    hip: {name: tensor} of the outputs; o64 / o32: (parameters with .grad, {name: tensor}) of the oracle in float64 / float32"""
    ref = {}
    for dt, (pr, outs) in (('f64', o64), ('f32', o32)):
        ref[dt] = dict({'grad ' + k: t.grad.double() for k, t in pr.items() if t.grad is not None}, **{k: t.double() for k, t in outs.items()})
    f64, f32 = ref['f64'], ref['f32']
    hg = blk.params_grad()
    hip = dict({k: torch.from_numpy(hg[k[5:]]).double().reshape(f64[k].shape) for k in f64 if k.startswith('grad ')},
               **{k: t.double().reshape(f64[k].shape) for k, t in hip.items()})
    assert sorted(f32) == sorted(f64) == sorted(hip) and all(not k.startswith('grad ') or k[5:].startswith(prefix) for k in hip), sorted(hip)
    assert sum(k.startswith('grad ') for k in hip) >= 8, sorted(hip)
    gmax = max(float(t.abs().max()) for k, t in f64.items() if k.startswith('grad '))
    rows = []
    for k in sorted(f64):
        d_hip, d_32 = float((hip[k] - f64[k]).abs().max()), float((f32[k] - f64[k]).abs().max())
        s = gmax if k.startswith('grad ') else float(f64[k].abs().max())
        rows.append((k, d_hip, d_32, s, d_hip / max(d_32, 2.0 ** -23 * s)))
    return rows


def _params(blk, dt):
    return {k: t.detach().clone().to(dt).requires_grad_(True) for k, t in blk.p.items()}


def run_cb(blk, xseed=1):
    """hual_conv_block_fwd + hual_conv_block_bwd on random activations (xseed 1: those of test_gpu_blocks.test_conv_block_fwd_bwd); the
    launched kernels and gate (a) asserted; returns the rows of gate (b)"""
    lib, l = blk.lib, blk.l
    x, dy = blk.rand(blk.R, xseed), blk.rand(blk.R, xseed + 1)
    xd, dyd = x.to(blk.dev), dy.to(blk.dev)
    y, dx = torch.empty_like(xd), torch.empty_like(xd)

    def call():
        lib.check(l.hual_conv_block_fwd(*blk.args(), lib.ptr(xd), lib.ptr(y), *blk.tail()))
        lib.check(l.hual_conv_block_bwd(*blk.args(), lib.ptr(dyd), lib.ptr(dx), lib.ptr(blk.grads), *blk.tail()))
    _assert_form(_prof(lib, l, call), CB_FAMILY, cb_dispatch(blk.B, blk.T, blk.L))
    pins_v = [blk.m.tap_bits('cb.rb%d' % i)[:blk.Nv].reshape(blk.B, blk.T, -1) for i in range(4)]
    pins_q = [blk.m.tap_bits('cb.rb%d' % i)[blk.Nv:].reshape(blk.B, blk.L, -1) for i in range(4)]

    def oracle(dt):
        pr = _params(blk, dt)
        xr = x.clone().to(dt).requires_grad_(True)
        xv, xq = blk.split(xr)
        tv, tq = {}, {}
        yv = R.conv_block(xv, pr, 'conv_block', blk.rng, px.SITE_CONV, blk.rows_v, tv, 'cb', pins_v)
        yq = R.conv_block(xq, pr, 'conv_block', blk.rng, px.SITE_CONV, blk.rows_q, tq, 'cb', pins_q)
        ref = torch.cat([yv.reshape(blk.Nv, 128), yq.reshape(blk.Nq, 128)])
        ref.backward(dy.to(dt))
        return pr, dict(y=ref.detach(), dx=xr.grad), tv, tq
    pr, o32, tv, tq = oracle(torch.float32)
    # the pins are the kernel's own active sets: audit them against the oracle's pre-activations
    pu.assert_pins_ok([('v%d' % i, tv['cb.z%d' % i], pins_v[i]) for i in range(4)] + [('q%d' % i, tq['cb.z%d' % i], pins_q[i]) for i in range(4)])
    _close('y', y.cpu(), o32['y'])
    _close('dx', dx.cpu(), o32['dx'])
    _check_param_grads(blk, pr, lambda k: k.startswith('conv_block/'))
    return _floor_rows(blk, 'conv_block/', dict(y=y.cpu(), dx=dx.cpu()), oracle(torch.float64)[:2], (pr, o32))


def run_pred(blk, xseed=7):
    """hual_predictor_fwd + hual_predictor_bwd on random masked `outputs` and logit gradients (xseed 7: those of
    test_gpu_blocks.test_predictor_fwd_bwd); the launched kernels and gate (a) asserted; returns the rows of gate (b)"""
    lib, l = blk.lib, blk.l
    B, T, Nv = blk.B, blk.T, blk.Nv
    x = blk.rand(Nv, xseed) * blk.v_mask.reshape(Nv, 1).float()             # `outputs` is masked (model.py:97)
    g = torch.Generator().manual_seed(xseed + 1)
    ds, de = torch.randn(B, T, generator=g), torch.randn(B, T, generator=g)
    xd, dsd, ded = x.to(blk.dev), ds.to(blk.dev), de.to(blk.dev)
    s_log, e_log = torch.empty(B, T, device=blk.dev), torch.empty(B, T, device=blk.dev)
    si, ei = torch.empty(B, dtype=torch.int64, device=blk.dev), torch.empty(B, dtype=torch.int64, device=blk.dev)
    dx = torch.empty_like(xd)

    def call():
        lib.check(l.hual_predictor_fwd(*blk.args(), lib.ptr(xd), lib.ptr(s_log), lib.ptr(e_log), lib.ptr(si), lib.ptr(ei), *blk.tail()))
        lib.check(l.hual_predictor_bwd(*blk.args(), lib.ptr(dsd), lib.ptr(ded), lib.ptr(dx), lib.ptr(blk.grads), *blk.tail()))
    _assert_form(_prof(lib, l, call), PRED_FAMILY, pred_dispatch(B, T))
    pin = {}
    for ps in range(2):
        pin['fe%d' % ps] = [blk.m.tap_bits('fe%d.rb%d' % (ps, i)).reshape(B, T, -1) for i in range(4)]
    pin['head.hs'] = (blk.m.tap('head.hs').cpu() > 0).reshape(B, T, -1)
    pin['head.he'] = (blk.m.tap('head.he').cpu() > 0).reshape(B, T, -1)

    def oracle(dt):
        pr = _params(blk, dt)
        xr = x.clone().to(dt).requires_grad_(True)
        tap = {}
        s_ref, e_ref = R.conditioned_predictor(xr.reshape(B, T, 128), pr, blk.cfg.num_heads, blk.v_mask, blk.rng, blk.rows_v, tap, pin)
        ((s_ref * ds.to(dt)).sum() + (e_ref * de.to(dt)).sum()).backward()
        return pr, dict(start_logits=s_ref.detach(), end_logits=e_ref.detach(), d_outputs=xr.grad), tap
    pr, o32, tap = oracle(torch.float32)
    pu.assert_pins_ok([('fe%d.z%d' % (ps, i), tap['fe%d.z%d' % (ps, i)], pin['fe%d' % ps][i]) for ps in range(2) for i in range(4)] +
                      [('head.zs', tap['head.zs'], pin['head.hs']), ('head.ze', tap['head.ze'], pin['head.he'])])
    _close('start_logits', s_log.cpu(), o32['start_logits'])
    _close('end_logits', e_log.cpu(), o32['end_logits'])
    # the span argmax on the kernel's own logits (rounding-level differences in the logits may move a near tie)
    si_ref, ei_ref = R.ans_predictor(s_log.cpu(), e_log.cpu(), blk.v_mask)
    assert torch.equal(si.cpu(), si_ref) and torch.equal(ei.cpu(), ei_ref)
    _close('d_outputs', dx.cpu(), o32['d_outputs'])
    _check_param_grads(blk, pr, lambda k: k.startswith('predictor/'))
    return _floor_rows(blk, 'predictor/', dict(start_logits=s_log.cpu(), end_logits=e_log.cpu(), d_outputs=dx.cpu()), oracle(torch.float64)[:2], (pr, o32))


def _gate(cls, blk, rows):
    """gate (b): every tensor's ratio printed, then held to the class's M"""
    for r in rows:
        print('%-8s B%d T%d L%d drop %.1f  %-75s d_hip %.3e  d_32 %.3e  s %.3e  ratio %6.2f' % ((cls, blk.B, blk.T, blk.L, blk.drop) + r))
    assert M[cls] <= CAP
    bad = [r for r in rows if not r[4] <= M[cls]]
    assert not bad, (cls, 'M = %g' % M[cls], bad)


# ---------------------------------------------------------------------------------------------------- block parity per form
@pytest.mark.parametrize('cls,shape,drop', CB_RUNS, ids=_id)
def test_conv_block_fwd_bwd_by_form(cls, shape, drop):
    assert drop in (0.0, DROP)
    blk = make_block(shape, drop)
    _gate(cls, blk, run_cb(blk))


@pytest.mark.parametrize('cls,shape,drop', PRED_RUNS, ids=_id)
def test_predictor_fwd_bwd_by_form(cls, shape, drop):
    assert drop in (0.0, DROP)
    blk = make_block(shape, drop)
    _gate(cls, blk, run_pred(blk))
