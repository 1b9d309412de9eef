"""GPU: every kernel form of the context-query attention (csrc/cq.hip launch_cq_fwd / launch_cq_bwd_impl choose between seven by padded
shape) against the oracle, each case proving in the same test which form it ran (hual_prof_get) - so a change of the dispatch cannot
take a shape off a form without a failing test.

Two gates per case.  The 1e-3 contract of test_gpu_blocks (_oracle_gate), and a gate at the float32 noise floor: the block has no
ReLU, so it is compared with R.cq_attention in float64 (parameters and inputs cast, the same dropout masks), next to the float32
oracle's own distance to float64:  d_hip = max|hip - f64|  <=  M max(d_32, 2^-23 s),  d_32 = max|f32 - f64|, s = max|f64| of the
tensor (feats, dx) or the block's largest parameter gradient (the parameter gradients, as _check_param_grads scales them).

M per class of form: twice the worst ratio d_hip / max(d_32, 2^-23 s) measured on an MI355X over every case and tensor here at three
data seeds (profiles/cq_forms_parity.txt, scripts/cq_forms_parity.py), rounded up to a power of two, and never above a cap that is
not a measurement: 16 for the fp16-pair forms (22-bit operands are 4 float32 rounding units; the rest is for subnormal residuals,
HISTORY.md section 3), 4 for the float32 forms (they differ from the oracle in summation order only).
  fp16 pairs (staged, wide8, wide16, wide64): worst 3.19 (staged B1 T4 L6, dropout on, gradient of v2q_attn linear_kernel4mul, d_hip
    3.4e-5 against d_32 1.1e-5; staged otherwise <= 2.47, wide64 1.68, wide8 / wide16 1.33) -> M = 8.
  float32 (lFlB 2.16, gFgB 1.88, lFgB 1.72, all three at a linear_kernel4mul gradient with d_hip 1.5e-4 .. 1.8e-4 against d_32
    7.8e-5 .. 8.5e-5): the rule gives 8, the cap holds: M = 4, i.e. 1.85 times the worst ratio instead of twice.
The factor two is for the spread of a maximum norm from seed to seed: a (case, tensor) line's largest ratio over the three seeds is
1.5 times its smallest in the median, 5.2 times at most (fp16 pairs; 4.4 float32).  At the data the cases below use (seed 0) the
worst ratios are 1.88 and 1.90."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import parity_util as pu
from oracle import philox as px
from oracle import seqpan_ref as R
from test_gpu_blocks import DROP, OFFSET, SEED, Block
from test_gpu_cq_long_queries import _oracle_gate
from test_gpu_shapes import _check_all

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

_WIDE = lambda a: ('cq_fwd_wide_kernel<%s>' % a, 'cq_bwd_wide_kernel<%s>' % a)
_F32 = ('tri_prep_kernel', 'cq_fwd_kernel', 'cq_bwd_kernel')
# form -> (kernel symbols, each launched once; `cq.gs` in the workspace table; `d.cq.gd` in it; class of the noise-floor gate).  The scratch
# pair is all that tells the three float32 forms apart: score matrices in LDS forward and backward / global backward / global both
FORMS = {'wide8': (_WIDE('8'), False, False, 'f16'), 'wide16': (_WIDE('16'), False, False, 'f16'), 'wide64': (_WIDE('8, 64'), False, False, 'f16'),
         'staged': (('cq_fwd_staged_kernel', 'cq_bwd_staged_kernel'), False, False, 'f16'),
         'lFlB': (_F32, False, False, 'f32'), 'lFgB': (_F32, False, True, 'f32'), 'gFgB': (_F32, True, True, 'f32')}
SYMBOLS = sorted({s for f in FORMS.values() for s in f[0]})
FAMILY = ('cq_fwd_', 'cq_bwd_kernel', 'cq_bwd_staged', 'cq_bwd_wide', 'tri_prep')      # (cq_bwd_pre_kernel belongs to every form)
M = {'f16': 8.0, 'f32': 4.0}

# (B, T, L) at the edges of each form's region of (T, L)
SHAPES = {
    'staged': [(1, 4, 6),                   # one short clip with a longer query: the inference case
               (3, 5, 7), (3, 16, 17),      # N1p = 16 exactly
               (3, 31, 33), (3, 32, 33),    # both sides of the 32-row padding
               (2, 32, 128), (2, 20, 128),  # the longest query
               (3, 33, 34), (2, 48, 49),    # first and last T of the second strip
               (2, 48, 64),                 # the largest LDS footprint
               (9, 12, 20), (8, 12, 20)],   # xcd_round8 with and without idle workgroups
    'lFlB': [(2, 48, 65), (2, 49, 50),      # one word / one frame past the staged form
             (2, 64, 65), (2, 64, 128), (2, 20, 129), (9, 5, 130)],
    'lFgB': [(2, 65, 65), (2, 128, 96),     # the last shape before the forward goes global
             (3, 100, 70)],
    'gFgB': [(2, 128, 97), (2, 97, 97), (2, 33, 129), (2, 129, 33)],      # neighbours across each boundary
    'wide64': [(3, 33, 33), (3, 64, 64), (2, 128, 64),                    # the wide neighbours of the forms above
               (3, 100, 47)],                                             # (test_gpu_cq_long_queries.CQ64_SHAPES[1])
    'wide8': [(5, 100, 30)], 'wide16': [(2, 170, 32)]}                    # (test_gpu_blocks.CQ_WIDE_SHAPES)
CASES = [(form, dict(B=B, T=T, L=L, C=4, seed=500 + 10 * i + k, max_vlen=max(T, L)))
         for i, form in enumerate(SHAPES) for k, (B, T, L) in enumerate(SHAPES[form])]
NO_WIDE_SHAPES = [dict(B=3, T=64, L=20, C=4, seed=581, max_vlen=64), dict(B=3, T=48, L=40, C=4, seed=582, max_vlen=48)]


def _id(v):
    return 'B%d_T%d_L%d' % (v['B'], v['T'], v['L']) if isinstance(v, dict) else str(v)


def _launch(blk, drop, xseed=5):
    """hual_cq_attn_fwd + hual_cq_attn_bwd on random activations (xseed 5: those of test_gpu_cq_long_queries._run_block) between
    hual_prof_begin and hual_prof_end; returns x, dy, feats, dx on the host and {kernel symbol: launches}"""
    lib, l = blk.lib, blk.l
    blk.opts = blk.m._opts(drop)
    x, dy = blk.rand(blk.R, xseed), blk.rand(blk.R, xseed + 1)
    xd, dyd = x.to(blk.dev), dy.to(blk.dev)
    feats, dx = torch.empty_like(xd), torch.empty_like(xd)
    lib.check(l.hual_prof_begin())
    lib.check(l.hual_cq_attn_fwd(*blk.args(), lib.ptr(xd), lib.ptr(feats), *blk.tail()))
    lib.check(l.hual_cq_attn_bwd(*blk.args(), lib.ptr(dyd), lib.ptr(dx), lib.ptr(blk.grads), *blk.tail()))
    n = l.hual_prof_end()
    torch.cuda.synchronize()
    got = {}
    for i in range(n):
        name, cnt = ctypes.create_string_buffer(256), ctypes.c_int64()
        lib.check(l.hual_prof_get(i, name, 256, ctypes.byref(cnt), None, None, None))
        got[name.value.decode()] = int(cnt.value)
    return x, dy, feats.cpu(), dx.cpu(), got


def _form_of(blk, got):
    """the form whose symbols - all of them, once each, and no other symbol of the family - were launched, with its scratch pair"""
    ran = {s: sum(c for k, c in got.items() if k.startswith(s)) for s in SYMBOLS}
    ran = {s: c for s, c in ran.items() if c}
    stray = [k for k in got if k.startswith(FAMILY) and not k.startswith(tuple(SYMBOLS))]
    assert not stray, ('context-query kernels no form lists', stray, got)
    tab = blk.lib.ws_table(blk.m.cfg, blk.B, blk.T, blk.L, blk.C)
    key = (tuple(sorted(ran)), 'cq.gs' in tab, 'd.cq.gd' in tab)
    forms = [f for f, (syms, gs, gd, _) in FORMS.items() if (tuple(sorted(syms)), gs, gd) == key]
    assert len(forms) == 1 and set(ran.values()) == {1}, ('no form launches this', ran, key[1:], got)
    return forms[0]


def _floor_rows(blk, x, dy, feats, dx, drop):
    """[(tensor, d_hip, d_32, s, d_hip / max(d_32, 2^-23 s))] for feats, dx and every parameter gradient of the block"""
    rng = px.DropoutRNG(SEED, OFFSET, drop)
    ref = {}
    for dt in (torch.float64, torch.float32):
        pr = {k: t.detach().clone().to(dt).requires_grad_(True) for k, t in blk.p.items()}
        xr = x.clone().to(dt).requires_grad_(True)
        v, q = blk.split(xr)
        q2v = R.cq_attention(v, q, blk.v_mask, blk.q_mask, pr, 'q2v_attn', rng, px.SITE_TRI + 0, blk.rows_v, px.SITE_TRI + 1, blk.rows_q)
        v2q = R.cq_attention(q, v, blk.q_mask, blk.v_mask, pr, 'v2q_attn', rng, px.SITE_TRI + 2, blk.rows_q, px.SITE_TRI + 3, blk.rows_v)
        out = torch.cat([q2v.reshape(blk.Nv, 128), v2q.reshape(blk.Nq, 128)])
        out.backward(dy.to(dt))
        ref[dt] = dict({'grad ' + k: t.grad.double() for k, t in pr.items() if t.grad is not None}, feats=out.detach().double(), dx=xr.grad.double())
    f64, f32 = ref[torch.float64], ref[torch.float32]
    hg = blk.params_grad()
    hip = dict({k: torch.from_numpy(hg[k[5:]]).double().reshape(f64[k].shape) for k in f64 if k.startswith('grad ')}, feats=feats.double(), dx=dx.double())
    assert len(hip) == 10 and all(k in ('feats', 'dx') or k[5:].startswith(('q2v_attn/', 'v2q_attn/')) for k in hip), sorted(hip)
    gmax = max(float(t.abs().max()) for k, t in f64.items() if k.startswith('grad '))
    rows = []
    for k in sorted(f64):
        d_hip, d_32 = float((hip[k] - f64[k]).abs().max()), float((f32[k] - f64[k]).abs().max())
        s = gmax if k.startswith('grad ') else float(f64[k].abs().max())
        rows.append((k, d_hip, d_32, s, d_hip / max(d_32, 2.0 ** -23 * s)))
    return rows


def _case(form, blk, drop):
    """one parity case: the form that ran, the 1e-3 gate, the gate at the noise floor"""
    x, dy, feats, dx, got = _launch(blk, drop)
    assert _form_of(blk, got) == form, (form, got)
    _oracle_gate(blk, x, dy, feats, dx, drop_on=drop > 0)
    rows = _floor_rows(blk, x, dy, feats, dx, drop)
    for r in rows:
        print('%-7s B%d T%d L%d drop %.1f  %-55s d_hip %.3e  d_32 %.3e  s %.3e  ratio %6.2f' % ((form, blk.B, blk.T, blk.L, drop) + r))
    bad = [r for r in rows if not r[4] <= M[FORMS[form][3]]]
    assert not bad, (form, 'M = %g' % M[FORMS[form][3]], bad)


# ---------------------------------------------------------------------------------------------------- block parity per form
@pytest.mark.parametrize('drop', [0.2, 0.0])
@pytest.mark.parametrize('form,shape', CASES, ids=_id)
def test_cq_attn_fwd_bwd_by_form(form, shape, drop):
    assert drop in (0.0, DROP)
    _case(form, Block(**shape), drop)


def _mask_block(T, L, seed=71):
    """B = 4: a full clip, a 1-frame clip with a one-word query, a 2-frame clip, a clip of 7/12 T frames with a query of L - 2 words
    (as test_gpu_cq_long_queries._mask_case builds them)"""
    cfg, p, wv, b, labels = pu.make_case(B=4, T=T, L=L, C=5, seed=seed, max_vlen=max(T, L))
    lens = np.array([T, 1, 2, 7 * T // 12], dtype=np.int32)
    b['lens'] = torch.tensor(lens)
    for k in range(4):
        b['video'][k, lens[k]:] = 0.0
    b['word_ids'][1, 1:] = 0
    b['char_ids'][1, 1:] = 0
    b['word_ids'][3, :L - 2].clamp_(min=1)
    b['word_ids'][3, L - 2:] = 0
    b['char_ids'][3, L - 2:] = 0
    make, pu.make_case = pu.make_case, lambda **kw: (cfg, p, wv, b, labels)
    try:
        blk = Block()
    finally:
        pu.make_case = make
    assert (blk.T, blk.L) == (T, L) and blk.v_mask.sum(1).tolist() == lens.tolist()
    assert int(blk.q_mask[1].sum()) == 1 and int(blk.q_mask[3].sum()) == L - 2
    return blk


MASK_CASES = [('staged', 12, 20), ('lFlB', 49, 60)]


@pytest.mark.parametrize('drop', [0.2, 0.0])
@pytest.mark.parametrize('form,T,L', MASK_CASES)
def test_cq_attn_mask_paths_by_form(form, T, L, drop):
    _case(form, _mask_block(T, L), drop)


# ---------------------------------------------------------------------------------------------------- the staged kernels with T >= L
_CHILD = '''
import sys, json
import test_gpu_cq_forms as t
t._no_wide_child(json.loads(sys.argv[1]))
'''


def _no_wide_child(shape):
    for drop in (0.2, 0.0):
        _case('staged', Block(**shape), drop)


@pytest.mark.parametrize('shape', NO_WIDE_SHAPES, ids=_id)
def test_staged_kernels_with_the_clip_as_the_long_side(shape):
    """the orientation in which the staged kernels served the short queries before csrc/cqwide.hip: HUAL_CQ_NO_WIDE=1 (read once per
    process, so a fresh child process per shape; it asserts the symbols and both gates itself)"""
    env = dict(os.environ, HUAL_CQ_NO_WIDE='1', PYTHONPATH=os.pathsep.join([HERE, os.path.dirname(HERE)] + [q for q in sys.path if q]))
    r = subprocess.run([sys.executable, '-c', _CHILD, json.dumps(shape)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    print(r.stdout.decode()[-6000:])
    assert r.returncode == 0


# ---------------------------------------------------------------------------------------------------- whole model, graph replay
@pytest.mark.parametrize('shape', [dict(B=2, T=12, L=20, C=5, seed=95, max_vlen=32),       # staged
                                   dict(B=2, T=64, L=96, C=5, seed=96, max_vlen=96)],      # lFlB
                         ids=_id)
def test_whole_model_queries_longer_than_the_clip(shape):
    """more query rows than video rows in the unified row space; the pool_align_bwd instantiations for these lengths"""
    _check_all(pu.make_case(**shape), 0.2)


def test_steps_with_queries_longer_than_the_clip_replay_bit_identical_to_eager():
    """the pattern of test_gpu_cq_long_queries.test_steps_with_long_queries_replay_bit_identical_to_eager at two staged shapes"""
    from hual_amd.train import Trainer
    cases = [pu.make_case(B=4, T=12, L=L, C=8, seed=400 + L, max_vlen=32, vdim=64) for L in (20, 24)]
    m = pu.hip_model(*cases[0][:3])
    assert m.ws_poison == 0xFF
    tr = Trainer(m, world=1, use_graph=True)
    tr.reserve(4, 12, 24, 8)
    dev = m.device
    feeds = []
    for cfg, p, wv, b, labels in cases:
        feeds.append(dict(video=b['video'].to(dev), video_seq_len=b['lens'].to(torch.int32).to(dev), word_ids=b['word_ids'].to(torch.int32).to(dev),
                          char_ids=b['char_ids'].to(torch.int32).to(dev), y1=labels[0].float().to(dev), y2=labels[1].float().to(dev),
                          match_labels=labels[2].to(torch.int32).to(dev), inner_labels=labels[3].float().to(dev)))
    p0 = m.params.clone()
    runs = []
    for pas in range(3):                                          # eager / captured / replayed
        before = dict(tr.stats)
        out = []
        for k, f in enumerate(feeds):
            m.set_rng(777, k)
            tr.set_batch_device(f)
            tr.step(lr=0.0, drop_rate=0.2)
            B = tr.shape[0]
            out.append((tr.loss_terms.clone(), tr.start_logits.clone(), tr.end_logits.clone(), tr.spans[:, :B].clone()))
        runs.append((out, {k: tr.stats[k] - before[k] for k in before}))
    torch.cuda.synchronize()
    assert runs[0][1]['eager'] == 2 and runs[1][1]['captured'] == 2 and runs[2][1]['replayed'] == 2, [r[1] for r in runs]
    assert torch.equal(m.params, p0)
    for pas in (1, 2):
        for a, b in zip(runs[0][0], runs[pas][0]):
            for x, y in zip(a, b):
                assert torch.equal(x, y)
    assert all(torch.isfinite(o[0]).all() for o in runs[2][0])
