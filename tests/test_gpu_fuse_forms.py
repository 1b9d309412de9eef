"""GPU: every form of the fuse stage and of the loss end (csrc/seqpan.hip fwd_fuse / bwd_fuse and the close of the loss, csrc/heads.hip
with the two mproj launches around it) against the oracle, through hual_fuse_fwd / hual_fuse_bwd - the one labelled per-block entry point -
and hual_localizing_loss, each case proving in the same test which kernels it ran (hual_prof_get), so a change of the dispatch cannot take
a shape off a form without a failing test.  The dispatch is restated below; tests/test_fuse_dispatch.py (no GPU) holds the case table to
every class and switch point named here and the restated constants to the sources.

What chooses a form (shapes and options, never the data).  Forward: pool_align_fwd_kernel (one launch, the alignment pooling as a second
grid row when labels are given), cq_concat as mproj_kernel<NT, 8> - the addend form, the addend (pooled . W_bot) indexed by row / T, NT
from mproj_rows(Nv): 16 rows per workgroup up to Nv 4096, two row tiles up to 8192, three up to 12288, four beyond -, the matching head
in match_align_fwd_kernel (grid min(ceil(Nv / 8), 512): a grid-stride loop from Nv > 4096; the rows of the [B, B] alignment similarity
as further workgroups unless align_external) and loss_tail_kernel unless the close is deferred.  Backward: zero_kernel, match_bwd_kernel
(grid min(ceil(Nv / 8), 256): loops from Nv > 2048, one row prefetched ahead and clamped to Nv - 1; closes the loss itself when
deferred), cq_concat^T as mproj_kernel<NT, 0>, pool_align_bwd_kernel<KT, KL> (KT 32 up to T 128, else 64; KL 8 / 16 / 32 / 64 up to L 32 /
64 / 128 / 256; L > 128 takes <64, 64> whatever T: seven instantiations), and the two weight-gradient jobs and the matching head's
partial sums through dw_table_write_kernel, dw_f16_balanced_kernel and colsum_kernel.  With align_external the test runs
hual_align_loss_rows between the two calls into d.align.that / d.align.vhat as the trainer's data-parallel step does
(align_sim_rows_kernel, align_sim_cols_kernel), reads the two buffers back and hands the oracle those very gradients.

The oracle is the reference's own cq_concat, align_pool, align_loss_from_pooled and the matching block of R.forward (its lines restated
in `compose`, gumbel branch included) in the order R.forward uses; at float32 it is R.forward's fuse / outputs / match_scores / t_hat /
v_hat taps and its match, align and total loss bit for bit (prove_composition; also run without a GPU by test_fuse_dispatch.py).  The
localizing term enters as the caller's loc_part [B], as it does in the kernels.

Three gates per case.  (i) the exact {kernel symbol: launches} of the two calls.  (ii) the 1e-3 contract: _close on outputs, the scores,
d cq.feats and the four loss terms, _check_param_grads on the stage's six parameter tensors (exactly those reached, nothing else
non-zero).  (iii) the float32 noise floor: d_hip = max|hip - f64|  <=  M max(d_32, 2^-23 s),  d_32 = max|f32 oracle - f64 oracle|,
s = max|f64| of the tensor (d cq.feats: video rows and query rows apart, so that the query rows - pooling and alignment - are not
measured against the scale of d outputs); parameter gradients: s = the stage's largest gradient, as _check_param_grads scales them;
reduced scalars (the four loss terms, loc_part): s = the sum of the absolute values of the reduced terms in the float64 oracle.
Every labelled case but the dead-clip one asserts that v_hat is non-zero for every clip: the labels are built so (make_case).  The
`align` class runs with d outputs = 0, so that the alignment's own gradient is a visible share of d cq.feats.  At B = 1 the reference's
alignment term is -2, not 0 (the reference hands kl_for_log_probs a probability where a log-probability belongs; the oracle keeps
that), its gradient is 0; the kernel returns exactly -2.

M per class: twice the worst ratio measured on an MI355X over every case and tensor of the class at three data seeds
(profiles/fuse_forms_parity.txt, scripts/fuse_forms_parity.py), rounded up to a power of two, never above 16 - a condition.
Worst ratio per class (case, seed, tensor, d_hip against d_32) -> M:
  pab    2.37 (B2 T100 L129, seed 0, the query rows of d cq.feats, 2.1e-6 against 8.7e-7) -> 8
  clamp  2.70 (B3 T1 L1, seed 0, gradient of cq_cat/dense/kernel, 4.6e-6 against 1.2e-6) -> 8
  grid   1.38 (B1 T5 L3, seed 1, the same gradient, 4.5e-6 against 3.2e-6) -> 4
  tiles  2.00 (B49 T256 L4, seed 1, the same gradient, 4.3e-4 against 2.2e-4; 1.77 in another run of the table: the weight-gradient
         launch's summation order is not fixed) -> 4
  loss   1.48 (deferred close, seed 1, gradient of cq_cat/weighted_pooling/weight, 2.6e-5 against 1.8e-5) -> 4
  align  1.75 .. 1.86 (B5 at d outputs = 0, seed 0, the same gradient - float atomics over the clips -, 1.2e-7 against 6.4e-8) -> 4
  alone  1.40 (B2 T100 L129, seed 2, the query rows of d cq.feats, 1.8e-10 against 1.3e-10) -> 4
  loc    1.63 (T 129, seed 2, de, 3.6e-8 against 8.9e-9) -> 4
No ratio exceeds 3, so none is a finding about the kernels, and no class comes near the cap.  outputs and the scores stay below 1.2,
the four loss terms below 1.7 (total), 1.41 (align), 0.97 (match) and 0.71 (loc), d cq.feats below 2.0 (video rows) and 2.4 (query
rows); the restated dispatch predicted every launch of all 44 cases at all three seeds, mproj_kernel<3, 8>, <4, 8> and the seven pool_align_bwd_kernel instantiations among them.  A case takes 0.01 .. 0.4 s of
test time (the first one pays the library's start; B49 T256: 0.17 s), the file 4 s.
What the gates see (scratch builds, arithmetic only, nothing committed).
(b) The addend row of a 16-row tile's first row for all of its rows, in every instantiation: 28 of the 39 cases of the first six classes
(`alone` came after these runs) fail - every case with more than one clip and T no multiple of 16 -, all of them already at gate (ii) on `outputs` (errors of 0.5 .. 0.9 of the tensor's
scale); so do 24 of the 80 older tests of test_gpu_blocks / test_gpu_model / test_gpu_shapes.  Confined to the instantiations no
test ran before (NT >= 3), exactly B33 T250 (<3, 8>) and B49 T256 (<4, 8>) of those 39 fail, again at gate (ii), the B32 / B48 T256 cases on the
same instantiations - whole clips per tile - pass, and all 80 older tests pass.
(a) The two l2-normalisation differences of pool_align_bwd_kernel in float instead of double: no gate fails in any of the 44 cases at
any of the three seeds, nor in the 80 older tests, and no ratio moves beyond its run-to-run noise - not even in the `alone` class, where d cq.feats is that gradient and nothing
else (its rows move by 1e-10 of 1e-3, up as often as down; worst ratio 1.40 with and without the mutation).  At random cq.feats t_hat
and its gradient are nearly orthogonal, so the difference does not cancel and float32 holds it to an ulp; and the float32 oracle evaluates
the same difference in float32, so its error is part of d_32 whatever the inputs: a gate against d_32 cannot ask for more than float32
PyTorch delivers.  The double arithmetic there is for trained features, which nothing here measures.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import parity_util as pu
from oracle import philox as px
from oracle import seqpan_ref as R
from test_gpu_blocks import DROP, OFFSET, SEED, Block, _check_param_grads, _close
from test_gpu_cb_forms import CAP, _assert_form
from test_gpu_da_bwd_fused import _prof
from test_gpu_da_forms import _cdiv

pytestmark = pytest.mark.gpu

M = {'pab': 8.0, 'clamp': 8.0, 'grid': 4.0, 'tiles': 4.0, 'loss': 4.0, 'align': 4.0, 'alone': 4.0, 'loc': 4.0}

# the tensors of the stage, by their names in the flat layout
STAGE = ['cq_cat/weighted_pooling/weight', 'cq_cat/dense/kernel', 'cq_cat/dense/bias', 'matching_loss/dense/kernel', 'matching_loss/dense/bias',
         'label_emb']
TERMS = ('loss', 'loc_loss', 'match_loss', 'align_loss')


# ---------------------------------------------------------------------------------------------------- the dispatch, restated
MP_ROWS = 64                               # csrc/mproj.hip
MPF_ADD = 8                                # csrc/mproj.h: the addend form's feature-set literal
MATCH_FWD_CAP, MATCH_BWD_CAP = 512, 256    # csrc/heads.hip match_fwd_blocks / match_bwd_blocks
PAB_T, PAB_L = 128, (32, 64, 128)          # csrc/heads.hip launch_pool_align_bwd: the switch points of KT / KL
PAB_FORMS = [(32, 8), (32, 16), (32, 32), (64, 8), (64, 16), (64, 32), (64, 64)]


def mproj_rows(R0):
    """csrc/mproj.hip mproj_rows of one problem: rows per workgroup"""
    t = 16
    while t < MP_ROWS and _cdiv(R0, t) > 256:
        t += 1
    return t


def mproj_nt(mt):
    """the NT of mproj_kernel<NT, F>: 16-row tiles of a workgroup, at least two"""
    return min(max(_cdiv(mt, 16), 2), 4)


def rowgrid(rows, cap):
    """csrc/heads.hip rowgrid: workgroups of eight rows, capped (a grid-stride loop beyond)"""
    return min(max(_cdiv(rows, 8), 1), cap)


def pab_form(T, L):
    """csrc/heads.hip launch_pool_align_bwd: (KT, KL) - rows per thread of the video / query side"""
    if L > PAB_L[2]:
        return 64, 64
    return (32 if T <= PAB_T else 64), (8 if L <= PAB_L[0] else 16 if L <= PAB_L[1] else 32)


def fuse_form(sp):
    """everything that chooses a code path of the stage"""
    B, T, L = sp['B'], sp['T'], sp['L']
    Nv = B * T
    mt = mproj_rows(Nv)
    return dict(Nv=Nv, mt=mt, nt=mproj_nt(mt), straddle=T % mt != 0, pab=pab_form(T, L), fwd_grid=rowgrid(Nv, MATCH_FWD_CAP),
                bwd_grid=rowgrid(Nv, MATCH_BWD_CAP), fwd_loops=_cdiv(Nv, 8) > MATCH_FWD_CAP, bwd_loops=_cdiv(Nv, 8) > MATCH_BWD_CAP,
                labels=sp['labels'], ext=sp['ext'], deferred=sp['deferred'], gumbel=sp['gumbel'], denom=sp['denom'] > 0)


def fuse_dispatch(sp):
    """{kernel symbol: launches} of hual_fuse_fwd (+ hual_fuse_bwd with labels): every launch of the calls"""
    f = fuse_form(sp)
    want = {'pack_weights_kernel': 1, 'pool_align_fwd_kernel': 1, 'mproj_kernel<%d, %d>' % (f['nt'], MPF_ADD): 1, 'match_align_fwd_kernel': 1}
    if not f['labels']:
        return want
    if not f['deferred']:
        want['loss_tail_kernel'] = 1
    if f['ext']:
        want.update({'align_sim_rows_kernel': 1, 'align_sim_cols_kernel': 1})      # the caller's hual_align_loss_rows between the calls
    want.update({'zero_kernel': 1, 'match_bwd_kernel': 1, 'mproj_kernel<%d, 0>' % f['nt']: 1, 'pool_align_bwd_kernel<%d, %d>' % f['pab']: 1,
                 'dw_table_write_kernel': 1, 'dw_f16_balanced_kernel': 1, 'colsum_kernel': 1})
    return want


# (class of the noise-floor gate, what it is there for, [case]).  A case: B, T, L and the loss form - labels (False: inference, forward
# only), ext (align_external), deferred (the backward closes the loss), gumbel (loss.no_gumbel false, tau 0.7), drop (the rate in the
# options: the stage has no dropout site, the gumbel draws share the rng state), denom (match_denom_override), dscale (scale of the
# two parts of d outputs), edge ('dead': clip 1 without an inner label; 'one': clip 1 with one valid frame and a one-word query), lam
# (loss.match_lambda)
def _c(B=3, T=37, L=9, labels=True, ext=False, deferred=False, gumbel=False, drop=0.0, denom=0.0, dscale=1.0, edge=None, lam=1.0):
    return dict(B=B, T=T, L=L, labels=labels, ext=ext, deferred=deferred, gumbel=gumbel, drop=drop, denom=denom, dscale=dscale, edge=edge, lam=lam)


TAU = 0.7
FUSE_TABLE = [
    ('pab', 'every pool_align_bwd instantiation, both sides of T 128|129 and of L 32|33, 64|65, 128|129',
     [_c(B=2, T=128, L=32), _c(B=2, T=128, L=33), _c(B=2, T=100, L=64), _c(B=2, T=100, L=65), _c(B=2, T=128, L=128), _c(B=2, T=100, L=129),
      _c(B=2, T=129, L=32), _c(B=2, T=256, L=33), _c(B=2, T=256, L=65), _c(B=2, T=256, L=128), _c(B=2, T=200, L=256), _c(B=2, T=256, L=256)]),
    ('clamp', 'the row clamps min(grp + 4 k, T - 1): T and L below 4, and no multiples of 4',
     [_c(T=3, L=2), _c(T=1, L=1), _c(T=5, L=3), _c(T=6, L=7), _c(T=37, L=9)]),
    ('grid', 'matching-head grids: fewer than eight rows, a ragged last workgroup, the first stride step of either loop with Nv % 8 != 0',
     [_c(B=1, T=5, L=3), _c(B=5, T=13, L=4), _c(B=8, T=256, L=4), _c(B=17, T=121, L=4), _c(B=16, T=256, L=4), _c(B=33, T=125, L=4)]),
    ('tiles', 'cq_concat tiles: two, three and four row tiles, both sides of Nv 8192|8193.. and 12288|12289.., tiles that straddle clips',
     [_c(B=17, T=241, L=4), _c(B=32, T=256, L=4), _c(B=33, T=250, L=4), _c(B=48, T=256, L=4), _c(B=49, T=256, L=4)]),
    ('loss', 'inference; align_external; gumbel with and without a dropout rate; a denominator override; the deferred close',
     [_c(labels=False), _c(ext=True), _c(gumbel=True, drop=DROP), _c(gumbel=True), _c(denom=37.5), _c(deferred=True),
      _c(deferred=True, ext=True, gumbel=True, drop=DROP)]),
    ('align', 'alignment edges at d outputs = 0: B 1, 2, 5, 6 (the column loop strides by 4), a dead clip (the eps branch), one frame / one word',
     [_c(B=1, dscale=0.0), _c(B=2, dscale=0.0), _c(B=5, dscale=0.0), _c(B=6, dscale=0.0), _c(B=3, dscale=0.0, edge='dead'),
      _c(B=3, dscale=0.0, edge='one')]),
    ('alone', 'the alignment gradient alone: d outputs = 0 and match_lambda = 0, so d cq.feats is the alignment term\'s and nothing else\'s',
     [_c(B=2, dscale=0.0, lam=0.0), _c(B=3, dscale=0.0, lam=0.0), _c(B=5, dscale=0.0, lam=0.0), _c(B=2, T=100, L=129, dscale=0.0, lam=0.0),
      _c(B=3, dscale=0.0, lam=0.0, ext=True)]),
]
FUSE_CASES = [(cls, dict(sp, seed=1700 + 20 * i + k)) for i, (cls, _, cases) in enumerate(FUSE_TABLE) for k, sp in enumerate(cases)]


def _id(v):
    if not isinstance(v, dict):
        return str(v)
    return 'B%d_T%d_L%d%s%s%s%s%s%s%s%s' % (v['B'], v['T'], v['L'], '' if v['labels'] else '_infer', '_ext' if v['ext'] else '',
                                          '_deferred' if v['deferred'] else '', '_gumbel' if v['gumbel'] else '', '_drop%g' % v['drop'] if v['drop'] else '',
                                          '_denom%g' % v['denom'] if v['denom'] else '', '' if v['dscale'] else '_dout0', ('_' + v['edge'] if v['edge'] else '') + ('' if v['lam'] == 1.0 else '_lam%g' % v['lam']))


# ---------------------------------------------------------------------------------------------------- one case
def make_case(sp):
    """(cfg, p, wv, batch, labels) for the case.  The stage reads the masks and the labels only: clips of (T + 1) // 2 .. T frames and
    queries of 1 .. L words (one of each at full length), match labels uniform on 0 .. 3, inner labels 0 / 1 with at least one 1 among
    the valid frames of every clip - so that v_hat is non-zero, which pu.make_case does not guarantee at small T - and none beyond"""
    B, T, L, C = sp['B'], sp['T'], sp['L'], 4
    cfg, p, wv, _, _ = pu.make_case(B=2, T=8, L=3, C=C, seed=1, max_vlen=max(T, L, 8), vdim=64)
    cfg = R.Cfg(dict(cfg, no_gumbel=not sp['gumbel'], tau=TAU, match_lambda=sp['lam']))
    g = np.random.default_rng(sp['seed'])
    lens = g.integers((T + 1) // 2, T + 1, size=B)
    qlens = g.integers(1, L + 1, size=B)
    lens[g.integers(0, B)], qlens[g.integers(0, B)] = T, L
    if sp['edge'] == 'one':
        lens[0], qlens[0], lens[1], qlens[1] = T, L, 1, 1
    word_ids, char_ids = np.zeros((B, L), dtype=np.int32), np.zeros((B, L, C), dtype=np.int32)
    match, inner = g.integers(0, 4, size=(B, T)).astype(np.int32), np.zeros((B, T), dtype=np.float32)
    for k in range(B):
        word_ids[k, :qlens[k]] = g.integers(1, cfg.num_words, size=qlens[k])
        char_ids[k, :qlens[k], 0] = g.integers(1, cfg.num_chars, size=qlens[k])
        inner[k, :lens[k]] = g.integers(0, 2, size=lens[k])
        inner[k, g.integers(0, lens[k])] = 1.0
    if sp['edge'] == 'dead':
        inner[1] = 0.0
    b = dict(video=torch.zeros(B, T, cfg.vdim), lens=torch.tensor(lens, dtype=torch.int32), word_ids=torch.tensor(word_ids),
             char_ids=torch.tensor(char_ids))
    zero = torch.zeros(B, T)
    return cfg, p, wv, b, (zero, zero, torch.tensor(match), torch.tensor(inner))


def make_block(sp):
    blk = Block(drop=sp['drop'], case=make_case(sp))
    blk.sp = sp
    assert (blk.B, blk.T, blk.L) == (sp['B'], sp['T'], sp['L'])
    return blk


def compose(pr, cfg, feats, v_mask, q_mask, labels, loc_part, seed, offset, ext=None, denom=None):
    """the stage in the order of R.forward (its lines 612-648) on the parameters pr and cq.feats `feats` [B (T + L), 128] (their dtype).
    labels: (match_labels, inner_labels) or None; loc_part [B]: the localizing loss' per-clip terms; ext: (d t_hat, d v_hat) - the
    alignment term is then the caller's (reported as 0, its gradients given); denom: the matching loss' denominator override.
    Returns the tensors, the loss terms, `obj_loss` (what the backward differentiates beside d outputs) and, per loss term, the sum of the
    absolute values of its reduced terms"""
    dt = feats.dtype
    (B, T), L = v_mask.shape, q_mask.shape[1]
    Nv = B * T
    q2v, v2q = feats[:Nv].reshape(B, T, -1), feats[Nv:].reshape(B, L, -1)
    fuse = R.cq_concat(q2v, v2q, q_mask, pr, 'cq_cat')
    o = dict(fuse=fuse)
    if labels is not None:
        match_labels, inner_labels = labels
        t_hat, v_hat = R.align_pool(v2q, q2v, q_mask, v_mask, inner_labels.to(dt))
        o.update(t_hat=t_hat, v_hat=v_hat)
    logits4 = R.conv1d(fuse, pr, 'matching_loss/dense')
    if not getattr(cfg, 'no_gumbel', True):
        u = torch.from_numpy(px.gumbel_uniform(seed, offset, np.arange(Nv))).to(dt).reshape(B, T, 4)
        noise = -torch.log(-torch.log(u + 1e-20) + 1e-20)
        logits4 = (logits4 + noise) / cfg.tau
    match_scores = torch.softmax(logits4, dim=-1)
    E = pr['label_emb']
    soft = match_scores @ E
    outputs = (fuse + soft) * v_mask.unsqueeze(-1).to(dt)
    o.update(match_scores=match_scores, outputs=outputs)
    if labels is None:
        return o
    onehot = torch.nn.functional.one_hot(match_labels.long(), 4).to(dt)
    per = -(onehot * torch.log_softmax(logits4, dim=-1)).sum(-1)
    m = v_mask.to(dt)
    den = (m.sum() + 1e-12) if denom is None else denom
    match_ce = (per * m).sum() / den
    ortho = torch.linalg.norm((E @ E.t()) * (1.0 - torch.eye(4, dtype=dt)))
    match_loss = match_ce + ortho
    loc_loss = loc_part.to(dt).sum()
    if ext is None:
        align = R.align_loss_from_pooled(t_hat, v_hat)
        obj_align = align
        vs, qs = torch.softmax((v_hat @ v_hat.t()).detach(), dim=-1), torch.softmax((t_hat @ v_hat.t()).detach(), dim=-1)
        s_align = float((qs * torch.log(qs)).abs().sum() + (vs * torch.log(vs)).abs().sum() + 2.0 * (qs * vs).abs().sum())
    else:
        align = torch.zeros((), dtype=dt)
        obj_align = (t_hat * ext[0].to(dt)).sum() + (v_hat * ext[1].to(dt)).sum()
        s_align = 0.0
    loss = loc_loss + cfg.match_lambda * match_loss + align * 1.0
    s_loc, s_match = float(loc_part.to(dt).abs().sum()), float(((per * m).abs().sum() / den + ortho.abs()).detach())
    o.update(loss=loss, loc_loss=loc_loss, match_loss=match_loss, align_loss=align, obj_loss=cfg.match_lambda * match_loss + obj_align,
             s_terms=dict(loss=s_loc + cfg.match_lambda * s_match + s_align, loc_loss=s_loc, match_loss=s_match, align_loss=s_align))
    return o


def prove_composition():
    """float32, with and without the gumbel branch: the composition on R.forward's own cq.feats is R.forward's fuse / outputs /
    match_scores / t_hat / v_hat taps and its match, align and total loss, bit for bit"""
    for gumbel in (False, True):
        cfg, p, wv, b, labels = pu.make_case(B=3, T=20, L=6, C=5, seed=3, vdim=64)
        cfg = R.Cfg(dict(cfg, no_gumbel=not gumbel, tau=TAU))
        out = R.forward(p, cfg, wv, b['video'], b['lens'], b['word_ids'], b['char_ids'], drop_rate=DROP, seed=SEED, offset=OFFSET, labels=labels, want_tap=True)
        tap = out['tap']
        (B, T), L = b['video'].shape[:2], b['word_ids'].shape[1]
        feats = torch.cat([tap['q2v'].reshape(B * T, -1), tap['v2q'].reshape(B * L, -1)])
        v_mask = (torch.arange(T).unsqueeze(0) < b['lens'].long().unsqueeze(1)).to(torch.int32)
        o = compose(p, cfg, feats, v_mask, (b['word_ids'] != 0).to(torch.int32), labels[2:], out['loc_loss'].reshape(1), SEED, OFFSET)
        for k, ref in (('fuse', tap['fuse']), ('outputs', tap['outputs']), ('match_scores', out['match_scores']), ('t_hat', tap['t_hat']),
                       ('v_hat', tap['v_hat']), ('match_loss', out['match_loss']), ('align_loss', out['align_loss']), ('loss', out['loss'])):
            assert torch.equal(o[k], ref), (gumbel, k)


def _ratio(d_hip, d_32, s):
    """d_hip / max(d_32, 2^-23 s); an exact result (d_hip = 0) is at ratio 0 whatever the floor"""
    return 0.0 if d_hip == 0.0 else d_hip / max(d_32, 2.0 ** -23 * s, 1e-300)


def run_fuse(blk, xseed=9):
    """hual_fuse_fwd (+ hual_fuse_bwd) on random cq.feats, d outputs and loc_part; gates (i) and (ii) asserted; returns
    (rows of gate (iii): [(tensor, d_hip, d_32, s, ratio)], the four loss terms as the kernels wrote them)"""
    lib, l, sp, m = blk.lib, blk.l, blk.sp, blk.m
    B, Nv, dev = blk.B, blk.Nv, blk.dev
    feats, d1, d2 = blk.rand(blk.R, xseed), blk.rand(Nv, xseed + 1, sp['dscale']), blk.rand(Nv, xseed + 2, sp['dscale'])
    loc = torch.rand(B, generator=torch.Generator().manual_seed(xseed + 3)) * 2.0 / B
    fd, d1d, d2d, locd = feats.to(dev), d1.to(dev), d2.to(dev), loc.to(dev)
    outputs, dfeats = torch.empty(Nv, 128, device=dev), torch.empty(blk.R, 128, device=dev)
    scores = torch.empty(Nv, 4, device=dev)
    terms, dterms = torch.full((4,), float('nan'), device=dev), torch.full((4,), float('nan'), device=dev)
    blk.opts = m._opts(sp['drop'], match_denom=sp['denom'], align_external=1 if sp['ext'] else 0)
    if sp['deferred']:
        blk.opts.deferred_loss_terms = dterms.data_ptr()
    lab_st, lab_keep = m._labels(*blk.labels) if sp['labels'] else (None, None)
    lab = ctypes.byref(lab_st) if sp['labels'] else None
    ext_loss = torch.zeros(1, device=dev)
    ext_scratch = torch.empty(2 * B * B + B, device=dev)

    def call():
        lib.check(l.hual_fuse_fwd(*blk.args(), lab, lib.ptr(fd), lib.ptr(locd) if sp['labels'] else None, lib.ptr(outputs), lib.ptr(scores),
                                  lib.ptr(terms), *blk.tail()))
        if not sp['labels']:
            return
        if sp['ext']:      # the [B, B] part outside, into the workspace buffers the backward reads: hual_amd/train.py _dp_part_b at world size 1
            tv = m.tap('align.tv')
            lib.check(l.hual_align_loss_rows(lib.ptr(tv), ctypes.c_void_p(tv.data_ptr() + 128 * 4), 256, B, 0, B, lib.ptr(ext_scratch),
                                             lib.ptr(m.tap('d.align.that')), lib.ptr(m.tap('d.align.vhat')), lib.ptr(ext_loss), 1.0, lib.stream_ptr()))
        lib.check(l.hual_fuse_bwd(*blk.args(), lab, lib.ptr(d1d), lib.ptr(d2d), lib.ptr(dfeats), lib.ptr(blk.grads), *blk.tail()))
    _assert_form(_prof(lib, l, call), '', fuse_dispatch(sp))
    ext = (m.tap('d.align.that').cpu().clone(), m.tap('d.align.vhat').cpu().clone()) if sp['ext'] else None
    hip = dict(outputs=outputs.cpu(), match_scores=scores.cpu(), dfeats=dfeats.cpu(), ext_loss=ext_loss.cpu())
    got_terms = (dterms if sp['deferred'] else terms).cpu()
    assert bool(torch.isnan(terms if sp['deferred'] or not sp['labels'] else dterms).all())      # the other buffer is not written
    return judge(blk, (feats, d1, d2, loc), hip, ext, got_terms, blk.params_grad), got_terms if sp['labels'] else None


def judge(blk, inputs, hip, ext, got_terms, params_grad):
    """gate (ii) asserted on what the kernels returned; the rows of gate (iii)"""
    sp, Nv = blk.sp, blk.Nv
    feats, d1, d2, loc = inputs
    dfeats, ext_loss = hip.pop('dfeats'), hip.pop('ext_loss')

    def oracle(dt):
        pr = {k: t.detach().clone().to(dt).requires_grad_(True) for k, t in blk.p.items()}
        fr = feats.detach().clone().to(dt).requires_grad_(True)
        o = compose(pr, blk.cfg, fr, blk.v_mask, blk.q_mask, blk.labels[2:] if sp['labels'] else None, loc, SEED, OFFSET, ext,
                    sp['denom'] if sp['denom'] > 0 else None)
        res = dict(outputs=o['outputs'].detach().reshape(Nv, 128), match_scores=o['match_scores'].detach().reshape(Nv, 4))
        if sp['labels']:
            (o['obj_loss'] + (o['outputs'].reshape(Nv, 128) * (d1 + d2).to(dt)).sum()).backward()
            res.update({'d cq.feats[v]': fr.grad[:Nv], 'd cq.feats[q]': fr.grad[Nv:]}, **{k: o[k].detach() for k in TERMS})
        return pr, res, o
    pr, o32, full32 = oracle(torch.float32)
    for k in ('outputs', 'match_scores'):
        _close(k, hip[k], o32[k])
    if not sp['labels']:
        p64, o64, _ = oracle(torch.float64)
        return _rows(hip, o64, o32, {}, {}, 0.0)
    vn = full32['v_hat'].detach().norm(dim=1)
    assert bool((vn > 0.5).all()) if sp['edge'] != 'dead' else (float(vn[1]) == 0.0 and float(vn[0]) > 0.5 and float(vn[2]) > 0.5), vn
    hip.update({'d cq.feats[v]': dfeats[:Nv], 'd cq.feats[q]': dfeats[Nv:]}, **{k: got_terms[i] for i, k in enumerate(TERMS)})
    _close('d cq.feats', dfeats, torch.cat([o32['d cq.feats[v]'], o32['d cq.feats[q]']]))
    for k in TERMS:
        _close(k, hip[k], o32[k])
    if sp['ext']:
        _close('external align loss', ext_loss, R.align_loss_from_pooled(full32['t_hat'], full32['v_hat']).detach())
    reached = sorted(k for k, t in pr.items() if t.grad is not None)
    assert reached == sorted(STAGE), reached
    _check_param_grads(blk, pr, lambda k: k in reached)
    p64, o64, full64 = oracle(torch.float64)
    hg = params_grad()
    gmax = max(float(p64[k].grad.abs().max()) for k in STAGE)
    return _rows(hip, o64, o32, {k: (torch.from_numpy(hg[k]), p64[k].grad, pr[k].grad) for k in STAGE}, full64['s_terms'], gmax)


def _rows(hip, o64, o32, grads, s_terms, gmax):
    rows = []
    for k in sorted(o64):
        h, a, b = hip[k].double().reshape(-1), o64[k].double().reshape(-1), o32[k].double().reshape(-1)
        d_hip, d_32 = float((h - a).abs().max()), float((b - a).abs().max())
        s = s_terms[k] if k in s_terms else float(a.abs().max())
        rows.append((k, d_hip, d_32, s, _ratio(d_hip, d_32, s)))
    for k in sorted(grads):
        h, a, b = (t.double().reshape(-1) for t in grads[k])
        d_hip, d_32 = float((h - a).abs().max()), float((b - a).abs().max())
        rows.append(('grad ' + k, d_hip, d_32, gmax, _ratio(d_hip, d_32, gmax)))
    assert all(math.isfinite(r[1]) for r in rows), rows
    return rows


def _gate(cls, name, rows):
    """gate (iii): every tensor's ratio printed, then held to the class's M"""
    for r in rows:
        print('%-6s %s  %-40s d_hip %.3e  d_32 %.3e  s %.3e  ratio %6.2f' % ((cls, name) + r))
    assert M[cls] <= CAP
    bad = [r for r in rows if not r[4] <= M[cls]]
    assert not bad, (cls, 'M = %g' % M[cls], bad)


# ---------------------------------------------------------------------------------------------------- stage parity per form
@pytest.mark.parametrize('cls,sp', FUSE_CASES, ids=_id)
def test_fuse_fwd_bwd_by_form(cls, sp):
    rows, _ = run_fuse(make_block(sp))
    _gate(cls, _id(sp), rows)


def test_forward_closed_and_deferred_loss_are_the_same_bits():
    """both closes run loss_tail_body on the same partial sums: the four terms are bit-equal"""
    sp = [sp for _, sp in FUSE_CASES if sp['deferred'] and not sp['ext']][0]
    _, deferred = run_fuse(make_block(sp))
    _, closed = run_fuse(make_block(dict(sp, deferred=False)))
    assert torch.equal(deferred, closed) and bool(torch.isfinite(closed).all()), (deferred, closed)


def test_backward_without_labels_is_refused():
    """a label-free backward would run pool_align_bwd on alignment buffers nobody wrote: an error code, no launch"""
    blk = make_block(FUSE_CASES[0][1])
    lib, l = blk.lib, blk.l
    x = torch.zeros(blk.R, 128, device=blk.dev)

    def call():
        with pytest.raises(lib.HualError):
            lib.check(l.hual_fuse_bwd(*blk.args(), None, lib.ptr(x), lib.ptr(x), lib.ptr(x), lib.ptr(blk.grads), *blk.tail()))
    assert _prof(lib, l, call) == {}


def test_composition_is_the_reference_forward():
    prove_composition()


# ---------------------------------------------------------------------------------------------------- the localizing loss on its own
LOC_T = [1, 5, 128, 129, 256]
LOC_B = 5


def loc_case(T, seed):
    """ragged clips (one of length T, one of one frame), logits of a few units, soft labels whose rows sum to 0.2 .. 3 - the kernel
    multiplies the softmax by the row sums, and the span-posterior training feeds such rows - and one all-zero label row"""
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint((T + 1) // 2, T + 1, (LOC_B,), generator=g)
    lens[0], lens[1] = T, 1
    mask = (torch.arange(T).unsqueeze(0) < lens.unsqueeze(1)).to(torch.int32)
    s, e = torch.randn(LOC_B, T, generator=g) * 3.0, torch.randn(LOC_B, T, generator=g) * 3.0
    y1, y2 = torch.rand(LOC_B, T, generator=g) * mask, torch.rand(LOC_B, T, generator=g) * mask
    scale = torch.tensor([0.2, 1.0, 3.0, 0.0, 1.7]).unsqueeze(1)
    y1, y2 = y1 / y1.sum(1, keepdim=True) * scale, y2 / y2.sum(1, keepdim=True) * torch.flip(scale, [0]) * (scale > 0)
    return s, e, mask, y1, y2


def loc_oracle(s, e, mask, y1, y2, dt):
    """per-clip terms of R.localizing_loss (their sum is its value) and its gradient wrt the logits, in dt; the per-clip sums of the
    absolute values of the reduced terms"""
    sr, er = s.detach().clone().to(dt).requires_grad_(True), e.detach().clone().to(dt).requires_grad_(True)
    ls = -(y1.to(dt) * torch.log_softmax(R.mask_logits(sr, mask), dim=-1))
    le = -(y2.to(dt) * torch.log_softmax(R.mask_logits(er, mask), dim=-1))
    part = (ls.sum(-1) + le.sum(-1)) / s.shape[0]
    loss = R.localizing_loss(sr, er, y1.to(dt), y2.to(dt), mask)
    assert abs(float(loss.detach()) - float(part.detach().sum())) <= 1e-5 * max(abs(float(loss.detach())), 1.0)
    loss.backward()
    return dict(loc_part=part.detach(), ds=sr.grad, de=er.grad), (ls.abs().sum(-1) + le.abs().sum(-1)).detach() / s.shape[0]


def run_loc(T, seed=31):
    from hual_amd import lib
    l = lib.load()
    s, e, mask, y1, y2 = loc_case(T, seed)
    dev = torch.device('cuda:0')
    sd, ed, md, y1d, y2d = s.to(dev), e.to(dev), mask.float().to(dev), y1.to(dev), y2.to(dev)
    ds, de, part = torch.empty_like(sd), torch.empty_like(sd), torch.empty(LOC_B, device=dev)
    si, ei = torch.empty(LOC_B, dtype=torch.int64, device=dev), torch.empty(LOC_B, dtype=torch.int64, device=dev)
    got = _prof(lib, l, lambda: lib.check(l.hual_localizing_loss(lib.ptr(sd), lib.ptr(ed), lib.ptr(md), lib.ptr(y1d), lib.ptr(y2d), lib.ptr(ds),
                                                                  lib.ptr(de), lib.ptr(part), lib.ptr(si), lib.ptr(ei), LOC_B, T, lib.stream_ptr())))
    assert got == {'heads_kernel<%d>' % (8 if T <= 128 else 16): 1}, got
    si_ref, ei_ref = R.ans_predictor(s, e, mask)
    assert torch.equal(si.cpu(), si_ref) and torch.equal(ei.cpu(), ei_ref)
    hip = dict(loc_part=part.cpu(), ds=ds.cpu(), de=de.cpu())
    o32, _ = loc_oracle(s, e, mask, y1, y2, torch.float32)
    o64, s_part = loc_oracle(s, e, mask, y1, y2, torch.float64)
    assert float(o64['loc_part'][3]) == 0.0 and float(o64['ds'][3].abs().max()) == 0.0      # the all-zero label row
    rows = []
    for k in ('loc_part', 'ds', 'de'):
        _close(k, hip[k], o32[k])
        d_hip, d_32 = (hip[k].double() - o64[k]).abs(), (o32[k].double() - o64[k]).abs()
        if k == 'loc_part':      # a reduced scalar per clip: each against its own sum of absolute terms
            r = max(_ratio(float(d_hip[i]), float(d_32[i]), float(s_part[i])) for i in range(LOC_B))
            rows.append((k, float(d_hip.max()), float(d_32.max()), float(s_part.max()), r))
        else:
            sc = float(o64[k].abs().max())
            rows.append((k, float(d_hip.max()), float(d_32.max()), sc, _ratio(float(d_hip.max()), float(d_32.max()), sc)))
    return rows


@pytest.mark.parametrize('T', LOC_T)
def test_localizing_loss(T):
    _gate('loc', 'B%d_T%d' % (LOC_B, T), run_loc(T))
