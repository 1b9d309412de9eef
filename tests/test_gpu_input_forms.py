"""GPU: every form of the input stage (csrc/seqpan.hip fwd_input / bwd_input with csrc/embed.hip, embed_gather.h, the feature paths of
csrc/gemm.hip / mproj.hip and the split layer norm of csrc/rowops.hip) against the oracle, through hual_video_proj_ln_fwd and its
backward hual_input_bwd, each case proving in the same test which kernels it ran (hual_prof_get), so a change of the dispatch cannot
take a shape off a form without a failing test.  The dispatch is restated below; tests/test_input_dispatch.py (no GPU) holds the case
table to every class of form named here and the restated constants to the sources.

What chooses a form (the configuration, never the data).  Feature load: `ksplit` - vdim a multiple of 256, at most 1024 - takes
feature_ksplit_kernel (weight quarters of vdim / 4 = 64 .. 256 rows) + ln_fwd_kernel, any other vdim one mproj_pair_kernel<NT, 63> with
the layer norm in its row phase, NT from mproj_rows(B T, B L) (16 rows per workgroup until the pair needs more than 256 workgroups).
bfloat16 clip features: `a_bf16` = 2 in the K-split kernel (no residual plane) when the dropout scale has at most four significant
bits (rate 0, 0.2, 0.5), else 1 - not visible in a symbol: the lossy direction (2 at a rate that needs 1) is an error of 2^-12 of the
features, three decades above gate (b); the other direction computes the same bits.  Char CNN: CP = 16 ceil(char_dim / 16),
ceil(4 CP / 128) weight steps forward (one step record, repeated) and as many column blocks in the window-gradient product
(mproj_kernel<NT, 0> for one, <NT, 32> for more); the max-pool rides in the product (mproj_kernel<NT, 128>) when C is a power of two
<= 16 and mproj_rows(Nq C), rounded up to a multiple of C, stays <= 64, else the tile is stored and char_pool_kernel pools it.
query_conv1d: catw = word_dim + 100 = 400, four K-blocks with a 16-wide last one forward, in the weight-gradient job and as four
column blocks of d cat (mproj_kernel<NT, 32>).  Per-block call: the position table's gradient is a launch of its own (pos_bwd_kernel
beside ln_bwd_kernel; the whole model runs ln_pos_bwd_kernel), the weight-gradient jobs (video_conv1d with the dropout / bfloat16
prologue, query_conv1d, the packed char filters) are one dw_f16_balanced_kernel behind one dw_table_write_kernel, and the last embed
step (window gradients folded into the char table in LDS) and the unpack of the filter gradients ride in colsum_kernel: no
embed_finish_kernel, no embed_unpack_kernel.  The per-block path skips nothing the whole model does: the forward call runs the
prologue (pack_weights_kernel with the gather), the backward call zeroes the bucket itself (zero_kernel).

Two gates per case.  (a) The 1e-3 contract: _close on x0, _check_param_grads on every parameter gradient the oracle's own backward
reached (exactly the stage's tensors, asserted by name; with finetune_word_emb the word table too), nothing else non-zero; the kernel's
char max-pool selections audited against the oracle's pre-pool values (audit_char_pins).  (b) The float32 noise floor, as in
test_gpu_cb_forms.py: the oracle - R.word_embs, R.char_embs, R.conv1d, R.layer_norm, R.add_pos_embs and the video dropout at SITE_VIDEO
in the order of R.forward, its float32 x0 asserted bit-equal to R.forward's cb.x0 tap - runs in float64 and in float32 with the same
dropout masks and the kernel's selections;  d_hip = max|hip - f64|  <=  M max(d_32, 2^-23 s),  d_32 = max|f32 - f64|,  s = max|f64| of
x0 or, for the gradients, the stage's largest gradient.  bfloat16 cases feed the kernel the bfloat16 tensor, the oracle its values.

M per class: twice the worst ratio measured on an MI355X over every case and tensor of the class at three data seeds
(profiles/input_forms_parity.txt, scripts/input_forms_parity.py), rounded up to a power of two, never above 16 - a condition.
Worst ratio per class (run, seed, tensor, d_hip against d_32) -> M:
  ksplit  1.64 (vdim 1024, no dropout, seed 1, gradient of video_conv1d/bias, 1.8e-5 against 9.0e-6) -> 4
  generic 1.11 (vdim 320, dropout on, seed 2, the same gradient, 2.2e-5 against 1.9e-5) -> 4
  rows    3.14 (B70 T55 L5 vdim 64, dropout on, seed 2, the same gradient, 8.3e-4 against 2.6e-4) -> 8
  char    1.43 (char_dim 50, dropout on, seed 2, the same gradient, 2.8e-5 against 1.9e-5) -> 4
  pool    2.06 (C 4, dropout on, seed 1, the same gradient, 2.6e-5 against 9.7e-6) -> 8
  words   1.42 (fine-tuned table, dropout on, seed 0, gradient of query_conv1d/bias, 4.3e-5 against 2.8e-5) -> 4
  edges   2.08 (B1 T1 L1 C4, no dropout, seed 1, gradient of video_conv1d/kernel, 2.3e-6 against 8.4e-7) -> 8
No ratio exceeds 4, so none is a finding about the kernels, and no class comes near the cap.  The worst tensors are bias gradients -
column sums of d lin over up to 3 850 rows, where the summation order of the weight-gradient launch meets the oracle's; x0 stays
below 1.0 everywhere.  At the data the runs below use (seed 0) the worst ratios are 1.43, 1.09, 1.75, 1.21, 1.26, 1.42 and 1.45.  The
gradients share one scale s (the stage's largest gradient: 7 for the one-row case, 1e2 .. 2e3 otherwise), so for the
small tensors (char filters, unk) the floor 2^-23 s, not d_32, is the yardstick - as _check_param_grads scales them.  A run takes
under 0.3 s of test time (the 4 200-row cases are the slowest); the restated dispatch predicted every launch of all 35 runs at all
three seeds.
What the gates see (scratch builds, arithmetic only, nothing committed).  With the two residual passes (hi.lo, lo.hi) taken out of
dw_f16_segment<DWB_DROP, 4> only - the video_conv1d weight-gradient job, which takes that instantiation whatever the feed and the rate -
all 35 runs here fail, every one of them at gate (b) alone, on the gradient of video_conv1d/kernel (ratios 258 .. 2 797; gate (a)
passes throughout: the error is about 5e-5 of the stage's largest gradient), while test_gpu_blocks.test_video_proj_ln_fwd (forward only) and
both cases of test_gpu_model.test_bfloat16_video_feed_parity still pass.  With them taken out of the pool-epilogue instantiation
mproj_body<NT, 128> only, exactly the 7 runs that take the epilogue fail (C 4, 8, 16, the 4 160-window case, B1 T1 L1 C4, with and
without dropout) and the 28 stored-tile runs pass: 6 at gate (b) alone (x0 at ratios 154 .. 162, the gradient of
q_layer_norm/layer_norm_scale at 34 .. 130, char biases and query_conv1d/bias at 8 .. 45), the 4 160-window case already in gate (a)
at audit_char_pins (a selection 1.9e-4 max|z| below the oracle's maximum against PIN_Z_TOL = 1e-4); test_video_proj_ln_fwd, whose C 4
shape runs the same epilogue, and the whole-model bfloat16 test still pass.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import parity_util as pu
from finetune_ref import WORD_TABLE
from oracle import philox as px
from oracle import seqpan_ref as R
from test_gpu_blocks import DROP, OFFSET, SEED, Block, _check_param_grads, _close
from test_gpu_cb_forms import CAP, _assert_form, _floor_rows
from test_gpu_da_bwd_fused import _prof
from test_gpu_da_forms import _cdiv

pytestmark = pytest.mark.gpu

M = {'ksplit': 4.0, 'generic': 4.0, 'rows': 8.0, 'char': 4.0, 'pool': 8.0, 'words': 4.0, 'edges': 8.0}

# the tensors of the stage, by their names in the flat layout
STAGE = ['word_embs/unk', 'char_embs/char_table'] + ['char_embs/%s_%d' % (n, i) for i in range(4) for n in ('filter', 'bias')] + \
        ['%s/%s' % (n, t) for n in ('query_conv1d', 'video_conv1d') for t in ('kernel', 'bias')] + \
        ['%s/layer_norm_%s' % (n, t) for n in ('q_layer_norm', 'v_layer_norm') for t in ('scale', 'bias')] + ['pos_emb/position_embeddings']


# ---------------------------------------------------------------------------------------------------- the dispatch, restated
MP_ROWS, MP_MAX = 64, 8          # csrc/mproj.hip, csrc/mproj.h
NALL, NCH = 128, 100             # csrc/embed_gather.h: padded / real channels of the char CNN's filter bank
DW_JOBS = 12                     # csrc/gemm.h HUAL_MAX_DW_JOBS: jobs per dw_table_write_kernel


def ksplit(vdim, word_dim=300):
    """csrc/seqpan.hip setup_ctx c.ksplit: the feature load on the K-split kernel"""
    catw = word_dim + 100
    qks = ((catw + 3) // 4 + 63) & ~63
    return vdim % 256 == 0 and vdim <= 1024 and catw % 8 == 0 and qks <= 256


def a_bf16(bf16, rate):
    """csrc/gemm.hip launch_feature_ksplit: 0 float32 features; 2 bfloat16 without the residual plane (the dropout scale has at most
    four significant bits); 1 bfloat16 with the full split"""
    if not bf16:
        return 0
    m16 = math.frexp(float(px.keep_scale(rate)) if rate > 0 else 1.0)[0] * 16.0
    return 2 if m16 == math.floor(m16) else 1


def mproj_pair_grid(R0, R1, t):
    """csrc/mproj.hip: workgroups of a pair launch, 8 x the largest per-XCD count of the two problems' tiles"""
    nb0, nb1 = _cdiv(R0, t), _cdiv(R1, t)
    return 8 * max((nb0 * (x + 1) // 8 - nb0 * x // 8) + (nb1 * (x + 1) // 8 - nb1 * x // 8) for x in range(8))


def mproj_rows(R0, R1=0):
    """csrc/mproj.hip mproj_rows: rows per workgroup of one problem / of a pair launched together"""
    t = 16
    while t < MP_ROWS and (mproj_pair_grid(R0, R1, t) if R1 > 0 else _cdiv(R0, t)) > 256:
        t += 1
    return t


def mproj_nt(mt):
    """the NT of mproj_kernel<NT, F>: 16-row tiles of a workgroup, at least two"""
    return min(max(_cdiv(mt, 16), 2), 4)


def cpad(char_dim):
    return 16 * _cdiv(char_dim, 16)


def char_steps(char_dim):
    """weight steps of the char CNN forward = column blocks of the window-gradient product"""
    return _cdiv(4 * cpad(char_dim), 128)


def pool_epilogue(Nq, C):
    """csrc/embed.hip launch_embed_fwd: (the max-pool rides in the product, rows per workgroup of the forward product)"""
    mt = mproj_rows(Nq * C)
    mtp = _cdiv(mt, C) * C
    ep = (C & (C - 1)) == 0 and C <= 16 and mtp <= 64
    return ep, mtp if ep else mt


def input_form(sp):
    """everything that chooses a code path of the stage"""
    B, T, L, C = sp['B'], sp['T'], sp['L'], sp['C']
    Nv, Nq, catw = B * T, B * L, 300 + 100
    ep, mt_c = pool_epilogue(Nq, C)
    return dict(ksplit=ksplit(sp['vdim']), quarter=sp['vdim'] // 4, a_bf16=a_bf16(sp.get('bf16', False), sp['rate']), R=Nv + Nq,
                mt_pair=mproj_rows(Nv, Nq), part_k=sp['vdim'] % 128, char_steps=char_steps(sp['char_dim']), pool=ep, mt_char=mt_c,
                mt_win=mproj_rows(Nq * C), char_ragged=(Nq * C) % mt_c != 0, mt_q=mproj_rows(Nq), q_steps=_cdiv(catw, 128), q_last=catw % 128,
                finetune=sp.get('words') == 'finetune')


def input_dispatch(sp):
    """{kernel symbol: launches} of hual_video_proj_ln_fwd + hual_input_bwd: every launch of the two calls"""
    f = input_form(sp)
    want = {}

    def add(k):
        want[k] = want.get(k, 0) + 1
    add('pack_weights_kernel')                                                  # prologue: masks, weight images, the gather
    if f['pool']:
        add('mproj_kernel<%d, 128>' % mproj_nt(f['mt_char']))                  # char CNN with the pool epilogue
    else:
        add('mproj_kernel<%d, 0>' % mproj_nt(f['mt_char']))
        add('char_pool_kernel')
    if f['ksplit']:
        add('feature_ksplit_kernel')
        add('ln_fwd_kernel')
    else:
        add('mproj_pair_kernel<%d, 63>' % mproj_nt(f['mt_pair']))
    add('zero_kernel')
    add('pos_bwd_kernel')
    add('ln_bwd_kernel')
    assert f['q_steps'] > 1
    add('mproj_kernel<%d, 32>' % mproj_nt(f['mt_q']))                            # d cat: four column blocks of one operand
    add('char_pool_bwd_kernel')
    add('mproj_kernel<%d, %d>' % (mproj_nt(f['mt_win']), 32 if f['char_steps'] > 1 else 0))      # d windows
    assert 3 <= DW_JOBS
    add('dw_table_write_kernel')
    add('dw_f16_balanced_kernel')
    add('colsum_kernel')
    return want


# (class of the noise-floor gate, what it is there for, [case]).  A case: B, T, L, C, vdim, char_dim and - optional - bf16, rate (the
# dropout rate of its run, DROP unless given), words (a batch with unk, pad and char-less words: 'frozen' | 'finetune'), max_vlen.
# Every class runs at dropout 0.2, its first case without dropout as well
def _c(B=3, T=20, L=6, C=5, vdim=64, char_dim=50, **kw):
    return dict(dict(B=B, T=T, L=L, C=C, vdim=vdim, char_dim=char_dim, rate=DROP), **kw)


IN_TABLE = [
    ('ksplit', 'the K-split feature load at every quarter size; bfloat16 with and without the residual plane',
     [_c(vdim=256), _c(vdim=256, bf16=True), _c(vdim=256, bf16=True, rate=0.1), _c(vdim=512), _c(vdim=768),
      _c(vdim=1024), _c(vdim=1024, rate=0.0), _c(vdim=1024, bf16=True), _c(vdim=1024, bf16=True, rate=0.1)]),
    ('generic', 'mproj_pair with the layer norm in the row phase; vdim 320 ends on a partial weight block',
     [_c(vdim=320), _c(vdim=64), _c(vdim=320, bf16=True)]),
    ('rows', 'more than 256 x 16 rows: workgroups above 16 rows, ragged last tile; K-split and pair launch',
     [_c(B=70, T=55, L=5, vdim=256), _c(B=70, T=55, L=5, vdim=64)]),
    ('char', '1, 2 and 4 weight steps of the char CNN, stored-tile pool', [_c(char_dim=20), _c(char_dim=50), _c(char_dim=100)]),
    ('pool', 'pool epilogue (C 4, 8, 16) against the stored tile (C 5, 12, 32); above 4096 window rows',
     [_c(T=8, C=4), _c(T=8, C=5), _c(T=8, C=8), _c(T=8, C=12), _c(T=8, C=16), _c(T=8, C=32), _c(B=52, T=8, L=10, C=8)]),
    ('words', 'unk, pad and char-less words, short queries; frozen and fine-tuned table',
     [_c(B=4, L=9, C=6, words='frozen'), _c(B=4, L=9, C=6, words='finetune')]),
    ('edges', 'one row of each kind; the last row of the position table', [_c(B=1, T=1, L=1, C=4), _c(B=2, T=12, L=12, max_vlen=12)]),
]
IN_CASES = [(cls, dict(sp, seed=1500 + 10 * i + k)) for i, (cls, _, cases) in enumerate(IN_TABLE) for k, sp in enumerate(cases)]
IN_RUNS = [(cls, sp) for cls, sp in IN_CASES] + \
          [(cls, dict(sp, rate=0.0)) for i, (cls, _, cases) in enumerate(IN_TABLE) for sp in [dict(cases[0], seed=1500 + 10 * i)]]


def _id(v):
    if not isinstance(v, dict):
        return str(v)
    return 'B%d_T%d_L%d_C%d_v%d_c%d%s%s_drop%g' % (v['B'], v['T'], v['L'], v['C'], v['vdim'], v['char_dim'], '_bf16' if v.get('bf16') else '',
                                                 '_' + v['words'] if v.get('words') else '', v['rate'])


# ---------------------------------------------------------------------------------------------------- one case
MIN_T, MIN_L = 8, 3


def make_case(sp):
    """pu.make_case for the case (R.synthetic_batch needs clips that hold a labelled span and draws queries of at least three words:
    a shorter T or L takes the first frames / word columns of such a batch).  words: a small vocabulary with repeated words, unk words
    (id 1) in and at the end of queries, a query of one word, and words none of whose chars is a real one"""
    B, T, L, C = sp['B'], sp['T'], sp['L'], sp['C']
    cfg, p, wv, b, labels = pu.make_case(B=B, T=max(T, MIN_T), L=max(L, MIN_L), C=C, seed=sp['seed'], max_vlen=sp.get('max_vlen', max(T, L, 8)),
                                         vdim=sp['vdim'], char_dim=sp['char_dim'])
    b = dict(b, video=b['video'][:, :T].contiguous(), lens=b['lens'].clamp(max=T), word_ids=b['word_ids'][:, :L].contiguous(),
             char_ids=b['char_ids'][:, :L].contiguous())
    assert int(b['lens'].max()) == T
    if sp.get('words'):
        g = np.random.default_rng(sp['seed'])
        w, ch = b['word_ids'].clone(), b['char_ids'].clone()
        for k in range(B):
            n = int((w[k] > 0).sum())
            w[k, :n] = torch.tensor(g.integers(1, 12, size=n), dtype=w.dtype)
        w[0, :3] = torch.tensor([7, 7, 1])
        w[1, 1:], ch[1, 1:] = 0, 0                      # a query of one word
        w[2, int((w[2] > 0).sum()) - 1] = 1             # unk as the last word
        ch[0, 1], ch[3, 1] = 0, 0                       # table words without a char
        assert int((w == 1).sum()) >= 2 and int((w == 0).sum()) >= L - 1 and int(((ch == 0).all(-1) & (w > 1)).sum()) >= 2
        b = dict(b, word_ids=w, char_ids=ch)
    if sp.get('bf16'):
        b = dict(b, video=b['video'].to(torch.bfloat16).to(torch.float32))       # the oracle's feed: the same values
    return cfg, p, wv, b, labels


def _finetune_model(cfg, p, wv):
    """pu.hip_model with hual_cfg.finetune_word_emb: the table is the last entry of the flat layout and starts as wv"""
    from hual_amd import lib
    from hual_amd.model import SeqPAN
    hc = lib.make_cfg(vdim=cfg.vdim, dim=cfg.dim, num_heads=cfg.num_heads, word_dim=cfg.word_dim, char_dim=cfg.char_dim,
                      max_vlen=cfg.max_vlen, attn_layer=cfg.attn_layer, num_chars=cfg.num_chars, num_words=cfg.num_words,
                      match_lambda=cfg.match_lambda, clip_norm=cfg.clip_norm, no_gumbel=1 if cfg.get('no_gumbel', True) else 0,
                      tau=float(cfg.get('tau', 0.3)), finetune_word_emb=1)
    m = SeqPAN(hc, wv.numpy())
    m.ws_poison = 0xFF
    m.load_state_dict({k: v.detach().numpy() for k, v in p.items()})
    return m


class InBlock(Block):
    """Block for one case: the bfloat16 feed and the fine-tuning model where the case asks for them"""

    def __init__(self, sp):
        super().__init__(drop=sp['rate'], case=make_case(sp))
        self.sp = sp
        self.finetune = sp.get('words') == 'finetune'
        if self.finetune:
            self.m = _finetune_model(self.cfg, self.p, self.wv)
            self.m.set_rng(SEED, OFFSET)
            self.ws = self.m._workspace(self.B, self.T, self.L, self.C)
            self.opts = self.m._opts(self.drop)
            self.grads = torch.full_like(self.m.params, 3.0)
        b = self.b
        feed = b['video'].to(torch.bfloat16) if sp.get('bf16') else b['video'].numpy()
        self.bt, self.keep, _ = self.m._prep(feed, b['lens'].numpy(), b['word_ids'].numpy(), b['char_ids'].numpy())
        assert (self.B, self.T, self.L, self.C) == (sp['B'], sp['T'], sp['L'], sp['C'])

    def in_args(self):
        lib = self.lib
        return [ctypes.byref(self.m.cfg), lib.ptr(self.m.params), lib.ptr(self.m.word_table), ctypes.byref(self.bt), ctypes.byref(self.opts)]

    def char_arg(self):
        """the window every (word, channel) unit of the char CNN took its maximum from (-1: the relu floor), int32 [B, L, 100]"""
        off, rows, cols = self.m._ws_table['char_arg']
        assert (rows, cols) == (self.Nq, NCH)
        return self.m._ws[off:off + rows * cols * 4].view(torch.int32).cpu().reshape(self.B, self.L, cols).clone()


def make_block(sp):
    return InBlock(sp)


def compose(pr, wv, b, rng, pin=None, tap=None):
    """the stage in the order of R.forward (model.py:36-56) on the parameters pr (their dtype): x0 [B (T + L), 128]"""
    dt = pr['video_conv1d/kernel'].dtype
    B, T = b['video'].shape[:2]
    L = b['word_ids'].shape[1]
    rows_v, rows_q0 = np.arange(B * T), np.arange(B * L)
    we = R.word_embs(b['word_ids'], pr, wv.to(dt), rng, rows_q0)
    ce = R.char_embs(b['char_ids'], pr, rng, rows_q0, pin, tap)
    cat = torch.cat([we, ce], dim=-1)
    q = R.layer_norm(R.conv1d(cat, pr, 'query_conv1d'), pr, 'q_layer_norm')
    v = R._dropout(b['video'].to(dt), rng, px.SITE_VIDEO, rows_v)
    v = R.layer_norm(R.conv1d(v, pr, 'video_conv1d'), pr, 'v_layer_norm')
    pos = pr['pos_emb/position_embeddings']
    v, q = R.add_pos_embs(v, pos), R.add_pos_embs(q, pos)
    return torch.cat([v.reshape(B * T, -1), q.reshape(B * L, -1)])


def oracle_rng(drop):
    """the rng R.forward builds for the rate (none without dropout)"""
    return px.DropoutRNG(SEED, OFFSET, drop) if drop else None


def _params(blk, dt):
    pr = {k: t.detach().clone().to(dt).requires_grad_(True) for k, t in blk.p.items()}
    wv = blk.wv.detach().clone().to(dt)
    if blk.finetune:
        pr[WORD_TABLE] = wv.requires_grad_(True)
    return pr, wv


def run_input(blk, xseed=9, prove=False):
    """hual_video_proj_ln_fwd + hual_input_bwd on a random d_x0; the launched kernels and gate (a) asserted; returns the rows of gate
    (b).  prove: the composed oracle's float32 x0 is R.forward's cb.x0 tap, bit for bit"""
    lib, l = blk.lib, blk.l
    dx0 = blk.rand(blk.R, xseed)
    dxd = dx0.to(blk.dev)
    x0 = torch.empty_like(dxd)

    def call():
        lib.check(l.hual_video_proj_ln_fwd(*blk.in_args(), lib.ptr(x0), *blk.tail()))
        lib.check(l.hual_input_bwd(*blk.in_args(), lib.ptr(dxd), lib.ptr(blk.grads), *blk.tail()))
    _assert_form(_prof(lib, l, call), '', input_dispatch(blk.sp))
    pin, rng = blk.char_arg(), oracle_rng(blk.drop)

    def oracle(dt):
        pr, wv = _params(blk, dt)
        tap = {}
        ref = compose(pr, wv, blk.b, rng, pin, tap)
        ref.backward(dx0.to(dt))
        return pr, dict(x0=ref.detach()), tap
    pr, o32, tap = oracle(torch.float32)
    pu.audit_char_pins(tap, {'char.arg': pin})
    if prove:
        b = blk.b
        out = R.forward(blk.p, blk.cfg, blk.wv, b['video'], b['lens'], b['word_ids'], b['char_ids'], drop_rate=blk.drop, seed=SEED, offset=OFFSET,
                        want_tap=True, relu_pin={'char.arg': pin})
        assert torch.equal(o32['x0'], torch.cat([out['tap']['cb.x0.v'].reshape(blk.Nv, 128), out['tap']['cb.x0.q'].reshape(blk.Nq, 128)]))
    _close('x0', x0.cpu(), o32['x0'])
    # the filter of the parameter gradients: the oracle's own list of the tensors its backward reached - the stage's, by name
    reached = sorted(k for k, t in pr.items() if t.grad is not None)
    assert reached == sorted(STAGE + ([WORD_TABLE] if blk.finetune else [])), reached
    _check_param_grads(blk, pr, lambda k: k in reached)
    return _floor_rows(blk, tuple(reached), dict(x0=x0.cpu()), oracle(torch.float64)[:2], (pr, o32))


def _gate(cls, blk, rows):
    """gate (b): every tensor's ratio printed, then held to the class's M"""
    for r in rows:
        print('%-8s %s  %-40s d_hip %.3e  d_32 %.3e  s %.3e  ratio %6.2f' % ((cls, _id(blk.sp)) + r))
    assert M[cls] <= CAP
    bad = [r for r in rows if not r[4] <= M[cls]]
    assert not bad, (cls, 'M = %g' % M[cls], bad)


# ---------------------------------------------------------------------------------------------------- stage parity per form
@pytest.mark.parametrize('cls,sp', IN_RUNS, ids=_id)
def test_input_fwd_bwd_by_form(cls, sp):
    blk = make_block(sp)
    _gate(cls, blk, run_input(blk, prove=(cls, sp['vdim'], sp['rate'], sp.get('bf16')) == ('ksplit', 256, DROP, None)))


def test_fine_tuned_table_rows():
    """the fine-tuned case's table gradient by rows: a row of a word that is absent from the batch is exactly zero, every present word's
    row is not, and pad / unk ids reach no row of the table"""
    (sp,) = [sp for cls, sp in IN_CASES if sp.get('words') == 'finetune']
    blk = make_block(sp)
    run_input(blk)
    gt = torch.from_numpy(blk.params_grad()[WORD_TABLE])
    present = sorted(set(int(i) - 2 for i in blk.b['word_ids'].reshape(-1) if int(i) >= 2))
    absent = [r for r in range(blk.cfg.num_words - 2) if r not in present]
    assert present and absent and float(gt[absent].abs().max()) == 0.0 and float(gt[present].abs().max(1).values.min()) > 0.0
