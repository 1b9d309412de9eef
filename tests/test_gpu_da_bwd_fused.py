"""GPU: the fused backward launch of the dual attention block (csrc/dablock.hip ln2_mid_bwd_kernel<NT>): dense_2^T + layer_norm_2
backward and the gated middle behind it as one launch in the whole model - parity with the oracle at one, two and three row tiles
per workgroup with a ragged last tile, which kernels a whole step and a per-block call launch, and one / three attention layers
(the last layer takes dropout'(dx) from the keep bits, the layers below read the dz2 the layer above left)."""
import ctypes

import numpy as np
import pytest
import torch

import parity_util as pu
from oracle import seqpan_ref as R
from test_gpu_blocks import Block
from test_gpu_shapes import _check, _check_all

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------- row tiles (csrc/common.h)
def _tiles(rows, mt):
    return (rows + mt - 1) // mt


def _grid(R, Nv, mt):
    """xcd_clip_grid: workgroups of a launch over R rows (the first Nv: video rows) at mt rows per workgroup"""
    nq = R - Nv
    return 8 * max((_tiles(Nv * (x + 1) // 8, mt) - _tiles(Nv * x // 8, mt)) +
                   (_tiles(Nv + nq * (x + 1) // 8, mt) - _tiles(Nv + nq * x // 8, mt)) for x in range(8))


def _rows_per_workgroup(R, Nv):
    """xcd_clip_rows(R, Nv, 16, 48) = ln_proj_bwd_rows = da_post_rows"""
    mt = max((R + 255) // 256, 16)
    while mt < 48 and _grid(R, Nv, mt) > 256:
        mt += 1
    return min(mt, 48)


# one / two / three 16-row tiles per workgroup; the last workgroup's rows end inside its tile (R % MT != 0) and, where a workgroup
# may hold other than 16 rows at all (MT >= 16 always: one tile means MT = 16), its last tile is partly used (MT % 16 != 0)
FUSED_SHAPES = [(1, dict(B=5, T=50, L=11, C=5, seed=21, max_vlen=64)),
                (2, dict(B=44, T=128, L=20, C=8, seed=22, max_vlen=128, vdim=512)),
                (3, dict(B=60, T=128, L=20, C=8, seed=23, max_vlen=128, vdim=512))]


@pytest.mark.parametrize('nt,shape', FUSED_SHAPES)
def test_whole_model_at_one_two_three_row_tiles(nt, shape):
    """forward + backward of the whole model (the fused launch) against the oracle: every tap, output, loss term and gradient
    within 1e-3 (test_gpu_shapes._check_all), span indices equal"""
    R_, Nv = shape['B'] * (shape['T'] + shape['L']), shape['B'] * shape['T']
    mt = _rows_per_workgroup(R_, Nv)
    assert (mt + 15) // 16 == nt and R_ % mt != 0 and (nt == 1 or mt % 16 != 0), (R_, mt)
    _check_all(pu.make_case(**shape), 0.2)


# ---------------------------------------------------------------------------------------------------- which kernels run
def _prof(lib, l, fn):
    lib.check(l.hual_prof_begin())
    fn()
    torch.cuda.synchronize()
    n = l.hual_prof_end()
    got = {}
    for i in range(n):
        name = ctypes.create_string_buffer(256)
        cnt = ctypes.c_int64()
        lib.check(l.hual_prof_get(i, name, 256, ctypes.byref(cnt), None, None, None))
        got[name.value.decode()] = int(cnt.value)
    return got


def test_whole_step_launches_the_fused_kernel():
    """one forward + backward at the bench shape (two layers, 38 rows per workgroup): one fused launch per layer, no da_mid_bwd_kernel
    and no one-product ln_proj_bwd_kernel of its own; the six-product launches behind the attentions are as they were"""
    from hual_amd import lib
    cfg, p, wv, b, labels = pu.make_case(B=64, T=128, L=20, C=8, seed=12345, max_vlen=128, vdim=1024)
    m = pu.hip_model(cfg, p, wv)
    m.set_rng(5, 7)

    def step():
        m.forward(b['video'].numpy(), b['lens'].numpy(), b['word_ids'].numpy(), b['char_ids'].numpy(), drop_rate=0.2,
                  labels=tuple(x.numpy() for x in labels))
        m.backward()
    got = _prof(lib, lib.load(), step)
    assert got.get('ln2_mid_bwd_kernel<3>') == cfg.attn_layer == 2, got
    assert not [k for k in got if k.startswith('da_mid_bwd_kernel')], got
    assert 'ln_proj_bwd_kernel<false, 3>' not in got, got
    assert got.get('ln_proj_bwd_kernel<false, 3, true>') == 2, got


@pytest.mark.parametrize('layer', [0, 1])
def test_per_block_call_launches_the_unfused_pair(layer):
    blk = Block(B=4, T=64, L=20, C=6, seed=9, max_vlen=64)
    lib = blk.lib
    xd, dyd = blk.rand(blk.R, 3).to(blk.dev), blk.rand(blk.R, 4).to(blk.dev)
    y, dx = torch.empty_like(xd), torch.empty_like(xd)

    def call():
        lib.check(blk.l.hual_dual_attn_fwd(*blk.args(), layer, lib.ptr(xd), lib.ptr(y), *blk.tail()))
        lib.check(blk.l.hual_dual_attn_bwd(*blk.args(), layer, lib.ptr(dyd), lib.ptr(dx), lib.ptr(blk.grads), *blk.tail()))
    got = _prof(lib, blk.l, call)
    assert got.get('da_mid_bwd_kernel<1>') == 1 and got.get('ln_proj_bwd_kernel<false, 1>') == 1, got
    assert not [k for k in got if k.startswith('ln2_mid_bwd')], got


def test_kernel_pipe_of_the_fused_kernel():
    from hual_amd import lib
    l = lib.load()
    ref, rp = ctypes.c_int32(), ctypes.c_int32()
    lib.check(l.hual_prof_kernel_pipe(b'da_mid_bwd_kernel<3>', ctypes.byref(ref), ctypes.byref(rp)))
    pipe, passes = ctypes.c_int32(), ctypes.c_int32()
    lib.check(l.hual_prof_kernel_pipe(b'ln2_mid_bwd_kernel<3>', ctypes.byref(pipe), ctypes.byref(passes)))
    assert (pipe.value, passes.value) == (ref.value, rp.value) and passes.value == 3


# ---------------------------------------------------------------------------------------------------- layer boundaries
def _case_with_layers(n_layers, B, T, L, C, seed, max_vlen):
    """parity_util.make_case with model.attn_layer = n_layers"""
    cfg = R.default_cfg(max_vlen=max_vlen, num_words=60, attn_layer=n_layers)
    p = R.init_params(cfg, seed=1)
    g = np.random.default_rng(101)
    for k in p:
        if k.endswith('bias') or 'bias_' in k or k.endswith('layer_norm_scale'):
            p[k] = p[k] + torch.tensor(g.normal(0, 0.05, size=tuple(p[k].shape)), dtype=torch.float32)
    p['label_emb'] = p['label_emb'] + torch.tensor(g.normal(0, 0.1, size=tuple(p['label_emb'].shape)), dtype=torch.float32)
    wv = R.init_word_vectors(cfg)
    b = R.synthetic_batch(cfg, B, T, L, C, seed=seed)
    lens = b['lens'].numpy()
    for k in range(0, B, 2):
        b['s_ind'][k] = 1
        b['e_ind'][k] = int(lens[k]) - 2
    from hual_amd import data
    y1, y2, mm, ii = data.make_labels(b['s_ind'], b['e_ind'], lens, max_len=T)
    return cfg, p, wv, b, (torch.tensor(y1), torch.tensor(y2), torch.tensor(mm), torch.tensor(ii, dtype=torch.float32))


@pytest.mark.parametrize('n_layers,drop', [(1, 0.0), (1, 0.2), (3, 0.0)])
def test_one_and_three_attention_layers(n_layers, drop):
    """attn_layer = 1: only the last layer's form of the fused launch (the operand of its product is dropout'(dx) from the forward's keep
    bits, saved as dz2) and no layer below; attn_layer = 3: two layers that read the dz2 the six-product launch above them left.
    Three layers run without dropout: the dropout site ids of a dual attention layer are SITE_DA + 8 li + {0..4} = 8 + 8 li, and those
    of li = 2 are the ids of the trilinear sites (SITE_TRI = 24, oracle/philox.py, include/hual_seqpan.h) - the oracle and the
    library draw different streams there already in the forward pass, whatever the backward launches do"""
    case = _case_with_layers(n_layers, B=6, T=41, L=9, C=5, seed=31, max_vlen=48)
    assert case[0].attn_layer == n_layers
    rows, idx_equal, o, h, m = pu.compare(*case, drop_rate=drop)
    _check(rows, idx_equal)
    assert len([r for r in rows if r[0] == 'grad' and r[1].startswith('d_attn_')]) > 0
