"""GPU: the 64-short-row form of the wide context-query kernels (csrc/cqwide.hip cq_fwd_wide_kernel<8, 64> / cq_bwd_wide_kernel<8, 64>):
queries of 33-64 words against clips of at most 128 frames - which kernels serve which padded shape, parity with the oracle at the
tile edges of the short side, the whole model, the same gate through the path it replaces, graph replay and guard bands."""
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
from test_gpu_blocks import Block, _check_param_grads, _close
from test_gpu_guard_bands import GUARD, Arena
from test_gpu_shapes import _check_all

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

OLD = ('cq_fwd_kernel', 'cq_bwd_kernel', 'cq_fwd_staged_kernel', 'cq_bwd_staged_kernel', 'tri_prep_kernel')


def _run_block(blk, drop_on=True):
    """hual_cq_attn_fwd + hual_cq_attn_bwd on random activations; returns (x, dy, feats, dx) on the host"""
    lib = blk.lib
    if not drop_on:
        blk.opts = blk.m._opts(0.0)
    x, dy = blk.rand(blk.R, 5), blk.rand(blk.R, 6)
    xd, dyd = x.to(blk.dev), dy.to(blk.dev)
    feats, dx = torch.empty_like(xd), torch.empty_like(xd)
    lib.check(blk.l.hual_cq_attn_fwd(*blk.args(), lib.ptr(xd), lib.ptr(feats), *blk.tail()))
    lib.check(blk.l.hual_cq_attn_bwd(*blk.args(), lib.ptr(dyd), lib.ptr(dx), lib.ptr(blk.grads), *blk.tail()))
    torch.cuda.synchronize()
    return x, dy, feats.cpu(), dx.cpu()


def _kernels(T, L, B=3):
    """names of the kernels one forward + backward of the block launches (hual_prof_get)"""
    blk = Block(B=B, T=T, L=L, C=4, seed=31, max_vlen=max(T, L, 32))
    l = blk.l
    blk.lib.check(l.hual_prof_begin())
    _run_block(blk)
    n = l.hual_prof_end()
    got = {}
    for i in range(n):
        name = ctypes.create_string_buffer(256)
        cnt = ctypes.c_int64()
        blk.lib.check(l.hual_prof_get(i, name, 256, ctypes.byref(cnt), None, None, None))
        got[name.value.decode()] = int(cnt.value)
    return got


# ---------------------------------------------------------------------------------------------------- 1. dispatch
@pytest.mark.parametrize('TL', [(100, 33), (100, 45), (100, 64), (64, 40), (128, 64), (64, 64), (33, 33), (48, 40)])
def test_long_queries_run_the_wide_kernels(TL):
    got = _kernels(*TL)
    assert got.get('cq_fwd_wide_kernel<8, 64>') == 1 and got.get('cq_bwd_wide_kernel<8, 64>') == 1, got      # one launch covers both directions
    assert not [k for k in got if k.startswith(OLD) or (('wide' in k) and '64>' not in k)], got


@pytest.mark.parametrize('TL', [(100, 65), (100, 79), (40, 50), (256, 40)])
def test_shapes_outside_the_range_keep_their_kernels(TL):
    got = _kernels(*TL, B=2)
    assert not [k for k in got if 'wide' in k], got
    assert [k for k in got if k.startswith(('cq_fwd_kernel', 'cq_fwd_staged_kernel'))], got
    assert [k for k in got if k.startswith(('cq_bwd_kernel', 'cq_bwd_staged_kernel'))], got


@pytest.mark.parametrize('TL,fwd,bwd', [((100, 32), 'cq_fwd_wide_kernel<8>', 'cq_bwd_wide_kernel<8>'),
                                        ((256, 20), 'cq_fwd_wide_kernel<16>', 'cq_bwd_wide_kernel<16>')])
def test_short_queries_run_the_symbols_they_ran_before(TL, fwd, bwd):
    got = _kernels(*TL, B=2)
    assert got.get(fwd) == 1 and got.get(bwd) == 1, got
    assert not [k for k in got if k.startswith(OLD) or ('wide' in k and k not in (fwd, bwd))], got


def test_kernel_pipe_of_the_new_symbols():
    from hual_amd import lib
    ref = ctypes.c_int32()
    lib.check(lib.load().hual_prof_kernel_pipe(b'cq_fwd_staged_kernel', ctypes.byref(ref), ctypes.byref(ctypes.c_int32())))
    for k in ('cq_fwd_wide_kernel<8, 64>', 'cq_bwd_wide_kernel<8, 64>'):
        pipe, passes = ctypes.c_int32(), ctypes.c_int32()
        lib.check(lib.load().hual_prof_kernel_pipe(k.encode(), ctypes.byref(pipe), ctypes.byref(passes)))
        assert pipe.value == ref.value and passes.value == 3      # the 16-bit matrix pipe, three passes


# ---------------------------------------------------------------------------------------------------- 2. block parity
def _oracle_gate(blk, x, dy, feats, dx, drop_on=True):
    """the gate of test_gpu_blocks.test_cq_attn_fwd_bwd; returns the largest differences (feats, dx) for messages"""
    rng = blk.rng if drop_on else px.DropoutRNG(5, 7, 0.0)
    pr = blk.oracle_params()
    xr = x.clone().requires_grad_(True)
    v, q = blk.split(xr)
    q2v = R.cq_attention(v, q, blk.v_mask, blk.q_mask, pr, 'q2v_attn', rng, px.SITE_TRI + 0, blk.rows_v, px.SITE_TRI + 1, blk.rows_q)
    v2q = R.cq_attention(q, v, blk.q_mask, blk.v_mask, pr, 'v2q_attn', rng, px.SITE_TRI + 2, blk.rows_q, px.SITE_TRI + 3, blk.rows_v)
    ref = torch.cat([q2v.reshape(blk.Nv, 128), v2q.reshape(blk.Nq, 128)])
    _close('feats', feats, ref.detach())
    ref.backward(dy)
    _close('dx', dx, xr.grad)
    _check_param_grads(blk, pr, lambda k: k.startswith('q2v_attn/') or k.startswith('v2q_attn/'))
    return float((feats - ref.detach()).abs().max()), float((dx - xr.grad).abs().max())


CQ64_SHAPES = [dict(B=3, T=100, L=L, C=4, seed=100 + L, max_vlen=100) for L in (33, 47, 48, 49, 63, 64)] + [
    dict(B=3, T=64, L=64, C=4, seed=201, max_vlen=64), dict(B=2, T=128, L=64, C=4, seed=202, max_vlen=128),
    dict(B=3, T=65, L=33, C=4, seed=203, max_vlen=96),                  # ragged second chunk round
    dict(B=9, T=100, L=45, C=4, seed=204, max_vlen=100), dict(B=1, T=100, L=50, C=4, seed=205, max_vlen=100),
    dict(B=2, T=33, L=33, C=4, seed=206, max_vlen=48)]                  # fewer M2 scratch rows than short-side rows


@pytest.mark.parametrize('drop', [0.2, 0.0])
@pytest.mark.parametrize('shape', CQ64_SHAPES, ids=lambda s: 'B%d_T%d_L%d' % (s['B'], s['T'], s['L']))
def test_cq_attn_fwd_bwd_long_queries(shape, drop):
    blk = Block(**shape)
    x, dy, feats, dx = _run_block(blk, drop_on=drop > 0)
    _oracle_gate(blk, x, dy, feats, dx, drop_on=drop > 0)


def _mask_case():
    """a one-word query and a 1-frame clip next to full ones (as test_gpu_shapes.test_tiny_clips_and_one_word_queries builds them)"""
    cfg, p, wv, b, labels = pu.make_case(B=4, T=100, L=40, C=5, seed=71, max_vlen=100)
    lens = np.array([100, 1, 2, 57], dtype=np.int32)
    b['lens'] = torch.tensor(lens)
    for k in range(4):
        b['video'][k, lens[k]:] = 0.0
    b['word_ids'][1, 1:] = 0
    b['char_ids'][1, 1:] = 0
    b['word_ids'][3, 35:] = 0
    b['char_ids'][3, 35:] = 0
    return cfg, p, wv, b, labels


@pytest.mark.parametrize('drop', [0.2, 0.0])
def test_cq_attn_long_queries_mask_paths(drop, monkeypatch):
    case = _mask_case()
    monkeypatch.setattr(pu, 'make_case', lambda **kw: case)
    blk = Block()
    assert (blk.T, blk.L) == (100, 40) and int(blk.q_mask[1].sum()) == 1 and int(blk.v_mask[1].sum()) == 1
    x, dy, feats, dx = _run_block(blk, drop_on=drop > 0)
    _oracle_gate(blk, x, dy, feats, dx, drop_on=drop > 0)


# ---------------------------------------------------------------------------------------------------- 3. whole model
@pytest.mark.parametrize('shape', [dict(B=6, T=100, L=45, C=13, seed=92, max_vlen=100), dict(B=4, T=100, L=64, C=22, seed=94, max_vlen=100)])
def test_whole_model_long_queries(shape):
    _check_all(pu.make_case(char_dim=100, **shape), 0.2)


# ---------------------------------------------------------------------------------------------------- 4. the path it replaces
_CHILD = '''
import sys, json, torch
import test_gpu_cq_long_queries as t
from test_gpu_blocks import Block
blk = Block(**json.loads(sys.argv[1]))
x, dy, feats, dx = t._run_block(blk)
t._oracle_gate(blk, x, dy, feats, dx)
torch.save(dict(feats=feats, dx=dx, grads=blk.grads.cpu()), sys.argv[2])
'''


@pytest.mark.parametrize('shape', [CQ64_SHAPES[1], CQ64_SHAPES[7]], ids=lambda s: 'B%d_T%d_L%d' % (s['B'], s['T'], s['L']))
def test_same_gate_through_the_kernels_it_replaces(shape, tmp_path):
    blk = Block(**shape)
    x, dy, feats, dx = _run_block(blk)
    _oracle_gate(blk, x, dy, feats, dx)
    out = str(tmp_path / 'nowide.pt')
    # a fresh child process: HUAL_CQ_NO_WIDE is read once per process
    env = dict(os.environ, HUAL_CQ_NO_WIDE='1', PYTHONPATH=os.pathsep.join([HERE, os.path.dirname(HERE)] + [q for q in sys.path if q]))
    r = subprocess.run([sys.executable, '-c', _CHILD, json.dumps(shape), out], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode()[-4000:]      # (the child asserts the oracle gate itself)
    o = torch.load(out)
    d = {k: float((o[k] - v).abs().max()) for k, v in (('feats', feats), ('dx', dx), ('grads', blk.grads.cpu()))}
    print('wide (64 short rows) against HUAL_CQ_NO_WIDE=1, largest differences:', d)
    assert all(np.isfinite(v) for v in d.values()), d


# ---------------------------------------------------------------------------------------------------- 5. graph replay, workspace
def test_steps_with_long_queries_replay_bit_identical_to_eager():
    from hual_amd.train import Trainer
    cases = [pu.make_case(B=16, T=100, L=L, C=8, seed=300 + L, max_vlen=100, vdim=64) for L in (45, 64)]
    m = pu.hip_model(*cases[0][:3])
    assert m.ws_poison == 0xFF
    tr = Trainer(m, world=1, use_graph=True)
    tr.reserve(16, 100, 64, 8)
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
    for a, b in zip(runs[0][0], runs[2][0]):
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    assert all(torch.isfinite(o[0]).all() for o in runs[2][0])


def test_no_write_outside_the_callers_buffers_long_queries():
    """forward + backward + optimizer at B=3, T=100, L=64, C=9 with every buffer carved from the arena, the workspace at exactly the
    queried size (as test_gpu_guard_bands.test_no_write_outside_the_callers_buffers)"""
    from hual_amd import lib
    B, T, L, C, V = 3, 100, 64, 9, 64
    cfg, p, wv, b, labels = pu.make_case(seed=9, B=B, T=T, L=L, C=C, vdim=V, max_vlen=100)
    m = pu.hip_model(cfg, p, wv)
    need = lib.query_workspace(m.cfg, B, T, L, C)
    tab = lib.ws_table(m.cfg, B, T, L, C)
    assert 'cq.gs' not in tab and 'd.cq.gd' not in tab            # no score scratch of the global-operand kernels for this shape
    n = m.params.numel()
    total = 25 * (GUARD + 512) + need + 4 * n * 4 + B * T * V * 4 + B * L * (C + 1) * 4 + 8 * B * T * 4 + 4096
    ar = Arena(total + (1 << 20), m.device)
    f32, i32 = torch.float32, torch.int32
    for name in ('params', 'grads', 'adam_m', 'adam_v'):
        t = ar.take(n * 4, f32)
        t.copy_(getattr(m, name))
        setattr(m, name, t)
    m._ws = ar.take((need + 255) // 256 * 256)
    m._ws_need[(B, T, L, C)] = need
    m._ws_tables[(B, T, L, C)] = tab
    video = ar.take(B * T * V * 4, f32, (B, T, V)); video.copy_(b['video'])
    lens = ar.take(B * 4, i32, (B,)); lens.copy_(b['lens'])
    words = ar.take(B * L * 4, i32, (B, L)); words.copy_(b['word_ids'])
    chars = ar.take(B * L * C * 4, i32, (B, L, C)); chars.copy_(b['char_ids'])
    lab = []
    for t, dt in zip(labels, (f32, f32, i32, f32)):
        v = ar.take(B * T * 4, dt, (B, T)); v.copy_(t.to(dt)); lab.append(v)
    outs = dict(start_logits=ar.take(B * T * 4, f32, (B, T)), end_logits=ar.take(B * T * 4, f32, (B, T)),
                match_scores=ar.take(B * T * 16, f32, (B, T, 4)), start_index=ar.take(B * 8, torch.int64, (B,)),
                end_index=ar.take(B * 8, torch.int64, (B,)))
    loss_terms = ar.take(16, f32, (4,))

    def _outputs(B_, T_, with_loss):
        st = lib.hual_outputs(*[lib.ptr(outs[k]).value for k in ('start_logits', 'end_logits', 'match_scores', 'start_index', 'end_index')],
                              lib.ptr(loss_terms).value if with_loss else None)
        return outs, (loss_terms if with_loss else None), st
    m._outputs = _outputs
    ar.check('set-up')
    m.set_rng(3, 1)
    for drop in (0.0, 0.2):
        o = m.forward(video, lens, words, chars, drop_rate=drop, labels=tuple(lab))
        torch.cuda.synchronize(); ar.check('forward, dropout %.1f' % drop)
        m.backward()
        torch.cuda.synchronize(); ar.check('backward, dropout %.1f' % drop)
        m.apply_gradients(1e-4)
        torch.cuda.synchronize(); ar.check('clip + AdamWD')
        assert torch.isfinite(o['loss']).all()
    assert torch.isfinite(m.params).all() and int(outs['start_index'].min()) >= 0
