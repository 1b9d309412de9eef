"""CPU: model.finetune_word_emb (modules.py:8-16 with finetune=True) - the parameter layout with the GloVe table as its last entry,
the config default, and the CPU reference train step of tests/finetune_ref.py checked against hand-written restatements."""
import collections

import numpy as np
import pytest
import torch

import finetune_ref as F
from oracle import seqpan_ref as R


def _tables(**kw):
    from hual_amd import build, lib
    build.build()
    off = lib.param_table(lib.make_cfg(**kw))
    on = lib.param_table(lib.make_cfg(finetune_word_emb=1, **kw))
    return off, on


@pytest.mark.parametrize('num_words', [500, 1502, 12002])
def test_param_table_with_the_flag_off_and_on(num_words):
    (e0, pad0, n0), (e1, pad1, n1) = _tables(num_chars=40, num_words=num_words)
    if num_words == 500:
        assert n0 == 1186508                                 # the Charades layout of ABI 9, unchanged
    assert F.WORD_TABLE not in [e['name'] for e in e0]
    assert e1[:-1] == e0                                      # every other entry: same name, offset, size, shape, decay
    t = e1[-1]
    assert t['name'] == F.WORD_TABLE and t['shape'] == [num_words - 2, 300] and t['size'] == (num_words - 2) * 300
    assert t['decay'] and R.uses_weight_decay(t['name'])     # ops.py:123: no LayerNorm|layer_norm|bias in the name
    assert t['offset'] == pad0 and (t['offset'] * 4) % 16 == 0
    assert n1 == n0 + t['size'] and pad1 == pad0 + ((t['size'] + 3) & ~3) and pad1 % 4 == 0


def test_init_keeps_every_other_value_and_starts_from_glove():
    from hual_amd import lib
    from hual_amd.params import ParamTable
    wv = np.random.default_rng(3).normal(0, 0.3, size=(58, 300)).astype(np.float32)
    t0 = ParamTable(lib.make_cfg(num_words=60))
    t1 = ParamTable(lib.make_cfg(num_words=60, finetune_word_emb=1))
    f0, f1 = t0.init_flat(7), t1.init_flat(7, wv)
    assert np.array_equal(f1[:t0.padded], f0)                 # no generator draw for the table entry
    e = t1.by_name[F.WORD_TABLE]
    assert np.array_equal(f1[e['offset']:e['offset'] + e['size']].reshape(58, 300), wv)
    with pytest.raises(lib.HualError):
        t1.init_flat(7)
    d = t1.decay_flat()
    assert np.all(d[e['offset']:e['offset'] + e['size']] == np.float32(0.01))


def test_config_key_defaults_to_frozen():
    from hual_amd import lib
    from hual_amd.model import cfg_from_configs
    base = dict(model=dict(vdim=1024, dim=128, num_heads=8, word_dim=300, char_dim=50, max_vlen=64, attn_layer=2), num_chars=40)
    assert cfg_from_configs(base, 500).finetune_word_emb == 0
    on = dict(base, model=dict(base['model'], finetune_word_emb=True))
    assert cfg_from_configs(on, 500).finetune_word_emb == 1
    assert lib.make_cfg().finetune_word_emb == 0
    bad = lib.make_cfg(finetune_word_emb=2)
    assert lib.load().hual_seqpan_validate(bad) != 0 and b'finetune_word_emb' in lib.load().hual_last_error()


def _case(drop, seed=4):
    cfg = R.default_cfg(max_vlen=24, num_words=40, vdim=64)
    p = R.init_params(cfg, seed=1)
    wv = R.init_word_vectors(cfg)
    b = R.synthetic_batch(cfg, 3, 16, 7, 5, seed=seed)
    w = b['word_ids'].clone()
    w[0, :4] = torch.tensor([5, 5, 1, 9])                     # a repeated word and unk; PAD rows stay as synthetic_batch made them
    w[1, :2] = torch.tensor([9, 1])
    w[1, 5:] = 0
    b['word_ids'] = w
    from hual_amd import data
    y1, y2, m, i = data.make_labels(b['s_ind'], b['e_ind'], b['lens'].numpy(), max_len=16)
    labels = (torch.tensor(y1), torch.tensor(y2), torch.tensor(m), torch.tensor(i, dtype=torch.float32))
    return cfg, F.with_table(p, wv), (b['video'], b['lens'], b['word_ids'], b['char_ids']), labels


@pytest.mark.parametrize('drop', [0.0, 0.2])
def test_reference_table_gradient_is_the_scatter_of_the_word_embedding_gradient(drop):
    """d word_table[id - 2] = sum over positions with that id of the gradient of the (dropped) word embedding (modules.py:15)"""
    cfg, p, batch, labels = _case(drop)
    out, g = F.grads(p, cfg, batch, labels, drop_rate=drop, seed=3, offset=2, want_tap=True)
    # the same loss with the word embedding rows as leaves: the gradient w.r.t. the looked-up rows, before the dropout
    wid = batch[2]
    table = torch.cat([torch.zeros(1, 300), p['word_embs/unk'], p[F.WORD_TABLE]], 0)
    rows = table[wid.long()].clone().requires_grad_(True)
    orig = R.word_embs

    def word_embs(word_ids, pp, word_vectors, rng, rows_q):
        assert torch.equal(word_ids, wid)
        return R._dropout(rows, rng, R.px.SITE_WORD, rows_q)
    R.word_embs = word_embs
    try:
        pr = collections.OrderedDict((k, v) for k, v in p.items() if k != F.WORD_TABLE)
        o2 = R.forward(pr, cfg, p[F.WORD_TABLE], *batch, drop_rate=drop, seed=3, offset=2, labels=labels)
    finally:
        R.word_embs = orig
    torch.testing.assert_close(o2['loss'], out['loss'], rtol=0, atol=0)
    (drow,) = torch.autograd.grad(o2['loss'], [rows])
    want = torch.zeros_like(p[F.WORD_TABLE])
    unk = torch.zeros(300)
    for b in range(wid.shape[0]):
        for l in range(wid.shape[1]):
            i = int(wid[b, l])
            if i >= 2:
                want[i - 2] += drow[b, l]
            elif i == 1:
                unk += drow[b, l]
    torch.testing.assert_close(g[F.WORD_TABLE], want, rtol=1e-5, atol=1e-7)
    torch.testing.assert_close(g['word_embs/unk'][0], unk, rtol=1e-5, atol=1e-7)
    present = set(int(i) - 2 for i in wid.reshape(-1) if int(i) >= 2)
    absent = [r for r in range(want.shape[0]) if r not in present]
    assert absent and float(g[F.WORD_TABLE][absent].abs().max()) == 0.0
    assert float(g[F.WORD_TABLE][sorted(present)].abs().max()) > 0.0


def test_reference_adam_step_is_dense_and_decays_absent_rows():
    """ops.py:166-170: the IndexedSlices gradient becomes dense in the first moment, so a row whose word is not in the batch still
    moves, by the weight decay alone (its m and v stay 0)"""
    cfg, p, batch, labels = _case(0.0)
    m = {k: torch.zeros_like(v) for k, v in p.items()}
    v = {k: torch.zeros_like(t) for k, t in p.items()}
    lr = 1e-3
    p2, m2, v2, info = F.train_step(p, m, v, cfg, batch, labels, lr, 0.0)
    gt = info['grads'][F.WORD_TABLE]
    absent = (gt.abs().sum(1) == 0).nonzero().reshape(-1)
    present = (gt.abs().sum(1) != 0).nonzero().reshape(-1)
    assert len(absent) > 0 and len(present) > 0
    w0, w1 = p[F.WORD_TABLE], p2[F.WORD_TABLE]
    torch.testing.assert_close(w1[absent], w0[absent] - lr * 0.01 * w0[absent], rtol=0, atol=1e-9)
    assert float(m2[F.WORD_TABLE][absent].abs().max()) == 0.0 and float(v2[F.WORD_TABLE][absent].abs().max()) == 0.0
    assert float((w1[present] - w0[present]).abs().max()) > 10 * lr * 0.01 * float(w0.abs().max())
    # the clip saw the table: the norm is that of every gradient including it
    gn = torch.sqrt(sum((x.double() ** 2).sum() for x in F.grads(p, cfg, batch, labels)[1].values()))
    torch.testing.assert_close(info['grad_norm'].double(), gn, rtol=1e-5, atol=0)
