"""GPU: model.finetune_word_emb (modules.py:8-16 with finetune=True) on the HIP path - the word table's gradient against the CPU
reference of tests/finetune_ref.py, the unchanged forward, training steps (eager and as replayed step graphs), the Runner's
checkpoints and the data-parallel step."""
import collections
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import finetune_ref as F
import parity_util as pu
from oracle import seqpan_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(cfg, p, wv, finetune=True):
    """pu.hip_model with the flag: the table starts as GloVe (load_state_dict of a dict without it keeps it)"""
    from hual_amd import lib
    from hual_amd.model import SeqPAN
    hc = lib.make_cfg(vdim=cfg.vdim, word_dim=cfg.word_dim, char_dim=cfg.char_dim, max_vlen=cfg.max_vlen, attn_layer=cfg.attn_layer,
                      num_chars=cfg.num_chars, num_words=cfg.num_words, match_lambda=cfg.match_lambda, clip_norm=cfg.clip_norm,
                      finetune_word_emb=1 if finetune else 0)
    m = SeqPAN(hc, wv.numpy())
    m.ws_poison = 0xFF
    m.load_state_dict({k: v.detach().numpy() for k, v in p.items()})
    return m


def _case(B, T, L, C, seed, max_vlen=32, num_words=60):
    cfg, p, wv, b, labels = pu.make_case(B=B, T=T, L=L, C=C, seed=seed, max_vlen=max_vlen, num_words=num_words)
    w = b['word_ids'].clone()
    g = np.random.default_rng(seed)
    qlen = (w > 0).sum(1)
    for k in range(B):               # a small vocabulary: repeated words, unk, PAD behind every query
        n = int(qlen[k])
        w[k, :n] = torch.tensor(g.integers(1, 12, size=n), dtype=w.dtype)
    w[0, :3] = torch.tensor([7, 7, 1])
    b['word_ids'] = w
    return cfg, p, wv, b, labels


@pytest.mark.parametrize('shape', [(3, 20, 6, 5), (2, 24, 79, 6)], ids=['c1', 'anet_L79'])
@pytest.mark.parametrize('drop', [0.0, 0.2])
def test_table_gradient_matches_the_reference(shape, drop):
    B, T, L, C = shape
    cfg, p, wv, b, labels = _case(B, T, L, C, seed=11, max_vlen=80)
    m = _model(cfg, p, wv)
    m.set_rng(5, 7)
    m.debug_taps = True
    h = m.forward(b['video'].numpy(), b['lens'].numpy(), b['word_ids'].numpy(), b['char_ids'].numpy(), drop_rate=drop,
                  labels=tuple(x.numpy() for x in labels))
    m.backward()
    torch.cuda.synchronize()
    pins = pu.relu_pins(m, B, T, L)
    batch = (b['video'], b['lens'], b['word_ids'], b['char_ids'])
    o, g = F.grads(F.with_table(p, wv), cfg, batch, labels, drop_rate=drop, seed=5, offset=7, relu_pin=pins, want_tap=True)
    pu.audit_pins(o['tap'], pins)
    rows = []

    def add(kind, name, hip, ref):
        hip, ref = hip.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
        rows.append((kind, name, float((hip - ref).abs().max()), float(ref.abs().max())))
        if kind == 'grad':
            pu.GL2_SIZE[name] = ref.numel()
            rows.append(('gl2', name, float((hip - ref).norm()), float(ref.norm())))
    for k in ('start_logits', 'end_logits', 'match_scores'):
        add('out', k, h[k], o[k])
    for k in ('loss', 'loc_loss', 'match_loss', 'align_loss'):
        add('loss', k, h[k], o[k])
    hg = m.grads_dict()
    assert set(hg) == set(g) and len(g) == len(m.table.entries) and F.WORD_TABLE in g
    for k, ref in g.items():
        add('grad', k, torch.from_numpy(hg[k]), ref)
    pu.assert_rows(rows)
    assert torch.equal(h['start_index'].cpu(), o['start_index']) and torch.equal(h['end_index'].cpu(), o['end_index'])
    gt = torch.from_numpy(hg[F.WORD_TABLE])
    ref = g[F.WORD_TABLE]
    assert float((gt - ref).abs().max()) <= 1e-3 * float(ref.abs().max())      # relative to the table gradient's own scale
    present = sorted(set(int(i) - 2 for i in b['word_ids'].reshape(-1) if int(i) >= 2))
    absent = [r for r in range(cfg.num_words - 2) if r not in present]
    assert float(gt[absent].abs().max()) == 0.0                                  # exactly: no row of an absent word is touched
    assert float(gt[present].abs().min(1).values.max()) > 0.0


@pytest.mark.parametrize('drop', [0.0, 0.2])
def test_forward_is_bit_identical_with_the_flag(drop):
    cfg, p, wv, b, labels = _case(3, 20, 9, 5, seed=12)
    feeds = (b['video'].numpy(), b['lens'].numpy(), b['word_ids'].numpy(), b['char_ids'].numpy())
    outs = []
    for ft in (False, True):
        m = _model(cfg, p, wv, finetune=ft)
        m.set_rng(3, 1)
        o = m.forward(*feeds, drop_rate=drop, labels=tuple(x.numpy() for x in labels))
        o2 = m.forward(*feeds)
        torch.cuda.synchronize()
        outs.append({k: v.cpu() for k, v in list(o.items()) + [('eval_' + k, v) for k, v in o2.items()]})
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), k


def test_word_table_pointer_must_be_the_entry():
    from hual_amd import lib
    cfg, p, wv, b, labels = _case(2, 16, 6, 5, seed=13)
    m = _model(cfg, p, wv)
    feeds = (b['video'].numpy(), b['lens'].numpy(), b['word_ids'].numpy(), b['char_ids'].numpy())
    ref = {k: v.cpu() for k, v in m.forward(*feeds).items()}
    own = m.word_table
    e = m.table.by_name[F.WORD_TABLE]
    assert own.data_ptr() == m.params.data_ptr() + 4 * e['offset']
    try:
        m.word_table = own.clone()                        # same values, another address: an error, not a result
        with pytest.raises(lib.HualError, match='finetune_word_emb'):
            m.forward(*feeds)
        m.word_table = own
        m.forward(*feeds, labels=tuple(x.numpy() for x in labels))
        m.word_table = own.clone()
        with pytest.raises(lib.HualError, match='finetune_word_emb'):
            m.backward()
        m.word_table = None                               # NULL: the entry
        got = {k: v.cpu() for k, v in m.forward(*feeds).items()}
    finally:
        m.word_table = own
    torch.cuda.synchronize()
    for k in ref:
        assert torch.equal(ref[k], got[k]), k


def test_training_steps_follow_the_reference():
    """teacher-forced: 8 consecutive steps as ONE replayed step graph each, the reference taking the same step from the HIP state
    with the HIP ReLU active sets (as test_gpu_train.py); then 30 free-running HIP steps, where every row of a word that is in no
    batch moves by the dense Adam update alone (m = v = 0: the weight decay) exactly as the reference's"""
    from hual_amd.train import Trainer
    lr, drop, seed, off = 1e-3, 0.2, 99, 5
    B, T, L, C = 4, 24, 7, 5
    cfg, p, wv, b, labels = _case(B, T, L, C, seed=21)
    m = _model(cfg, p, wv)
    m.set_rng(seed, off)
    tr = Trainer(m, world=1, use_graph=True)
    tr.set_batch(b['video'].numpy(), b['lens'].numpy(), b['word_ids'].numpy(), b['char_ids'].numpy(), *[x.numpy() for x in labels])
    rp = F.with_table(p, wv)
    rm = {k: torch.zeros_like(v) for k, v in rp.items()}
    rv = {k: torch.zeros_like(v) for k, v in rp.items()}
    batch = (b['video'], b['lens'], b['word_ids'], b['char_ids'])
    present = sorted(set(int(i) - 2 for i in b['word_ids'].reshape(-1) if int(i) >= 2))
    absent = [r for r in range(cfg.num_words - 2) if r not in present]
    for s in range(8):
        prev = {k: v.clone() for k, v in rp.items()}
        tr.step(lr=lr, drop_rate=drop)
        torch.cuda.synchronize()
        pins = pu.relu_pins(m, B, T, L)
        rp, rm, rv, info = F.train_step(rp, rm, rv, cfg, batch, labels, lr, drop, seed=seed, offset=off + s, relu_pin=pins,
                                        want_tap=True)
        pu.audit_pins(info['tap'], pins)
        np.testing.assert_allclose(float(tr.last_loss()), float(info['loss']), rtol=1e-3, atol=1e-3)
        assert torch.equal(tr.start_index.cpu(), info['start_index']) and torch.equal(tr.end_index.cpu(), info['end_index'])
        got = m.state_dict()
        for k, v in rp.items():
            moved = float(np.abs(v.numpy() - prev[k].numpy()).max())
            d = float(np.abs(got[k] - v.numpy()).max())
            assert d < 2e-5 + 0.02 * moved, (s, k, d, moved)
        t = got[F.WORD_TABLE]
        np.testing.assert_allclose(t[absent], rp[F.WORD_TABLE].numpy()[absent], rtol=1e-6, atol=1e-9)
        assert float(np.abs(t[present] - wv.numpy()[present]).max()) > lr       # the rows in the batch train
        rp = collections.OrderedDict((k, torch.from_numpy(got[k])) for k in rp)
        rm = {k: torch.from_numpy(a) for k, a in m.table.unpack(m.adam_m.cpu().numpy()).items()}
        rv = {k: torch.from_numpy(a) for k, a in m.table.unpack(m.adam_v.cpu().numpy()).items()}
    # free running: the absent rows against the reference's own update of a zero gradient, 30 steps, no re-seeding
    a0 = {F.WORD_TABLE: rp[F.WORD_TABLE][absent].clone()}
    z = {F.WORD_TABLE: torch.zeros_like(a0[F.WORD_TABLE])}
    am, av = dict(z), dict(z)
    for s in range(30):
        tr.step(lr=1e-4, drop_rate=drop)
        a0, am, av = R.adam_weight_decay_step(a0, z, am, av, 1e-4)
    torch.cuda.synchronize()
    t = m.state_dict()[F.WORD_TABLE]
    np.testing.assert_allclose(t[absent], a0[F.WORD_TABLE].numpy(), rtol=2e-6, atol=1e-9)
    assert np.isfinite(m.params.cpu().numpy()).all()


def test_epoch_loop_graphs_match_eager_steps():
    """Trainer.run_epoch (per-shape step graphs, device epoch cursor) with the flag on, against eager steps on fresh feeds
    (the yardstick of test_gpu_epoch_loop.py)"""
    import al_synth
    from hual_amd import al, lib
    from hual_amd.dataset import DeviceDataset
    from hual_amd.model import SeqPAN
    from hual_amd.train import Trainer
    vdim, max_vlen = 64, 24
    recs, vis, data_gt, _ = al_synth.make_trainset(64, 16, vdim, max_vlen, seed=5)
    cfg = lib.make_cfg(vdim=vdim, max_vlen=max_vlen, num_words=200, num_chars=30, finetune_word_emb=1)
    wv = np.random.default_rng(1).normal(0, 0.4, size=(198, 300)).astype(np.float32)
    ds = DeviceDataset(recs, vis)
    s0, e0 = al.labels_from_times(data_gt, ds.vlen_h)
    ds.set_labels(s0, e0)
    N, bs, lr, drop = len(ds), 16, 1e-4, 0.2
    g = np.random.default_rng(0)
    orders = [g.permutation(N).astype(np.int32) for _ in range(2)]
    m0 = SeqPAN(cfg, wv)
    m0.ws_poison = 0xFF
    t0 = Trainer(m0, world=1, use_graph=False)
    ref_spans, ref_loss = [], []
    for order in orders:
        for lo in range(0, N, bs):
            t0.set_batch_device(ds.assemble(order[lo:lo + bs], out=None, min_chars=4))
            t0.step(lr=lr, drop_rate=drop)
            ref_spans.append((t0.start_index.cpu().numpy().copy(), t0.end_index.cpu().numpy().copy()))
            ref_loss.append(float(t0.last_loss()))
    m1 = SeqPAN(cfg, wv)
    m1.ws_poison = 0xFF
    t1 = Trainer(m1, world=1, use_graph=True)
    got = [t1.run_epoch(ds, order, bs, lr=lr, drop_rate=drop, min_chars=4) for order in orders]
    torch.cuda.synchronize()
    nsteps = 2 * ((N + bs - 1) // bs)
    assert t1.stats['replayed'] > 0
    np.testing.assert_array_equal(got[0][0][:bs], ref_spans[0][0])
    np.testing.assert_array_equal(got[0][1][:bs], ref_spans[0][1])
    assert abs(float(t1.last_loss()) - ref_loss[-1]) <= 2e-2 * abs(ref_loss[-1])
    assert float((m1.params - m0.params).abs().max()) <= 2.0 * lr * nsteps * 3.2
    w0, w1 = torch.from_numpy(wv).cuda(), m1.word_table
    assert m1.word_table.data_ptr() == m1.params.data_ptr() + 4 * m1.table.by_name[F.WORD_TABLE]['offset']
    assert float((w1 - w0).abs().max()) > lr and float((w1 - m0.word_table).abs().max()) <= 2.0 * lr * nsteps * 3.2
    assert torch.isfinite(m1.params).all()


def _videos(nvid, vdim, seed):
    g = np.random.default_rng(seed)
    vis = {}
    for v in range(nvid):
        T = int(g.integers(20, 33))
        f = 0.1 * g.standard_normal((T, vdim)).astype(np.float32)
        f[:, 0] = np.linspace(-1, 1, T)
        vis['v%d' % v] = f
    return vis


def _task(n, vis, seed):
    g = np.random.default_rng(seed)
    recs = []
    for i in range(n):
        vid = 'v%d' % int(g.integers(0, len(vis)))
        T = vis[vid].shape[0]
        part = int(g.integers(0, 3))
        s = part * T // 3 + 1
        e = min(T - 1, s + T // 3 - 2)
        words = ['w%d' % (2 + part), 'w%d' % int(g.integers(5, 30)), 'w%d' % int(g.integers(5, 30))]
        recs.append(dict(vid=vid, duration=float(T), v_len=T, words=words, w_ids=[int(w[1:]) for w in words],
                         c_ids=[[1 + part, 2, 3, 4]] * 3, s_ind=s, e_ind=e))
    return recs


def test_runner_trains_checkpoints_and_reloads_the_table(tmp_path):
    from hual_amd import lib
    from hual_amd.runner import Runner
    vdim = 64
    vis = _videos(12, vdim, 0)
    train, test = _task(64, vis, 1), _task(32, vis, 2)
    model = dict(vdim=vdim, dim=128, num_heads=8, word_dim=300, char_dim=50, max_vlen=32, attn_layer=2)
    cfg = dict(task='synth', train=dict(batch_size=16, droprate=0.1, lr=2e-3, epochs=2, clip_norm=1.0),
               model=dict(model, finetune_word_emb=True), loss=dict(match_lambda=1.0, tau=0.3, no_gumbel=True), num_chars=10)
    frozen = dict(cfg, model=model)
    wv = np.random.default_rng(0).normal(0, 0.4, size=(40, 300)).astype(np.float32)
    lines = []

    class Log:
        def info(self, s):
            lines.append(str(s))
    r = Runner(cfg, wv, train, test, vis, ckpt_dir=str(tmp_path / 'ft'), logger=Log())
    assert r.model.finetune_word_emb
    r.train()
    path = str(tmp_path / 'ft' / 'best_SeqPAN.npz')
    with np.load(path) as z:
        t = z['word_embs|word_table']
    assert t.shape == wv.shape and float(np.abs(t - wv).max()) > 1e-4
    t_best = r.test()
    r.model.params.add_(0.05 * torch.randn_like(r.model.params))
    r.load(path)
    assert r.test_epoch() == t_best
    assert np.array_equal(r.model.word_table.cpu().numpy(), t)
    # a frozen run's checkpoint into a fine-tuning model: the table stays GloVe, and the log says so
    rf = Runner(frozen, wv, train, test, vis, ckpt_dir=str(tmp_path / 'fz'), logger=Log())
    fpath = str(tmp_path / 'fz' / 'frozen.npz')
    rf.save(fpath)
    r2 = Runner(cfg, wv, train, test, vis, ckpt_dir=str(tmp_path / 'ft2'), logger=Log())
    r2.model.word_table.add_(1.0)
    r2.load(fpath)
    assert np.array_equal(r2.model.word_table.cpu().numpy(), wv + np.float32(1.0))
    assert any('word_embs/word_table' in l and 'GloVe' in l for l in lines)
    for k, v in rf.model.state_dict().items():
        assert np.array_equal(r2.model.state_dict()[k], v), k
    # a fine-tuned checkpoint into a frozen model: refused, naming the key
    with pytest.raises(lib.HualError, match='finetune_word_emb'):
        rf.load(path)


def _dp_case():
    cfg, p, wv, b, labels = _case(4, 18, 6, 5, seed=33, max_vlen=24)
    return cfg, p, wv, b, labels


def _dp_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from hual_amd.train import Trainer
    cfg, p, wv, b, labels = _dp_case()
    sl = slice(rank * 2, rank * 2 + 2)
    m = _model(cfg, p, wv)
    tr = Trainer(m, world=world, use_graph=False)
    tr.set_batch(b['video'][sl].numpy(), b['lens'][sl].numpy(), b['word_ids'][sl].numpy(), b['char_ids'][sl].numpy(),
                 *[x[sl].numpy() for x in labels])
    tr.step(lr=1e-3, drop_rate=0.0)
    torch.cuda.synchronize()
    q.put((rank, m.grads_dict()[F.WORD_TABLE] / world, m.state_dict()[F.WORD_TABLE], m.params.cpu().numpy()))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_match_the_single_process_step():
    from hual_amd.train import Trainer
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 29500 + (os.getpid() % 150) + 17
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for pr in procs:
        pr.start()
    got = {}
    for _ in range(2):
        rank, g, t, par = q.get(timeout=300)
        got[rank] = (g, t, par)
    for pr in procs:
        pr.join(timeout=120)
        assert pr.exitcode == 0
    cfg, p, wv, b, labels = _dp_case()
    m = _model(cfg, p, wv)
    tr = Trainer(m, world=1, use_graph=False)
    tr.set_batch(b['video'].numpy(), b['lens'].numpy(), b['word_ids'].numpy(), b['char_ids'].numpy(), *[x.numpy() for x in labels])
    tr.step(lr=1e-3, drop_rate=0.0)
    torch.cuda.synchronize()
    g1, t1 = m.grads_dict()[F.WORD_TABLE], m.state_dict()[F.WORD_TABLE]
    assert float(np.abs(g1).max()) > 0
    assert np.abs(got[0][0] - g1).max() <= 1e-3 * float(np.abs(g1).max())
    assert np.array_equal(got[0][2], got[1][2])                      # replicas stay identical, the table included
    assert np.abs(got[0][1] - t1).max() < 2.5e-3
    assert np.abs(got[0][1] - wv.numpy()).max() > 1e-4
