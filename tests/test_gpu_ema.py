"""GPU: averaged weights (train.ema_decay) in the optimizer launch and the training-state resume.

The shadow's recurrence  s_k = s_{k-1} + (1 - d_k) (p_k - s_{k-1}),  d_k = min(decay, (1 + k) / (10 + k)) with warm-up, is evaluated
here in float64 on the float32 parameter values fetched after every update.  Bound after k updates: 4 k 2^-24 max|p| - three float32
roundings per update (p - s, the product, the sum; the device forms 1 - d_k with one more) of values no larger than 2 max|p|, each
damped by d_j < 1 afterwards, with a margin of one."""
import ctypes

import numpy as np
import pytest
import torch

import al_synth
import parity_util as pu

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
DECAY = 0.999


def _d(k, decay, warmup):
    d = float(np.float32(decay))
    return min(d, (1.0 + k) / (10.0 + k)) if warmup else d


class _Recurrence:
    """the float64 reference and its running bound"""

    def __init__(self, s0, decay=DECAY, warmup=True):
        self.s = s0.detach().double().cpu().clone()
        self.pmax = float(self.s.abs().max())
        self.k, self.decay, self.warmup = 0, decay, warmup

    def update(self, p):
        p = p.detach().double().cpu()
        self.k += 1
        self.s += (1.0 - _d(self.k, self.decay, self.warmup)) * (p - self.s)
        self.pmax = max(self.pmax, float(p.abs().max()))

    def check(self, shadow, factor=None):
        err = float((shadow.detach().double().cpu() - self.s).abs().max())
        bound = (4.0 * self.k if factor is None else factor) * U * self.pmax
        print('update %2d: d_k %.6f  |shadow - float64 recurrence| %.3e  bound %.3e' % (self.k, _d(self.k, self.decay, self.warmup), err, bound))
        assert err <= bound, 'update %d: shadow off by %.3e, bound %.3e' % (self.k, err, bound)


# ---------------------------------------------------------------------------------------------------- 1. the kernel alone
N_FLAT = 4 * (256 * 512 + 3)      # more float4s than one pass of the 512 x 256 grid, and not a multiple of it


def _optimizer_state(seed=0):
    g = torch.Generator().manual_seed(seed)
    n = N_FLAT
    st = dict(p=torch.randn(n, generator=g), g=0.1 * torch.randn(n, generator=g), m=0.01 * torch.randn(n, generator=g),
              v=1e-4 * torch.rand(n, generator=g), decay=0.01 * (torch.rand(n, generator=g) < 0.5).float(),
              s=torch.randn(n, generator=g))
    return {k: t.cuda() for k, t in st.items()}


@pytest.mark.parametrize('warmup', [True, False], ids=['warmup', 'constant'])
def test_kernel_average_follows_the_recurrence_and_leaves_the_update_alone(warmup):
    from hual_amd import lib
    l = lib.load()
    a = _optimizer_state()
    b = {k: t.clone() for k, t in a.items()}      # the same sequence through hual_adamw_clip_step_loop
    dev = a['p'].device
    lr = torch.full((1,), 1e-2, device=dev)
    sq = [torch.zeros(256, device=dev) for _ in range(2)]
    rng = [torch.tensor([1, 2, 0], dtype=torch.int32, device=dev) for _ in range(2)]
    cur = [torch.zeros(2, dtype=torch.int64, device=dev) for _ in range(2)]
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    ref = _Recurrence(a['s'], DECAY, warmup)
    s0 = a['s'].double().cpu()
    for k in range(1, 13):
        lib.check(l.hual_adamw_clip_step_ema(lib.ptr(a['p']), lib.ptr(a['g']), lib.ptr(a['m']), lib.ptr(a['v']), lib.ptr(a['decay']), N_FLAT,
                                             lib.ptr(lr), 1.0, 1.0, lib.ptr(sq[0]), lib.ptr(rng[0]), lib.ptr(cur[0]), None, None, 0, 4, 0,
                                             lib.ptr(a['s']), lib.ptr(count), DECAY, int(warmup), lib.stream_ptr()))
        lib.check(l.hual_adamw_clip_step_loop(lib.ptr(b['p']), lib.ptr(b['g']), lib.ptr(b['m']), lib.ptr(b['v']), lib.ptr(b['decay']), N_FLAT,
                                              lib.ptr(lr), 1.0, 1.0, lib.ptr(sq[1]), lib.ptr(rng[1]), lib.ptr(cur[1]), None, None, 0, 4, 0,
                                              lib.stream_ptr()))
        torch.cuda.synchronize()
        for name in ('p', 'm', 'v'):      # the average must not perturb the update: bit-equal
            assert torch.equal(a[name], b[name]), (k, name)
        assert torch.equal(rng[0], rng[1]) and torch.equal(cur[0], cur[1])
        assert int(count.item()) == k
        ref.update(a['p'])
        ref.check(a['s'])
        if k == 1:
            # d_1 explicitly: 2/11 with warm-up (an off-by-one in k gives 1/10 or 3/12), the target decay without
            d1 = 2.0 / 11.0 if warmup else float(np.float32(DECAY))
            want = s0 + (1.0 - d1) * (a['p'].double().cpu() - s0)
            err = float((a['s'].double().cpu() - want).abs().max())
            print('first update: d_1 %.6f  error %.3e  bound %.3e' % (d1, err, 8 * U * ref.pmax))
            assert err <= 8 * U * ref.pmax, (err, 8 * U * ref.pmax)
    assert int(count.item()) == 12 and int(rng[0][2].item()) == 12 and int(cur[0][0].item()) == 48
    assert not torch.equal(a['s'], a['p'])


# ---------------------------------------------------------------------------------------------------- models
def _model(cfg, p, wv, ema_decay=DECAY, warmup=True, finetune=False, seed=12345):
    from hual_amd import lib
    from hual_amd.model import SeqPAN
    hc = lib.make_cfg(vdim=cfg.vdim, word_dim=cfg.word_dim, char_dim=cfg.char_dim, max_vlen=cfg.max_vlen, attn_layer=cfg.attn_layer,
                      num_chars=cfg.num_chars, num_words=cfg.num_words, match_lambda=cfg.match_lambda, clip_norm=cfg.clip_norm,
                      finetune_word_emb=1 if finetune else 0)
    m = SeqPAN(hc, wv.numpy(), seed=seed, ema_decay=ema_decay, ema_warmup=warmup)
    m.ws_poison = 0xFF
    m.load_state_dict({k: v.detach().numpy() for k, v in p.items()})
    return m


@pytest.fixture(scope='module')
def case():
    return pu.make_case(B=3, T=20, L=6, C=5, max_vlen=32, vdim=256)


def _set_batch(tr, b, labels):
    tr.set_batch(b['video'].numpy(), b['lens'].numpy(), b['word_ids'].numpy(), b['char_ids'].numpy(), *(x.numpy() for x in labels))


def _fwd(m, b, labels=None, drop=0.0):
    return m.forward(b['video'].numpy(), b['lens'].numpy(), b['word_ids'].numpy(), b['char_ids'].numpy(), drop_rate=drop,
                     labels=None if labels is None else tuple(x.numpy() for x in labels))


FETCHES = ('start_logits', 'end_logits', 'match_scores', 'start_index', 'end_index')


def _same(o1, o2, keys=FETCHES):
    return all(torch.equal(o1[k], o2[k]) for k in keys)


# ---------------------------------------------------------------------------------------------------- 2. graph replay
def test_replayed_step_graph_counts_its_updates_on_the_device(case):
    """the first capture and 11 replays of one shape: k comes from the device counter - baked into the capture it would stay 1 and the
    shadow would leave the warm-up schedule at the third step"""
    from hual_amd.train import Trainer
    cfg, p, wv, b, labels = case
    m = _model(cfg, p, wv)
    assert torch.equal(m.ema, m.params) and int(m.ema_count.item()) == 0
    ref = _Recurrence(m.params)
    tr = Trainer(m, world=1, use_graph=True)
    _set_batch(tr, b, labels)
    snaps = []
    for k in range(12):
        tr.step(lr=1e-3, drop_rate=0.2)
        snaps.append((m.params.clone(), m.ema.clone(), m.ema_count.clone()))
    torch.cuda.synchronize()
    assert tr.graph is not None
    for k, (pk, sk, ck) in enumerate(snaps, 1):
        assert int(ck.item()) == k
        ref.update(pk)
        ref.check(sk)
    assert m.global_step == 12 and int(m.rng_state[2].item()) == 12


# ---------------------------------------------------------------------------------------------------- 3. epoch loop
def test_epoch_loop_updates_the_average_every_step():
    from hual_amd import al, lib
    from hual_amd.dataset import DeviceDataset
    from hual_amd.model import SeqPAN
    from hual_amd.train import Trainer
    recs, vis, data_gt, _ = al_synth.make_trainset(24, 8, 64, 24, seed=5)
    ds = DeviceDataset(recs, vis)
    s0, e0 = al.labels_from_times(data_gt, ds.vlen_h)
    ds.set_labels(s0, e0)
    cfg = lib.make_cfg(vdim=64, max_vlen=24, num_words=200, num_chars=30)
    wv = np.random.default_rng(1).normal(0, 0.4, size=(198, 300)).astype(np.float32)
    m = SeqPAN(cfg, wv, ema_decay=DECAY)
    tr = Trainer(m, world=1, use_graph=True)
    g = np.random.default_rng(0)
    st, en = tr.run_epoch(ds, g.permutation(24).astype(np.int32), 4, lr=1e-3, drop_rate=0.2, min_chars=4)
    assert len(st) == 24 and int(m.ema_count.item()) == 6 == m.global_step
    assert not torch.equal(m.ema, m.params) and torch.isfinite(m.ema).all()
    tr.run_epoch(ds, g.permutation(24).astype(np.int32), 4, lr=1e-3, drop_rate=0.2, min_chars=4)
    assert int(m.ema_count.item()) == 12 == m.global_step      # the second epoch continues the count
    assert tr.stats['replayed'] > 0


# ---------------------------------------------------------------------------------------------------- 4. selecting weights
@pytest.mark.parametrize('finetune', [False, True], ids=['frozen_table', 'finetune_word_emb'])
def test_use_weights_reads_the_shadow_without_a_copy(case, finetune):
    from hual_amd.params import WORD_TABLE
    from hual_amd.train import Trainer
    cfg, p, wv, b, labels = case
    m = _model(cfg, p, wv, finetune=finetune)
    tr = Trainer(m, world=1, use_graph=False)
    _set_batch(tr, b, labels)
    for _ in range(3):
        tr.step(lr=1e-2, drop_rate=0.0)
    raw = _fwd(m, b)
    ptrs = (m.params.data_ptr(), m.ema.data_ptr(), m.word_table.data_ptr())
    with m.use_weights('ema'):
        assert m.weights == 'ema'
        avg = _fwd(m, b)
        flat, table = m._read_weights()
        assert flat.data_ptr() == m.ema.data_ptr()
        if finetune:      # the word table view follows: the matching slice of the shadow
            e = m.table.by_name[WORD_TABLE]
            assert table.data_ptr() == m.ema.data_ptr() + 4 * e['offset'] and table.shape == m.word_table.shape
        else:
            assert table.data_ptr() == m.word_table.data_ptr()
        with m.use_weights('raw'):
            assert _same(_fwd(m, b), raw)
        assert m.weights == 'ema'
    assert m.weights == 'raw' and ptrs == (m.params.data_ptr(), m.ema.data_ptr(), m.word_table.data_ptr())
    assert _same(_fwd(m, b), raw)                                   # leaving the context restores the raw outputs bit for bit
    assert not torch.equal(avg['start_logits'], raw['start_logits'])
    # a second model whose PARAMETERS are the shadow computes the same bits
    m2 = _model(cfg, p, wv, ema_decay=0.0, finetune=finetune)
    assert m2.ema is None
    m2.params.copy_(m.ema)
    assert _same(_fwd(m2, b), avg)


def test_use_weights_without_average_raises(case):
    from hual_amd import lib
    cfg, p, wv, b, labels = case
    m = _model(cfg, p, wv, ema_decay=0.0)
    with pytest.raises(lib.HualError, match='ema_decay'):
        with m.use_weights('ema'):
            pass
    m1 = _model(cfg, p, wv)
    with pytest.raises(lib.HualError):
        with m1.use_weights('average'):
            pass


# ---------------------------------------------------------------------------------------------------- 5. off means off
def _prof(l, fn):
    from hual_amd import lib
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


def test_without_the_keys_the_step_is_what_it_was(case):
    from hual_amd import lib
    from hual_amd.train import Trainer
    cfg, p, wv, b, labels = case
    got = {}
    for decay in (0.0, DECAY):
        m = _model(cfg, p, wv, ema_decay=decay)
        assert (m.ema is None and m.ema_count is None) if decay == 0.0 else (m.ema is not None)
        tr = Trainer(m, world=1, use_graph=False)
        _set_batch(tr, b, labels)
        tr.step(lr=1e-3, drop_rate=0.2)              # (first-use calls, job table) outside the recording
        torch.cuda.synchronize()
        got[decay] = _prof(lib.load(), lambda: tr.step(lr=1e-3, drop_rate=0.2))
    assert got[0.0] == got[DECAY], (got[0.0], got[DECAY])
    assert got[0.0]['sqnorm_kernel'] == 1 and got[0.0]['adamw_kernel'] == 1, got[0.0]


# ---------------------------------------------------------------------------------------------------- runners
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


class _Log:
    def info(self, s):
        pass


def _runner(tmp_path, name, seed, ema_decay=DECAY, test=False):
    from hual_amd.runner import Runner
    vdim = 64
    vis = _videos(8, vdim, 0)
    train_cfg = dict(batch_size=4, droprate=0.2, lr=1e-3, epochs=3, clip_norm=1.0)
    if ema_decay is not None:
        train_cfg['ema_decay'] = ema_decay
    cfg = dict(task='synth', train=train_cfg,
               model=dict(vdim=vdim, dim=128, num_heads=8, word_dim=300, char_dim=50, max_vlen=32, attn_layer=2),
               loss=dict(match_lambda=1.0, tau=0.3, no_gumbel=True), num_chars=10)
    wv = np.random.default_rng(0).normal(0, 0.4, size=(40, 300)).astype(np.float32)
    return Runner(cfg, wv, _task(24, vis, 1), _task(8, vis, 2) if test else None, vis, seed=seed, ckpt_dir=str(tmp_path / name),
                  logger=_Log())


def test_checkpoint_keys_with_and_without_average(tmp_path):
    """off: the .npz of save() has exactly the key set of state_dict(); on: TensorFlow's <name>/ExponentialMovingAverage for every
    variable plus the counter, restored by load() and evaluated by default"""
    from hual_amd import lib
    from hual_amd.model import EMA_COUNT, EMA_SUFFIX
    off = _runner(tmp_path, 'off', 1, ema_decay=None)
    assert off.model.ema is None
    off.save(str(tmp_path / 'off.npz'))
    with np.load(str(tmp_path / 'off.npz')) as z:
        assert {k.replace('|', '/') for k in z.files} == set(off.model.state_dict())
    on = _runner(tmp_path, 'on', 1, test=True)
    on.train_epoch(1e-2)
    on.save(str(tmp_path / 'on.npz'))
    names = set(on.model.state_dict())
    with np.load(str(tmp_path / 'on.npz')) as z:
        assert {k.replace('|', '/') for k in z.files} == names | {n + EMA_SUFFIX for n in names} | {EMA_COUNT}
        assert int(z[EMA_COUNT.replace('/', '|')][0]) == 6
    # evaluation reads the averaged weights by default, and says which on request
    t_ema, t_raw = on.test_epoch(), on.test_epoch(weights='raw')
    assert on.test_epoch(weights='ema') == t_ema
    shadow, params = on.model.ema.clone(), on.model.params.clone()
    on.model.ema.zero_()
    on.model.ema_count.zero_()
    on.model.params.add_(1.0)
    on.load(str(tmp_path / 'on.npz'))
    assert torch.equal(on.model.ema, shadow) and torch.equal(on.model.params, params) and int(on.model.ema_count.item()) == 6
    assert on.test_epoch() == t_ema and on.test_epoch(weights='raw') == t_raw
    # a checkpoint without averaged entries: the shadow restarts from the loaded parameters, the count from 0
    on.load(str(tmp_path / 'off.npz'))
    assert torch.equal(on.model.ema, on.model.params) and int(on.model.ema_count.item()) == 0
    with pytest.raises(lib.HualError, match='ema_decay'):
        off.test_epoch(dataset=on.test_set, weights='ema')


# ---------------------------------------------------------------------------------------------------- 6. resume
def test_training_state_resumes_bit_for_bit(tmp_path):
    from hual_amd import lib
    path = str(tmp_path / 'state' / 'run.state')
    A = _runner(tmp_path, 'a', 1)
    A.run_one_epoch()
    A.save_state(path)
    A.save_state(path)                                             # over an existing file; nothing else is left behind
    assert [f.name for f in (tmp_path / 'state').iterdir()] == ['run.state']
    sel = np.arange(4)

    def fixed_forward(r):
        f = r.train_set.assemble(sel, labels=True, min_chars=4)
        outs = []
        for w in ('raw', 'ema'):
            with r.model.use_weights(w):
                outs.append(r.model.forward(f['video'], f['video_seq_len'], f['word_ids'], f['char_ids'], drop_rate=0.2,
                                            labels=(f['y1'], f['y2'], f['match_labels'], f['inner_labels'])))
        return outs
    oa = fixed_forward(A)
    B = _runner(tmp_path, 'b', 2)
    assert not torch.equal(B.model.params, A.model.params)
    B.load_state(path)
    ob = fixed_forward(B)
    for x, y in zip(oa, ob):
        assert _same(x, y, FETCHES + ('loss', 'loc_loss', 'match_loss', 'align_loss'))
    assert not torch.equal(oa[0]['start_logits'], oa[1]['start_logits'])
    for name in ('params', 'adam_m', 'adam_v', 'ema', 'ema_count', 'rng_state'):
        assert torch.equal(getattr(A.model, name), getattr(B.model, name)), name
    assert int(A.model.ema_count.item()) == 6 and A.model.global_step == B.model.global_step == 6
    assert A.progress == B.progress and A.progress['epoch'] == 1 and A.progress['epochs'] == 3
    # the continuation: the same lr and the same shuffle (the parameters after it are NOT compared: float atomics in the weight-gradient
    # sums, two uninterrupted runs differ as well)
    assert A.cur_lr() == B.cur_lr() == 1e-3 * (1.0 - 1.0 / 3.0)
    A.train_epoch(A.cur_lr())
    B.train_epoch(B.cur_lr())
    np.testing.assert_array_equal(A.trainer.last_epoch_ids, B.trainer.last_epoch_ids)
    assert int(B.model.ema_count.item()) == 12 and int(B.model.rng_state[2].item()) == int(A.model.rng_state[2].item()) == 12
    # a state with averaged weights into a run without them, and the reverse
    C = _runner(tmp_path, 'c', 1, ema_decay=None)
    with pytest.raises(lib.HualError, match=r'train\.ema_decay'):
        C.load_state(path)
    path_c = str(tmp_path / 'state' / 'c.state')
    C.save_state(path_c)
    with pytest.raises(lib.HualError, match=r'train\.ema_decay'):
        A.load_state(path_c)
    # train(resume=...) goes on where the file stands and writes the state after every epoch
    D = _runner(tmp_path, 'd', 3)
    with pytest.raises(lib.HualError, match='epochs'):
        D.train(epochs=5, resume=path)
    D.train(resume=path, state_path=path)
    assert D.progress['epoch'] == 3 and D.model.global_step == 18 and int(D.model.ema_count.item()) == 18
    E = _runner(tmp_path, 'e', 4)
    E.load_state(path)
    assert E.progress == D.progress and torch.equal(E.model.ema, D.model.ema)
