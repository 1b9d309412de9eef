"""GPU: the K-pass MC-dropout uncertainty bank - hual_al_mc_fold against the numpy fold (tests/mc_uncert_ref.py), what a fold may
write, hual_al_score_mc against hual_al_score at K = 2, and the K-pass infer_trainset / update_labels / run_round path on one and on
two ranks.  Float fields within 1e-6 (the bar of the active-learning tests), everything that is a selection or a copy bit for bit."""
import copy
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import al_synth
import mc_uncert_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x7fc0dead       # (as int32 bits) a NaN payload no arithmetic produces


def _poison(bank):
    for t in (bank.s0, bank.e0, bank.stats, bank.tlen):
        t.view(torch.int32).fill_(SENTINEL)


def _is_sentinel(t):
    return t.view(torch.int32) == SENTINEL


def _fold_case(N, ld, batches, K, seed, order=None):
    """batches: list of (rows, T_b, v_len list).  Folds k = 0 and K stochastic passes of seeded logits into a poisoned bank.
    Returns (bank, {row: (T_b, v_len, det logits [2,T], pass logits [K,2,T])})"""
    from hual_amd import al
    g = np.random.default_rng(seed)
    bank = al.McBank(N, ld)
    _poison(bank)
    truth = {}
    for rows, T, vl in batches:
        B = len(rows)
        det = (g.standard_normal((B, 2, T)) * 1.5).astype(np.float32)
        ps = (det[None] + 0.3 * g.standard_normal((K, B, 2, T))).astype(np.float32)
        v = torch.tensor(vl, dtype=torch.int32, device=bank.dev)
        bank.fold(rows, v, torch.from_numpy(det[:, 0].copy()).to(bank.dev), torch.from_numpy(det[:, 1].copy()).to(bank.dev), 0)
        for j, k in enumerate(order if order is not None else range(K)):
            bank.fold(np.asarray(rows), v, torch.from_numpy(ps[k, :, 0].copy()).to(bank.dev),
                      torch.from_numpy(ps[k, :, 1].copy()).to(bank.dev), j + 1)
        for b, n in enumerate(rows):
            truth[n] = (T, vl[b], det[b], ps[:, b])
    torch.cuda.synchronize()
    return bank, truth


def _check_fold(bank, truth, K):
    st = bank.stats.cpu().numpy()
    s0, e0, tlen = bank.s0.cpu().numpy(), bank.e0.cpu().numpy(), bank.tlen.cpu().numpy()
    for n, (T, v, det, ps) in truth.items():
        assert tlen[n] == T
        np.testing.assert_array_equal(s0[n, :T], det[0])
        np.testing.assert_array_equal(e0[n, :T], det[1])
        for h in range(2):
            p = R.probs(ps[:, h], v)                                      # [K, T]
            f = R.fold_passes(p)
            lo, hi, mean, m2 = st[h, :, n, :T]
            assert np.abs(lo - f.lo).max() <= 1e-6 and np.abs(hi - f.hi).max() <= 1e-6 and np.abs(mean - f.mean).max() <= 1e-6
            std = np.sqrt(2.0) * np.sqrt(m2.astype(np.float64) / (K - 1))
            assert np.abs(std - R.spread64(p)).max() <= 1e-6, (n, h, np.abs(std - R.spread64(p)).max())
            assert (lo[v:] == 0).all() and (hi[v:] == 0).all() and (m2[v:] == 0).all()          # p = 0 at t >= v_len
    # what a fold may write: columns [0, T_b) of the listed rows, nothing else
    touched = torch.zeros(bank.N, bank.ld, dtype=torch.bool)
    for n, (T, _, _, _) in truth.items():
        touched[n, :T] = True
    touched = touched.to(bank.dev)
    for t in (bank.s0, bank.e0) + tuple(bank.stats[h, j] for h in range(2) for j in range(4)):
        assert bool(_is_sentinel(t)[~touched].all()), 'a fold wrote outside its rows'
        assert not bool(_is_sentinel(t)[touched].any())
    rows = torch.zeros(bank.N, dtype=torch.bool)
    rows[list(truth)] = True
    assert bool(_is_sentinel(bank.tlen)[~rows.to(bank.dev)].all())


@pytest.mark.parametrize('K', [3, 16])
def test_fold_matches_numpy_fold_and_touches_only_its_rows(K):
    # three batches of their own padded length into permuted, non-contiguous rows; row 4 is never folded
    batches = [([8, 2, 5], 7, [1, 7, 2]), ([0, 7], 33, [33, 2]), ([6, 1, 3], 64, [1, 64, 40])]
    bank, truth = _fold_case(9, 64, batches, K, seed=50 + K)
    assert bank.K == K
    _check_fold(bank, truth, K)


def test_fold_long_rows_stride_the_frame_loop():
    bank, truth = _fold_case(3, 1024, [([2, 0], 1000, [1000, 513])], 3, seed=9)
    _check_fold(bank, truth, 3)


def test_fold_refuses_repeated_and_outside_rows():
    from hual_amd import al, lib
    bank = al.McBank(4, 16)
    z = torch.zeros(2, 8, device=bank.dev)
    v = torch.tensor([8, 8], dtype=torch.int32, device=bank.dev)
    with pytest.raises(lib.HualError, match='repeated'):
        bank.fold([1, 1], v, z, z, 0)
    with pytest.raises(lib.HualError, match=r'\[0, 4\)'):
        bank.fold([1, 4], v, z, z, 0)
    with pytest.raises(lib.HualError, match='T_b <= ld'):
        bank.fold([1, 2], v, torch.zeros(2, 17, device=bank.dev), torch.zeros(2, 17, device=bank.dev), 0)
    with pytest.raises(lib.HualError, match='K >= 2'):
        bank.uncert(1, 'range')


def test_range_is_bit_equal_under_a_permutation_of_the_passes():
    batches = [([3, 0, 2], 33, [33, 2, 20])]
    K = 5
    a, _ = _fold_case(4, 64, batches, K, seed=77)
    b, _ = _fold_case(4, 64, batches, K, seed=77, order=[3, 0, 4, 2, 1])
    for bank in (a, b):                      # (row 1 was never folded: give the poisoned row a length of 0 before scoring)
        bank.tlen[1] = 0
    for h in range(2):
        for name in ('lo', 'hi'):
            assert torch.equal(a.stat(h, name)[[3, 0, 2], :33], b.stat(h, name)[[3, 0, 2], :33])
    ua, ub = a.uncert(K, 'range'), b.uncert(K, 'range')
    assert torch.equal(ua[[3, 0, 2], :33], ub[[3, 0, 2], :33]) and float(ua[3, :33].max()) > 0


# ---------------------------------------------------------------------------------------------------------------------
# hual_al_score_mc at K = 2 against hual_al_score on the same two passes' logits
def _bank_of_records(prop):
    """the three logits pairs of classic records folded as k = 0, 1, 2 (rows grouped by their length: a fold is one [B, T_b] batch)"""
    from hual_amd import al
    N = len(prop)
    tlen = np.array([len(p['prop_logits'][0]) for p in prop])
    bank = al.McBank(N, int(tlen.max()))
    for T in np.unique(tlen):
        rows = np.nonzero(tlen == T)[0]
        v = torch.tensor([prop[n]['v_len'] for n in rows], dtype=torch.int32, device=bank.dev)
        for k, key in enumerate(('prop_logits', 'prop_logits1', 'prop_logits2')):
            s = torch.from_numpy(np.stack([prop[n][key][0] for n in rows])).to(bank.dev)
            e = torch.from_numpy(np.stack([prop[n][key][1] for n in rows])).to(bank.dev)
            bank.fold(rows, v, s, e, k)
    return bank


@pytest.mark.parametrize('with_aps', [False, True])
def test_bank_score_at_two_passes_is_hual_al_score(with_aps):
    from hual_amd import al
    from test_gpu_al import _synthetic_round
    N, tmax = 64, 100
    data_old, data_gt, prop = _synthetic_round(N, tmax, 4242, with_aps)
    aps = [([(f, True) for f in r[4]['pos_idx']] + [(f, False) for f in r[4]['neg_idx']]) if with_aps else [] for r in data_old]
    coff = al.get_coff('anet', 1)[6]
    old = al.LabelUpdater(prop, aps)
    old.score(coff)
    bank = _bank_of_records(prop)
    assert bank.K == 2
    vlen = [p['v_len'] for p in prop]
    new = al.LabelUpdater.from_bank(bank, vlen, aps, stat='range')
    assert new.logits is None
    new.score(coff)
    for name in ('uncert_frame', 'uncert_video', 'observe', 'sprob', 'eprob'):
        assert torch.equal(getattr(new, name), getattr(old, name)), name
    assert float(old.uncert_video.min()) > 0
    # STD at K = 2: sqrt(2) * sqrt(d * d / 2) = |d| up to rounding
    std = al.LabelUpdater.from_bank(bank, vlen, aps, stat='std')
    std.score(coff)
    assert float((bank.uncert(2, 'std') - bank.uncert(2, 'range')).abs().max()) <= 1e-6
    assert float((std.uncert_frame - old.uncert_frame).abs().max()) <= 1e-6
    assert float((std.uncert_video - old.uncert_video).abs().max()) <= 1e-6 * tmax          # a sum of at most tmax such terms
    assert torch.equal(std.sprob, old.sprob)


# ---------------------------------------------------------------------------------------------------------------------
# the pipeline: test_gpu_al_round's set
_ROUND = {}


def _round_set():
    if not _ROUND:
        from hual_amd import al, lib
        from hual_amd.dataset import DeviceDataset
        from hual_amd.model import SeqPAN
        N, vdim, max_vlen = 40, 64, 24
        recs, vis, data_gt, data_old = al_synth.make_trainset(N, 12, vdim, max_vlen, seed=3)
        cfg = lib.make_cfg(vdim=vdim, max_vlen=max_vlen, num_words=200, num_chars=30)
        wv = np.random.default_rng(1).normal(0, 0.4, size=(198, 300)).astype(np.float32)
        model = SeqPAN(cfg, wv)
        ds = DeviceDataset(recs, vis)
        s0, e0 = al.labels_from_times(data_old, ds.vlen_h)
        ds.set_labels(s0, e0)
        for r, a, b in zip(recs, s0, e0):
            r['s_ind'], r['e_ind'] = int(a), int(b)
        _ROUND.update(N=N, recs=recs, data_gt=data_gt, data_old=data_old, model=model, ds=ds)
    return _ROUND


def _batches(S, bs=16):
    for lo in range(0, S['N'], bs):
        sel = np.arange(lo, min(S['N'], lo + bs))
        f = S['ds'].assemble(sel, labels=False, min_chars=4)
        yield [S['recs'][i] for i in sel], f['video'], f['video_seq_len'], f['word_ids'], f['char_ids']


def _rng(model):
    st = model.rng_state.cpu().numpy().view(np.uint32)
    return int(st[0]) | (int(st[1]) << 32), int(st[2])


def test_pipeline_two_passes_equals_todays_round():
    from hual_amd import al
    S = _round_set()
    model, N = S['model'], S['N']
    seed, base = _rng(model)
    prop0, ious0 = al.infer_trainset(model, _batches(S), mc_dropout=0.5)
    assert _rng(model) == (seed, base + 2 * 3)
    model.set_rng(seed, base)
    bank = al.McBank.for_dataset(S['ds'])
    propb, iousb = al.infer_trainset(model, _batches(S), mc_dropout=0.5, mc_samples=2, bank=bank)
    assert _rng(model) == (seed, base + 2 * 3)
    assert set(propb[0]) == {'vid', 'duration', 'psuedo_idx', 'sentence', 'v_len', 'prop_idx', 'prop_logits', 'm_score', 'prop_uncert'}
    assert ious0 == iousb
    for a, b in zip(prop0, propb):
        for key in ('vid', 'duration', 'psuedo_idx', 'sentence', 'v_len', 'prop_idx'):
            assert a[key] == b[key]
        for key in ('prop_logits', 'm_score'):
            np.testing.assert_array_equal(np.asarray(a[key]), np.asarray(b[key]))
        assert b['prop_uncert'].dtype == np.float32 and b['prop_uncert'].shape == a['prop_logits'][0].shape
    assert max(float(p['prop_uncert'].max()) for p in propb) > 0              # dropout was on
    coff = al.get_coff('charades', 1)
    new0, d0 = al.update_labels(copy.deepcopy(S['data_old']), S['data_gt'], prop0, coff, return_debug=True)
    newb, db = al.update_labels(copy.deepcopy(S['data_old']), S['data_gt'], propb, coff, return_debug=True, bank=bank)
    assert db['updater'].logits is None
    np.testing.assert_array_equal(db['order'], d0['order'])
    np.testing.assert_array_equal(db['observe'], d0['observe'])
    np.testing.assert_array_equal(db['uncert_video'], d0['uncert_video'])
    np.testing.assert_array_equal(db['uncert_frame'], d0['uncert_frame'])
    np.testing.assert_array_equal(db['new_idx'], d0['new_idx'])
    assert [r[2] for r in newb] == [r[2] for r in new0] and [r[4] for r in newb] == [r[4] for r in new0]
    # and from the records alone (a round resumed from a pickle)
    newr, dr = al.update_labels(copy.deepcopy(S['data_old']), S['data_gt'], propb, coff, return_debug=True)
    np.testing.assert_array_equal(dr['uncert_frame'], d0['uncert_frame'])
    np.testing.assert_array_equal(dr['uncert_video'], d0['uncert_video'])
    assert [r[2] for r in newr] == [r[2] for r in new0]


def _device_probs(s, e, vlen):
    """sigmoid of logits [B, T] as the device computes it, through the existing hual_al_score (its sprob / eprob), zero at t >= v_len"""
    from hual_amd import al
    prop = [{'vid': 'v', 'v_len': int(vlen[b]), 'prop_logits': [s[b], e[b]], 'prop_logits1': [s[b], e[b]], 'prop_logits2': [s[b], e[b]]}
            for b in range(len(s))]
    up = al.LabelUpdater(prop, [[] for _ in prop])
    up.score(0.0)
    mask = np.arange(s.shape[1])[None, :] < np.asarray(vlen)[:, None]
    return np.where(mask, up.sprob.cpu().numpy(), np.float32(0)), np.where(mask, up.eprob.cpu().numpy(), np.float32(0))


def test_pipeline_four_passes_against_individually_fetched_forwards():
    from hual_amd import al
    S = _round_set()
    model, N, K = S['model'], S['N'], 4
    seed, base = _rng(model)
    bank = al.McBank.for_dataset(S['ds'])
    prop, _ = al.infer_trainset(model, _batches(S), mc_dropout=0.5, mc_samples=K, bank=bank, mc_stat='std')
    assert _rng(model) == (seed, base + K * 3) and bank.K == K
    lo, hi = [bank.stat(h, 'lo').cpu().numpy() for h in range(2)], [bank.stat(h, 'hi').cpu().numpy() for h in range(2)]
    um_range = bank.uncert(K, 'range').cpu().numpy()
    for i, (raw, video, lens, word_ids, char_ids) in enumerate(_batches(S)):
        vlen = lens.cpu().numpy()
        ps = []
        for k in range(1, K + 1):
            model.set_rng(seed, base + K * i + k - 1)
            o = model.forward(video, lens, word_ids, char_ids, drop_rate=0.5)
            ps.append(_device_probs(o['start_logits'].cpu().numpy(), o['end_logits'].cpu().numpy(), vlen))
        T = ps[0][0].shape[1]
        rows = np.arange(16 * i, 16 * i + len(raw))
        fs, fe = R.fold_passes([p[0] for p in ps]), R.fold_passes([p[1] for p in ps])
        for h, f in enumerate((fs, fe)):
            np.testing.assert_array_equal(lo[h][rows, :T], f.lo)
            np.testing.assert_array_equal(hi[h][rows, :T], f.hi)
        np.testing.assert_array_equal(um_range[rows, :T], R.uncert(fs, fe, 'range'))
        ref = R.spread64([p[0] for p in ps]) + R.spread64([p[1] for p in ps])
        for b, n in enumerate(rows):
            assert prop[n]['prop_uncert'].shape == (T,)
            assert np.abs(prop[n]['prop_uncert'] - ref[b]).max() <= 1e-6
    assert float(um_range.max()) > 0
    model.set_rng(seed, base + K * 3)
    # the records alone give the score the bank gives
    aps = [[] for _ in range(N)]
    a = al.LabelUpdater.from_bank(bank, [p['v_len'] for p in prop], aps, stat='std')
    b = al.LabelUpdater(prop, aps)
    assert b.logits is None
    for up in (a, b):
        up.score(0.25)
    for name in ('uncert_frame', 'uncert_video', 'observe', 'sprob', 'eprob'):
        assert torch.equal(getattr(a, name), getattr(b, name)), name


def test_run_round_with_four_passes():
    from hual_amd import al
    S = _round_set()
    model = S['model']
    bank = al.McBank.for_dataset(S['ds'])
    prop, _ = al.infer_trainset(model, _batches(S), mc_dropout=0.5, mc_samples=4, bank=bank)
    p_before = model.params.clone()
    new_data, prop1, m = al.run_round(model, S['ds'], copy.deepcopy(S['data_old']), S['data_gt'], prop, 'charades', 1, epochs=1,
                                      batch_size=16, lr=1e-3, drop_rate=0.2, mc_samples=4, bank=bank)
    assert m['mc_bank'] is bank and bank.K == 4
    assert len(prop1) == S['N'] and all('prop_uncert' in r and 'prop_logits1' not in r and 'prop_logits2' not in r for r in prop1)
    assert all(r['prop_uncert'].shape == r['prop_logits'][0].shape for r in prop1)
    assert float((model.params - p_before).abs().max()) > 0 and torch.isfinite(model.params).all()
    # the renewed labels are those of the records' own recorded term (the bank held the same passes)
    ref = al.update_labels(copy.deepcopy(S['data_old']), S['data_gt'], prop, al.get_coff('charades', 1))
    assert [r[2] for r in new_data] == [r[2] for r in ref] and [r[4] for r in new_data] == [r[4] for r in ref]


# ---------------------------------------------------------------------------------------------------------------------
# two ranks on one GPU over gloo (as test_gpu_dp_epoch.py launches them)
def _sharded_run(world):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from hual_amd import al, lib
    from hual_amd.dataset import DeviceDataset
    from hual_amd.model import SeqPAN
    recs, vis, data_gt, data_old = al_synth.make_trainset(40, 10, 64, 24, seed=8)
    cfg = lib.make_cfg(vdim=64, max_vlen=24, num_words=200, num_chars=30)
    wv = np.random.default_rng(1).normal(0, 0.4, size=(198, 300)).astype(np.float32)
    ds = DeviceDataset(recs, vis)
    s0, e0 = al.labels_from_times(data_old, ds.vlen_h)
    ds.set_labels(s0, e0)
    for r, a, b in zip(recs, s0, e0):
        r['s_ind'], r['e_ind'] = int(a), int(b)
    m = SeqPAN(cfg, wv)
    bank = al.McBank.for_dataset(ds)
    rng0 = m.rng_state.cpu().numpy().copy()
    out_r, ious = al.infer_trainset_sharded(m, ds, 6, mc_dropout=0.5, mc_samples=3, bank=bank, mc_stat='std')
    torch.cuda.synchronize()
    out = None
    if out_r is not None:
        out = dict(idx=np.array([r['prop_idx'] for r in out_r]), vids=[r['vid'] for r in out_r], ious=np.array(ious),
                   l0=[np.stack(r['prop_logits']) for r in out_r], um=[r['prop_uncert'] for r in out_r],
                   keys=sorted(out_r[0]), tlen=bank.tlen.cpu().numpy(), s0=bank.s0.cpu().numpy(), e0=bank.e0.cpu().numpy(),
                   stats=bank.stats.cpu().numpy(), K=bank.K)
    return out, rng0, m.rng_state.cpu().numpy().copy()


def _sharded_worker(rank, world, port, q):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    q.put((rank, _sharded_run(world)))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_gather_the_single_process_bank():
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 29780 + (os.getpid() % 100)
    procs = [ctx.Process(target=_sharded_worker, args=(r, 2, port, q)) for r in range(2)]
    for pr in procs:
        pr.start()
    got = dict(q.get(timeout=600) for _ in range(2))
    for pr in procs:
        pr.join(timeout=120)
        assert pr.exitcode == 0
    o1, rng_a, rng_b = _sharded_run(1)
    o0 = got[0][0]
    assert got[1][0] is None
    assert o0['keys'] == o1['keys'] and 'prop_uncert' in o0['keys'] and 'prop_logits1' not in o0['keys']
    assert o0['vids'] == o1['vids'] and o0['K'] == o1['K'] == 3
    for k in ('idx', 'ious', 'tlen', 's0', 'e0', 'stats'):
        np.testing.assert_array_equal(o0[k], o1[k])
    for k in ('l0', 'um'):
        for a, b in zip(o0[k], o1[k]):
            np.testing.assert_array_equal(a, b)
    assert max(float(u.max()) for u in o0['um']) > 0
    n_batches = (40 + 5) // 6
    for r in range(2):
        before, after = got[r][1].view(np.uint32), got[r][2].view(np.uint32)
        assert int(after[2]) - int(before[2]) == 3 * n_batches and (after[:2] == before[:2]).all()
    assert int(rng_b.view(np.uint32)[2]) - int(rng_a.view(np.uint32)[2]) == 3 * n_batches
