"""GPU: information-theoretic acquisition from the K-pass bank - hual_al_mc_fold_info against hual_al_mc_fold (bit for bit) and against the
float64 fold of tests/mc_info_ref.py, hual_al_score_info against hual_al_score_mc and a float64 restatement, the rows' round trip, and
the infer_trainset / update_labels path with mc_stat='bald'.

The bar against the float64 reference is an absolute 2e-5, derived and not tuned: with |logit| <= 8 the log-odds |log2((1-p)/p)| are at most
11.6 bits, so a 2-ulp difference in p between the device's 1/(1+expf(-x)) and torch.sigmoid moves h2 by at most about 1.4e-6; log2f at a
few ulp on terms of at most 0.53 adds about 1e-7 per term, the running mean over K <= 5 about K * 2^-24; two heads and one subtraction
stay under 1e-5, and the bar is twice that.  Each comparison prints its figure before it asserts."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import al_synth
import mc_info_ref as R

pytestmark = pytest.mark.gpu
TOL = 2e-5
SENTINEL = 0x7fc0dead       # (as int32 bits) a NaN payload no arithmetic produces
BANK_ARRAYS = ('tlen', 's0', 'e0', 'stats')


def _poison(bank):
    for t in (bank.s0, bank.e0, bank.stats, bank.tlen) + ((bank.ent,) if bank.ent is not None else ()):
        t.view(torch.int32).fill_(SENTINEL)


def _bits(t):
    return t.cpu().view(torch.int32).numpy()


def _logits(g, shape):
    """N(0, 2) clipped to |x| <= 8"""
    return np.clip(g.standard_normal(shape) * 2.0, -8.0, 8.0).astype(np.float32)


def _fold(bank, rows, vl, det, ps):
    """det [B, 2, T] as k = 0, ps [K, B, 2, T] as k = 1..K into the rows `rows`"""
    dev = bank.dev
    v = torch.tensor(vl, dtype=torch.int32, device=dev)
    for k, x in enumerate([det] + list(ps)):
        bank.fold(np.asarray(rows), v, torch.from_numpy(x[:, 0].copy()).to(dev), torch.from_numpy(x[:, 1].copy()).to(dev), k)


def _reference(ps, vl):
    """per row b: (InfoFold of the start head, of the end head) over the K passes ps [K, B, 2, T]"""
    return [tuple(R.fold_passes([R.probs(ps[k, b, h], vl[b]) for k in range(ps.shape[0])]) for h in range(2)) for b in range(ps.shape[1])]


def _stats(bank, K):
    return {s: bank.uncert(K, s).cpu().numpy() for s in R.STATS}


_CASES = {}


def _case(T, K, N=5, ld=70, rows=(4, 0, 2)):
    """B = 3 rows of one [B, T] fold each pass, v_len in {1, T - 1, T}: the same seeded logits through hual_al_mc_fold into a plain bank
    and through hual_al_mc_fold_info into an info bank, both poisoned first.  Computed once per (T, K) and left unchanged."""
    key = (T, K, N, ld)
    if key not in _CASES:
        from hual_amd import al
        g = np.random.default_rng(1000 * T + K)
        rows = list(rows)
        vl = [1, T - 1, T][:len(rows)]
        det, ps = _logits(g, (len(rows), 2, T)), _logits(g, (K, len(rows), 2, T))
        plain, info = al.McBank(N, ld), al.McBank(N, ld, info=True)
        for bank in (plain, info):
            _poison(bank)
            _fold(bank, rows, vl, det, ps)
        torch.cuda.synchronize()
        assert plain.K == info.K == K
        raw = {name: (_bits(getattr(plain, name)), _bits(getattr(info, name))) for name in BANK_ARRAYS}
        raw['ent'] = _bits(info.ent)
        unfolded = [n for n in range(N) if n not in rows]
        info.tlen[unfolded] = 0                       # (a poisoned length is no length: scoring reads tlen)
        _CASES[key] = dict(T=T, K=K, N=N, ld=ld, rows=rows, unfolded=unfolded, vl=vl, det=det, ps=ps, raw=raw, bank=info,
                           ent=info.ent.cpu().numpy(), stats=_stats(info, K), ref=_reference(ps, vl))
    return _CASES[key]


SHAPES = [(T, K) for T in (2, 33, 70) for K in (2, 5)]


# ---------------------------------------------------------------------------------------------------------------------
# 1. the same bank as hual_al_mc_fold leaves, bit for bit
@pytest.mark.parametrize('T,K', SHAPES)
def test_info_fold_leaves_the_bank_of_the_plain_fold(T, K):
    c = _case(T, K)
    for name in BANK_ARRAYS:
        a, b = c['raw'][name]
        np.testing.assert_array_equal(a, b, err_msg=name)
    tlen, stats = c['raw']['tlen'][1], c['raw']['stats'][1]
    assert (tlen[c['rows']] == T).all() and (tlen[c['unfolded']] == SENTINEL).all()
    assert (stats[:, :, c['rows'], :T] != SENTINEL).all()                 # (and the comparison above was not one of sentinels)
    # ent: columns [0, T) of the listed rows are written, nothing else
    ent = c['raw']['ent']
    touched = np.zeros((c['N'], c['ld']), dtype=bool)
    touched[c['rows'], :T] = True
    for h in range(2):
        assert (ent[h][~touched] == SENTINEL).all(), 'the info fold wrote ent outside its rows'
        assert (ent[h][touched] != SENTINEL).all()


# ---------------------------------------------------------------------------------------------------------------------
# 2. ent and the three statistics against the float64 reference
def _check_against_reference(c):
    T, K = c['T'], c['K']
    worst = {}
    for b, n in enumerate(c['rows']):
        fs, fe = c['ref'][b]
        for h, f in enumerate((fs, fe)):
            worst['ent'] = max(worst.get('ent', 0.0), float(np.abs(c['ent'][h, n, :T] - f.ent).max()))
        for s in R.STATS:
            worst[s] = max(worst.get(s, 0.0), float(np.abs(c['stats'][s][n, :T] - R.uncert(fs, fe, s)).max()))
    print('T_b=%d K=%d max |device - float64 reference|: %s' % (T, K, ', '.join('%s %.3g' % kv for kv in sorted(worst.items()))))
    for name, d in worst.items():
        assert d <= TOL, (name, d)
    assert max(float(c['stats'][s].max()) for s in R.STATS) > 0.1


@pytest.mark.parametrize('T,K', SHAPES)
def test_ent_and_statistics_match_the_float64_reference(T, K):
    _check_against_reference(_case(T, K))


# ---------------------------------------------------------------------------------------------------------------------
# 3. exact properties on the device
@pytest.mark.parametrize('T,K', SHAPES)
def test_masked_frames_and_columns_beyond_tlen_are_zero(T, K):
    c = _case(T, K)
    for s in R.STATS:
        um = c['stats'][s]
        for b, n in enumerate(c['rows']):
            assert (um[n, c['vl'][b]:] == 0).all(), (s, n)                # t >= v_len, and beyond tlen = T
            assert np.isfinite(um[n]).all() and um[n].min() >= 0 and um[n].max() <= 2.0 + 1e-6
        assert (um[c['unfolded']] == 0).all()
    for h in range(2):
        for b, n in enumerate(c['rows']):
            assert (c['ent'][h, n, c['vl'][b]:T] == 0).all()


def test_identical_passes_have_exactly_zero_bald():
    from hual_amd import al
    g = np.random.default_rng(31)
    N, ld, T, K = 3, 70, 70, 5
    det, one = _logits(g, (N, 2, T)), _logits(g, (N, 2, T))
    bank = al.McBank(N, ld, info=True)
    _fold(bank, [2, 0, 1], [1, T - 1, T], det, [one] * K)
    st = _stats(bank, K)
    assert (st['bald'] == 0).all()                    # Welford leaves mean == p, the running mean leaves ent == h2(p): the same h2 of the same float
    np.testing.assert_array_equal(st['entropy'], st['expected_entropy'])
    assert st['entropy'].max() > 1.0                   # while every pass is unsure
    for h in range(2):
        assert torch.equal(bank.stat(h, 'mean'), bank.stat(h, 'lo')) and float(bank.stat(h, 'm2').abs().max()) == 0.0


def test_saturated_logits_give_finite_values_in_range():
    from hual_amd import al
    g = np.random.default_rng(32)
    N, ld, T, K = 3, 70, 33, 3
    sign = np.where(g.random((K, N, 2, T)) < 0.5, -1.0, 1.0).astype(np.float32)
    ps = sign * np.float32(40.0)
    ps[:, 2] = sign[:, 2] * np.float32(np.inf)         # a row of +-inf
    bank = al.McBank(N, ld, info=True)
    _fold(bank, [0, 1, 2], [T, T - 1, T], np.zeros((N, 2, T), np.float32), ps)
    ent = bank.ent.cpu().numpy()
    assert np.isfinite(ent).all() and ent.min() >= 0 and ent.max() <= 1.0
    for s, um in _stats(bank, K).items():
        assert np.isfinite(um).all() and um.min() >= 0 and um.max() <= 2.0, s
    st = _stats(bank, K)
    assert st['bald'].max() > 1.0                      # passes of p = 0 and p = 1 disagree as much as passes can
    assert st['expected_entropy'].max() <= 1e-12       # and none of them is unsure


# ---------------------------------------------------------------------------------------------------------------------
# 4. long rows stride the frame loop
def test_long_rows_stride_the_frame_loop():
    c = _case(1000, 3, N=3, ld=1024, rows=(2, 0))
    for name in BANK_ARRAYS:
        a, b = c['raw'][name]
        np.testing.assert_array_equal(a, b, err_msg=name)
    assert c['vl'] == [1, 999]
    _check_against_reference(c)
    for s in R.STATS:
        assert (c['stats'][s][:, 1000:] == 0).all() and (c['stats'][s][2, 1:] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# 5. the score path
def _bank_of_records(prop, passes=('prop_logits1', 'prop_logits2'), info=True):
    """classic records folded as k = 0, 1, 2 (rows grouped by their length: a fold is one [B, T_b] batch)"""
    from hual_amd import al
    tlen = np.array([len(p['prop_logits'][0]) for p in prop])
    bank = al.McBank(len(prop), int(tlen.max()), info=info)
    for T in np.unique(tlen):
        rows = np.nonzero(tlen == T)[0]
        v = torch.tensor([prop[n]['v_len'] for n in rows], dtype=torch.int32, device=bank.dev)
        for k, key in enumerate(('prop_logits',) + tuple(passes)):
            s = torch.from_numpy(np.stack([prop[n][key][0] for n in rows])).to(bank.dev)
            e = torch.from_numpy(np.stack([prop[n][key][1] for n in rows])).to(bank.dev)
            bank.fold(rows, v, s, e, k)
    return bank


def _score_set(with_aps, N=48, tmax=100, seed=4242):
    from test_gpu_al import _synthetic_round
    data_old, data_gt, prop = _synthetic_round(N, tmax, seed, with_aps)
    aps = [([(f, True) for f in r[4]['pos_idx']] + [(f, False) for f in r[4]['neg_idx']]) if with_aps else [] for r in data_old]
    return prop, aps, [p['v_len'] for p in prop]


OUTPUTS = ('sprob', 'eprob', 'uncert_frame', 'uncert_video', 'observe')


@pytest.mark.parametrize('with_aps', [False, True])
def test_score_info_without_the_uncertainty_term_is_score_mc(with_aps):
    """coff_uncert = 0 leaves the distance score alone in uncert_frame: sprob, eprob, uncert_frame and observe_point are hual_al_score_mc's
    bit for bit whatever the statistic.  uncert_video is the row sum of the term itself, so it can only be compared where the two terms
    coincide - which they do, at non-zero values, for passes of p = 0 and p = 1 (logits -+100): per head RANGE and BALD (and ENTROPY) are
    both exactly 1 where the two passes differ and exactly 0 where they agree.  On that set all five outputs are compared."""
    from hual_amd import al
    prop, aps, vlen = _score_set(with_aps)
    g = np.random.default_rng(5)
    for p in prop:
        for key in ('prop_logits1', 'prop_logits2'):
            p[key] = [np.where(g.random(len(x)) < 0.5, np.float32(-100), np.float32(100)).astype(np.float32) for x in p['prop_logits']]
    bank = _bank_of_records(prop)
    mc = al.LabelUpdater.from_bank(bank, vlen, aps, stat='range')
    mc.score(0.0)
    assert float(mc.uncert_video.min()) > 0
    for stat in ('bald', 'entropy'):
        up = al.LabelUpdater.from_bank(bank, vlen, aps, stat=stat)
        up.score(0.0)
        for name in OUTPUTS:
            assert torch.equal(getattr(up, name), getattr(mc, name)), (stat, name)
    # and on passes that are not saturated: everything but the sum of the (different) term
    prop, aps, vlen = _score_set(with_aps)
    bank = _bank_of_records(prop)
    mc = al.LabelUpdater.from_bank(bank, vlen, aps, stat='range')
    mc.score(0.0)
    for stat in R.STATS:
        up = al.LabelUpdater.from_bank(bank, vlen, aps, stat=stat)
        up.score(0.0)
        for name in ('sprob', 'eprob', 'uncert_frame', 'observe'):
            assert torch.equal(getattr(up, name), getattr(mc, name)), (stat, name)
        assert float(up.uncert_video.min()) > 0


@pytest.mark.parametrize('with_aps', [False, True])
def test_score_info_mixture_is_its_float64_restatement(with_aps):
    """uncert_frame = (double)dist + (double)(um * coff_uncert) with um the kernel's own uncert_model output, dist the coff_uncert = 0
    result; uncert_video the sum of um; observe_point the first maximal frame"""
    from hual_amd import al, lib
    prop, aps, vlen = _score_set(with_aps)
    bank = _bank_of_records(prop)
    tlen = bank.tlen.cpu().numpy()
    for stat in R.STATS:
        base = al.LabelUpdater.from_bank(bank, vlen, aps, stat=stat)
        base.score(0.0)
        dist = base.uncert_frame.cpu().numpy()
        up = al.LabelUpdater.from_bank(bank, vlen, aps, stat=stat)
        um_d = torch.full((bank.N, bank.ld), float('nan'), device=bank.dev)
        p = lib.ptr
        lib.check(up._lib.hual_al_score_info(ctypes.byref(up.set), p(bank.s0), p(bank.e0), ctypes.byref(bank.c), ctypes.byref(bank.info_c),
                                             bank.K, lib.AL_STAT_INFO[stat], 0.25, p(up.sprob), p(up.eprob), p(up.uncert_frame),
                                             p(up.uncert_video), p(up.observe), p(um_d), lib.stream_ptr()))
        torch.cuda.synchronize()
        um, uf, uv, ob = um_d.cpu().numpy(), up.uncert_frame.cpu().numpy(), up.uncert_video.cpu().numpy(), up.observe.cpu().numpy()
        viaup = al.LabelUpdater.from_bank(bank, vlen, aps, stat=stat)          # LabelUpdater.score() is that launch
        viaup.score(0.25)
        for name in OUTPUTS:
            assert torch.equal(getattr(viaup, name), getattr(up, name)), (stat, name)
        np.testing.assert_array_equal(um[np.arange(bank.ld)[None, :] < tlen[:, None]], bank.uncert(bank.K, stat).cpu().numpy()[
            np.arange(bank.ld)[None, :] < tlen[:, None]])
        for n in range(bank.N):
            T, V = int(tlen[n]), vlen[n]
            assert np.isnan(um[n, T:]).all() and (um[n, V:T] == 0).all()      # written for [0, tlen) only; 0 at t >= v_len
            want = dist[n, :T] + (um[n, :T] * np.float32(0.25)).astype(np.float32).astype(np.float64)
            np.testing.assert_array_equal(uf[n, :T], want)
            assert ob[n] == int(np.argmax(want))
            assert abs(float(uv[n]) - float(um[n, :T].astype(np.float64).sum())) <= 1e-6 * max(1.0, float(uv[n]))
        assert float(um[np.isfinite(um)].max()) > 0.05


# ---------------------------------------------------------------------------------------------------------------------
# 6. rows as host arrays and back
def test_rows_round_trip_with_ent():
    from hual_amd import al, lib
    c = _case(33, 5)
    src = c['bank']
    part = src.export_rows(np.array(c['rows']))
    assert part['ent'].shape == (2, 3, c['ld'])
    dst = al.McBank(c['N'], c['ld'], info=True)
    dst.import_rows(part)
    assert dst.K == 5
    for h in range(2):
        np.testing.assert_array_equal(_bits(dst.stat(h, 'ent'))[c['rows'], :33], _bits(src.stat(h, 'ent'))[c['rows'], :33])
        assert float(dst.stat(h, 'ent')[c['unfolded']].abs().max()) == 0.0
    for s, um in _stats(dst, 5).items():
        np.testing.assert_array_equal(um[c['rows']], c['stats'][s][c['rows']], err_msg=s)
    plain = al.McBank(c['N'], c['ld'])
    with pytest.raises(lib.HualError, match='info='):
        plain.import_rows(part)
    with pytest.raises(lib.HualError, match='info='):
        dst.import_rows(plain.export_rows(np.array([0])))
    with pytest.raises(lib.HualError, match='info=True'):
        plain.uncert(2, 'bald')
    with pytest.raises(lib.HualError, match='info=True'):
        plain.stat(0, 'ent')


# ---------------------------------------------------------------------------------------------------------------------
# 7. through the model: a set of the c1 shape (T 64, V 1024), 12 samples at batch 4
_MODEL = {}


def _model_set():
    if not _MODEL:
        from hual_amd import al, lib
        from hual_amd.dataset import DeviceDataset
        from hual_amd.model import SeqPAN
        N, vdim, max_vlen = 12, 1024, 64
        recs, vis, data_gt, data_old = al_synth.make_trainset(N, 5, vdim, max_vlen, seed=21)
        cfg = lib.make_cfg(vdim=vdim, max_vlen=max_vlen, num_words=200, num_chars=30)
        wv = np.random.default_rng(1).normal(0, 0.4, size=(198, 300)).astype(np.float32)
        model = SeqPAN(cfg, wv)
        ds = DeviceDataset(recs, vis)
        s0, e0 = al.labels_from_times(data_old, ds.vlen_h)
        ds.set_labels(s0, e0)
        for r, a, b in zip(recs, s0, e0):
            r['s_ind'], r['e_ind'] = int(a), int(b)
        _MODEL.update(N=N, recs=recs, data_gt=data_gt, data_old=data_old, model=model, ds=ds)
    return _MODEL


def _batches(S, bs=4):
    for lo in range(0, S['N'], bs):
        sel = np.arange(lo, min(S['N'], lo + bs))
        f = S['ds'].assemble(sel, labels=False, min_chars=4)
        yield [S['recs'][i] for i in sel], f['video'], f['video_seq_len'], f['word_ids'], f['char_ids']


def _rng(model):
    st = model.rng_state.cpu().numpy().view(np.uint32)
    return int(st[0]) | (int(st[1]) << 32), int(st[2])


def test_pipeline_with_bald():
    from hual_amd import al, lib
    S = _model_set()
    model, K = S['model'], 4
    seed, base = _rng(model)
    # a run that never heard of the option ...
    plain = al.McBank.for_dataset(S['ds'])
    prop0, ious0 = al.infer_trainset(model, _batches(S), mc_dropout=0.5, mc_samples=K, bank=plain)
    # ... the same seeds with mc_stat='range' into a bank that folds the entropy too ...
    model.set_rng(seed, base)
    bank = al.McBank.for_dataset(S['ds'], info=True)
    prop1, ious1 = al.infer_trainset(model, _batches(S), mc_dropout=0.5, mc_samples=K, bank=bank, mc_stat='range')
    assert ious0 == ious1 and set(prop0[0]) == set(prop1[0])
    for a, b in zip(prop0, prop1):
        for key in ('vid', 'duration', 'psuedo_idx', 'sentence', 'v_len', 'prop_idx'):
            assert a[key] == b[key]
        for key in ('prop_logits', 'm_score', 'prop_uncert'):
            np.testing.assert_array_equal(np.asarray(a[key]), np.asarray(b[key]))
    for name in BANK_ARRAYS:
        assert torch.equal(getattr(plain, name), getattr(bank, name)), name
    assert max(float(p['prop_uncert'].max()) for p in prop0) > 0              # dropout was on
    # ... and with mc_stat='bald'
    model.set_rng(seed, base)
    with pytest.raises(lib.HualError, match='info=True'):
        al.infer_trainset(model, _batches(S), mc_dropout=0.5, mc_samples=K, bank=plain, mc_stat='bald')
    assert _rng(model) == (seed, base)                                        # refused before any forward
    propb, iousb = al.infer_trainset(model, _batches(S), mc_dropout=0.5, mc_samples=K, bank=bank, mc_stat='bald')
    assert _rng(model) == (seed, base + K * 3) and bank.K == K and iousb == ious0
    assert set(propb[0]) == set(prop0[0]) and 'prop_uncert' in propb[0] and 'prop_logits1' not in propb[0]
    um = bank.uncert(K, 'bald').cpu().numpy()
    tl = bank.tlen.cpu().numpy()
    for n, r in enumerate(propb):
        assert r['prop_uncert'].dtype == np.float32
        np.testing.assert_array_equal(r['prop_uncert'], um[n, :tl[n]])
        np.testing.assert_array_equal(np.asarray(r['prop_logits']), np.asarray(prop0[n]['prop_logits']))
    assert 0 < um.max() <= 2.0
    # the label update from the bank, and from the records alone (the resume path replays the recorded term, whichever statistic it is)
    coff = al.get_coff('charades', 1)
    newb, db = al.update_labels(copy.deepcopy(S['data_old']), S['data_gt'], propb, coff, return_debug=True, bank=bank, mc_stat='bald')
    assert db['updater'].stat == 'bald' and db['updater'].logits is None
    newr, dr = al.update_labels(copy.deepcopy(S['data_old']), S['data_gt'], propb, coff, return_debug=True)
    assert dr['updater'].stat == 'range' and dr['updater'].bank is None
    for key in ('order', 'observe', 'uncert_video', 'uncert_frame', 'new_idx', 'sprob', 'eprob'):
        np.testing.assert_array_equal(db[key], dr[key], err_msg=key)
    assert [r[2] for r in newb] == [r[2] for r in newr] and [r[4] for r in newb] == [r[4] for r in newr]
    assert float(db['uncert_video'].min()) > 0
    # a bank of this call only gets the entropy arrays when the statistic needs them
    model.set_rng(seed, base)
    recs_s, _ = al.infer_trainset_sharded(model, S['ds'], 4, mc_dropout=0.5, mc_samples=K, mc_stat='bald')
    for a, b in zip(recs_s, propb):
        np.testing.assert_array_equal(a['prop_uncert'], b['prop_uncert'])
