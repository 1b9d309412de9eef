"""GPU: hual_al_grad_embed against the float64 statement of its contract (tests/grad_embed_ref.py, which also works out the bars),
against the model's own backward, and the places it lands: al.GradBank and al.infer_trainset(grad_bank=).

The bars, u = 2^-24 (grad_embed_ref's docstring derives them; not tuned):
  desc     per column: (T + 8) u sum_t (p(t) + y(t)) |h(t, c)|
  gnorm2   that bound through the squares, plus 2 u of the value
  egl      that bound through d = h - mu and p d^2, plus 10 u of the value
  model    the project's gradient contract: 1e-3 of the tensor's own largest magnitude."""
import copy
import math

import numpy as np
import pytest
import torch

import al_synth
import grad_embed_ref as GR
import parity_util as pu
from span_clip_util import _pads_intact, _sentinel, _task, _videos

pytestmark = pytest.mark.gpu

FILL = 777.0
B = 6


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def make_case(T, ld, seed):
    """six clips: v_len 1 (where T allows the others to differ), full, in between, one v < 1 and one with an inf logit inside v;
    hypotheses inside, at both edges and outside [0, v); NaN in the logits' padding columns; rows: a permutation of bank rows with one
    foreign id"""
    g = np.random.default_rng(seed)
    hs = g.standard_normal((B * T, GR.H)).astype(np.float32)
    he = (2.0 * g.standard_normal((B * T, GR.H))).astype(np.float32)
    zs = np.full((B, ld), np.nan, dtype=np.float32)
    ze = np.full((B, ld), np.nan, dtype=np.float32)
    zs[:, :T] = (3.0 * g.standard_normal((B, T))).astype(np.float32)
    ze[:, :T] = (3.0 * g.standard_normal((B, T))).astype(np.float32)
    mid = max(1, (T + 1) // 2)
    v_len = np.array([1, T, mid, 0, T, T + 5], dtype=np.int32)            # (T + 5 reads as T)
    zs[4, T - 1] = np.inf                                                  # inside v
    hyp = np.array([[0, 0], [0, T - 1], [mid - 1, mid], [0, 0], [0, 0], [-1, T // 2]], dtype=np.int32)
    N = 9
    rows = np.array([7, 2, 0, 5, 3, N], dtype=np.int32)                    # sample 5 names a foreign row: nothing is written
    rows[[4, 5]] = rows[[5, 4]] if T % 2 else rows[[4, 5]]                 # the foreign id on the inf row for odd T, on a clean row otherwise
    return dict(hs=hs, he=he, zs=zs, ze=ze, v_len=v_len, hyp=hyp, rows=rows, N=N, T=T, ld=ld)


def launch(dev, c, ld_desc=256, rows=True):
    """one launch into sentinel-filled, padded banks -> (desc, gnorm2, egl) numpy, after checking the memory around them"""
    from hual_amd import lib
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    zs_whole, ze_whole = t(c['zs']), t(c['ze'])
    desc_v, desc_w, desc_p = _sentinel((c['N'], ld_desc), torch.float32, dev, FILL)
    gn_v, gn_w, gn_p = _sentinel((c['N'],), torch.float32, dev, FILL)
    eg_v, eg_w, eg_p = _sentinel((c['N'],), torch.float32, dev, FILL)
    got = lib.al_grad_embed(t(c['hs']), t(c['he']), zs_whole, ze_whole, t(c['v_len']), t(c['hyp']), desc_v, gn_v, eg_v,
                            rows=t(c['rows']) if rows else None)
    torch.cuda.synchronize()
    assert got[0] is desc_v and got[1] is gn_v and got[2] is eg_v
    assert _pads_intact(desc_w, desc_p, FILL) and _pads_intact(gn_w, gn_p, FILL) and _pads_intact(eg_w, eg_p, FILL)
    return desc_v.cpu().numpy(), gn_v.cpu().numpy(), eg_v.cpu().numpy()


@pytest.mark.parametrize('T', [1, 2, 33, 70, 256])
@pytest.mark.parametrize('pad', [0, 7])
def test_values_against_float64(dev, T, pad):
    c = make_case(T, T + pad, seed=100 * T + pad)
    ref = GR.embed(c['hs'], c['he'], c['zs'], c['ze'], c['v_len'], c['hyp'], T)
    assert ref['poisoned'].tolist() == [False, False, False, True, True, False]
    ld_desc = 256 if pad == 0 else 261                                     # a bank with wider rows: columns 256.. stay intact
    desc, gn, eg = launch(dev, c, ld_desc=ld_desc)
    written = np.zeros(c['N'], dtype=bool)
    worst = dict(desc=0.0, gnorm2=0.0, egl=0.0)
    for b, row in enumerate(c['rows'].tolist()):
        if not 0 <= row < c['N']:
            continue
        written[row] = True
        assert (desc[row, 256:] == FILL).all()
        if ref['poisoned'][b]:
            assert np.isnan(desc[row, :256]).all() and gn[row] == -1.0 and eg[row] == -1.0, (T, pad, b)
            continue
        err = np.abs(desc[row, :256].astype(np.float64) - ref['desc'][b])
        ratios = dict(desc=float((err / np.maximum(ref['desc_bar'][b], 1e-300)).max()),
                      gnorm2=abs(float(gn[row]) - ref['gnorm2'][b]) / max(ref['gnorm2_bar'][b], 1e-300),
                      egl=abs(float(eg[row]) - ref['egl'][b]) / max(ref['egl_bar'][b], 1e-300))
        if ref['egl'][b] == 0.0:                                           # one frame: h - mu is an exact zero
            assert eg[row] == 0.0
            ratios['egl'] = 0.0
        print('T %d ld %d sample %d (v %d): error / bar desc %.3f gnorm2 %.3f egl %.3f' % (T, T + pad, b, min(int(c['v_len'][b]), T), ratios['desc'],
                                                                                   ratios['gnorm2'], ratios['egl']))
        for k, r in ratios.items():
            worst[k] = max(worst[k], r)
            assert r <= 1.0, (T, pad, b, k, r)
    assert (desc[~written] == FILL).all() and (gn[~written] == FILL).all() and (eg[~written] == FILL).all()
    assert written.sum() == 5
    print('T %d ld %d: largest error / bar desc %.3f gnorm2 %.3f egl %.3f' % (T, T + pad, worst['desc'], worst['gnorm2'], worst['egl']))


def test_no_hypothesis_gives_the_expected_feature_and_rows_default_to_the_batch(dev):
    c = make_case(33, 33, seed=5)
    c['hyp'][:] = [[-1, 33]] * B
    desc, gn, eg = launch(dev, c, rows=False)
    ref = GR.embed(c['hs'], c['he'], c['zs'], c['ze'], c['v_len'], c['hyp'], 33)
    for b in (0, 1, 2, 5):
        assert (np.abs(desc[b].astype(np.float64) - ref['desc'][b]) <= ref['desc_bar'][b]).all()
    assert np.isnan(desc[3]).all() and np.isnan(desc[4]).all() and (desc[B:] == FILL).all()
    with_hyp = make_case(33, 33, seed=5)
    _, _, eg2 = launch(dev, with_hyp, rows=False)
    assert same_bits(eg[:B], eg2[:B])                                      # egl does not depend on the hypothesis


def test_second_launch_and_graph_replay_return_equal_bits(dev):
    from hual_amd import lib
    c = make_case(70, 77, seed=9)
    want = launch(dev, c)
    again = launch(dev, c)
    assert all(same_bits(a, w) for a, w in zip(again, want))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    args = [t(c[k]) for k in ('hs', 'he', 'zs', 'ze', 'v_len', 'hyp')]
    rows = t(c['rows'])
    banks = (torch.full((c['N'], 256), FILL, device=dev), torch.full((c['N'],), FILL, device=dev), torch.full((c['N'],), FILL, device=dev))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        lib.al_grad_embed(*args, *banks, rows=rows)                        # (warm-up)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        lib.al_grad_embed(*args, *banks, rows=rows)
    for _ in range(2):
        for o in banks:
            o.fill_(FILL)
        graph.replay()
        torch.cuda.synchronize()
        for o, w in zip(banks, want):
            assert same_bits(o.cpu().numpy(), w)


def test_it_is_the_models_gradient(dev):
    """forward(labels=) with y1 / y2 one-hot at the predicted span, backward(): with B = 1 the loss's gradient with respect to the
    start_dense / end_dense kernels is g_s / g_e of the launch on the same forward's taps"""
    from hual_amd import al, data
    cfg, p, wv, b, _ = pu.make_case(B=1, T=12, L=4, C=4, seed=5)
    m = pu.hip_model(cfg, p, wv)
    T = 12
    lens = b['lens']
    o = m.forward(b['video'], lens, b['word_ids'], b['char_ids'])
    si, ei = int(o['start_index'][0]), int(o['end_index'][0])
    _, _, ml, il = data.make_labels(np.array([si]), np.array([ei]), lens.numpy(), max_len=T)      # (the reference's y1 / y2 are soft)
    y1, y2 = np.zeros((1, T), dtype=np.float32), np.zeros((1, T), dtype=np.float32)
    y1[0, si] = y2[0, ei] = 1.0
    labels = (torch.tensor(y1), torch.tensor(y2), torch.tensor(ml), torch.tensor(il, dtype=torch.float32))
    o = m.forward(b['video'], lens, b['word_ids'], b['char_ids'], labels=labels)
    bank = al.GradBank(1, device=dev)
    hyp = torch.tensor([[si, ei]], dtype=torch.int32, device=dev)
    bank.embed(m, o, lens.to(device=dev, dtype=torch.int32), None, hyp)
    desc = bank.desc.cpu().numpy()[0]
    ref = GR.embed(m.tap('head.hs').cpu().numpy(), m.tap('head.he').cpu().numpy(), o['start_logits'].cpu().numpy(), o['end_logits'].cpu().numpy(),
                   lens.numpy(), [[si, ei]], T)
    assert (np.abs(desc - ref['desc'][0]) <= ref['desc_bar'][0]).all()     # the launch on the model's own taps, against float64
    m.backward()
    torch.cuda.synchronize()
    grads = m.grads_dict()
    for name, g in (('predictor/start_dense/kernel', desc[:128]), ('predictor/end_dense/kernel', desc[128:])):
        want = np.asarray(grads[name]).reshape(-1)
        scale = float(np.abs(want).max())
        err = float(np.abs(g - want).max())
        print('%s: max |g - grad| %.3e, tensor max %.3e, ratio %.3e (bar 1e-3); |g| %.3e |grad| %.3e cos %.4f' % (
            name, err, scale, err / scale, np.linalg.norm(g), np.linalg.norm(want), float(g @ want) / max(np.linalg.norm(g) * np.linalg.norm(want), 1e-300)))
        assert scale > 0 and err <= 1e-3 * scale
    assert float(bank.gnorm2[0]) == pytest.approx(float((desc.astype(np.float64) ** 2).sum()), rel=1e-6)


def _trainset(dev, N=20):
    """al_synth.make_trainset as a DeviceDataset with its pseudo-labels set, and a model of random weights for it"""
    from hual_amd import al, lib
    from hual_amd.dataset import DeviceDataset
    from hual_amd.model import SeqPAN
    vdim, max_vlen = 64, 24
    recs, vis, data_gt, data_old = al_synth.make_trainset(N, 6, vdim, max_vlen, seed=41)
    cfg = lib.make_cfg(vdim=vdim, max_vlen=max_vlen, num_words=200, num_chars=30)
    wv = np.random.default_rng(1).normal(0, 0.4, size=(198, 300)).astype(np.float32)
    ds = DeviceDataset(recs, vis, device=dev)
    s0, e0 = al.labels_from_times(data_old, ds.vlen_h)
    ds.set_labels(s0, e0)
    for r, a, b in zip(recs, s0, e0):
        r['s_ind'], r['e_ind'] = int(a), int(b)
    ds.lists = (data_old, data_gt)
    return SeqPAN(cfg, wv), ds


def test_infer_trainset_fills_the_bank_with_the_direct_launches(dev):
    from hual_amd import al, lib
    N, bs = 20, 8
    m, ds = _trainset(dev, N)
    rng0 = m.get_rng()
    base, ious0 = al.infer_trainset_sharded(m, ds, bs)
    m.set_rng(*rng0)
    again, _ = al.infer_trainset_sharded(m, ds, bs)
    for hyp_kind in al.GRAD_HYP:
        m.set_rng(*rng0)
        bank = al.GradBank.for_dataset(ds)
        got, ious = al.infer_trainset_sharded(m, ds, bs, grad_bank=bank, grad_hyp=hyp_kind)
        assert ious == ious0
        # the direct launches, batch by batch, on the same forward
        want = al.GradBank.for_dataset(ds)
        for lo in range(0, N, bs):
            sel = np.arange(lo, min(N, lo + bs))
            f = ds.assemble(sel, out=None, labels=False, min_chars=4)
            o = m.forward(f['video'], f['video_seq_len'], f['word_ids'], f['char_ids'])
            if hyp_kind == 'prediction':
                hyp = torch.stack([o['start_index'], o['end_index']], dim=1).to(torch.int32)
            else:
                hyp = torch.tensor([[ds.records[k]['s_ind'], ds.records[k]['e_ind']] for k in sel], dtype=torch.int32, device=dev)
            lib.al_grad_embed(m.tap('head.hs'), m.tap('head.he'), o['start_logits'], o['end_logits'], f['video_seq_len'], hyp, want.desc,
                              want.gnorm2, want.egl, rows=torch.from_numpy(sel.astype(np.int32)).to(dev))
        torch.cuda.synchronize()
        for name in ('desc', 'gnorm2', 'egl'):
            a, w = getattr(bank, name).cpu().numpy(), getattr(want, name).cpu().numpy()
            assert same_bits(a, w), (hyp_kind, name)
        egl, gn = bank.egl.cpu().numpy(), bank.gnorm2.cpu().numpy()
        assert (egl > 0).all() and np.isfinite(bank.desc.cpu().numpy()).all()
        for i, (r, r0) in enumerate(zip(got, base)):
            assert r['prop_egl'] == float(egl[i]) and r['prop_gnorm2'] == float(gn[i])
            assert sorted(r) == sorted(list(r0) + ['prop_egl', 'prop_gnorm2'])
    # without the argument: the records of the parent's pass
    assert al._head_taps(m)[1]                                             # the taps are read in place: nothing else lives in their bytes
    for r, r0 in zip(again, base):
        assert sorted(r) == sorted(r0) and 'prop_egl' not in r
        for k in r0:
            if k.startswith('prop_logits'):
                assert all(same_bits(np.asarray(x), np.asarray(y)) for x, y in zip(r[k], r0[k]))
            elif k == 'm_score':
                assert same_bits(r[k], r0[k])
            else:
                assert r[k] == r0[k], k


def test_taps_of_a_batch_of_several_clips_follow_the_row_stride(dev):
    """B = 3 through the whole model, clips of 20, 10 and 11 frames: sample b's rows of the taps are b * T .. b * T + T - 1.  The
    launch on the forward's own taps against float64 on the same taps read as [B, T, 128], and against the model's backward: the
    loss is the mean over the clips, so the gradient of a dense kernel is sum_b g_b / B"""
    from hual_amd import al, data
    B_, T = 3, 20
    cfg, p, wv, b, _ = pu.make_case(B=B_, T=T, L=6, C=5, seed=3)
    m = pu.hip_model(cfg, p, wv)
    lens = b['lens']
    assert len(set(lens.tolist())) > 1                                     # clips of different lengths
    o = m.forward(b['video'], lens, b['word_ids'], b['char_ids'])
    si, ei = o['start_index'].cpu().numpy(), o['end_index'].cpu().numpy()
    _, _, ml, il = data.make_labels(si, ei, lens.numpy(), max_len=T)
    y1, y2 = np.zeros((B_, T), dtype=np.float32), np.zeros((B_, T), dtype=np.float32)
    y1[np.arange(B_), si] = y2[np.arange(B_), ei] = 1.0
    labels = (torch.tensor(y1), torch.tensor(y2), torch.tensor(ml), torch.tensor(il, dtype=torch.float32))
    o = m.forward(b['video'], lens, b['word_ids'], b['char_ids'], labels=labels)
    bank = al.GradBank(B_, device=dev)
    hyp = torch.from_numpy(np.stack([si, ei], axis=1).astype(np.int32)).to(dev)
    bank.embed(m, o, lens.to(device=dev, dtype=torch.int32), None, hyp)
    desc = bank.desc.cpu().numpy()
    hs, he = m.tap('head.hs').cpu().numpy(), m.tap('head.he').cpu().numpy()
    assert hs.shape == (B_ * T, 128)
    ref = GR.embed(hs, he, o['start_logits'].cpu().numpy(), o['end_logits'].cpu().numpy(), lens.numpy(), hyp.cpu().numpy(), T)
    assert not ref['poisoned'].any()
    assert (np.abs(desc - ref['desc']) <= ref['desc_bar']).all()
    m.backward()
    torch.cuda.synchronize()
    grads = m.grads_dict()
    for name, g in (('predictor/start_dense/kernel', desc[:, :128]), ('predictor/end_dense/kernel', desc[:, 128:])):
        want = np.asarray(grads[name]).reshape(-1)
        mine = g.astype(np.float64).sum(axis=0) / B_                       # the loss is the mean over the clips
        scale = float(np.abs(want).max())
        err = float(np.abs(mine - want).max())
        print('%s (B = 3): max |sum_b g_b / B - grad| %.3e, tensor max %.3e, ratio %.3e (bar 1e-3)' % (name, err, scale, err / scale))
        assert scale > 0 and err <= 1e-3 * scale


def _asked(new, old):
    n = lambda r: (len(r[4]['pos_idx']) + len(r[4]['neg_idx'])) if len(r) > 4 else 0
    return [i for i in range(len(new)) if n(new[i]) > n(old[i])]


def test_a_round_fills_the_bank_the_next_round_selects_from(dev):
    """run_round(grad_bank=True) returns the bank of its inference; its records rank the next round by 'egl' and its desc is the
    space of select_by='badge'"""
    from hual_amd import al
    N, bs = 20, 8
    m, ds = _trainset(dev, N)
    data_old, data_gt = ds.lists
    prop0, _ = al.infer_trainset_sharded(m, ds, bs)
    kw = dict(epochs=0, batch_size=bs, lr=1e-3, drop_rate=0.1, mc_dropout=None)
    new1, prop1, met = al.run_round(m, ds, copy.deepcopy(data_old), data_gt, prop0, 'charades', 1, grad_bank=True, **kw)
    bank = met['grad_bank']
    assert isinstance(bank, al.GradBank) and bank.N == N and all('prop_egl' in p and 'prop_gnorm2' in p for p in prop1)
    direct = al.GradBank.for_dataset(ds)                                   # no training epoch: the same model, so the same bank
    al.infer_trainset_sharded(m, ds, bs, grad_bank=direct)
    for name in ('desc', 'gnorm2', 'egl'):
        assert same_bits(getattr(bank, name).cpu().numpy(), getattr(direct, name).cpu().numpy()), name
    egl = bank.egl.cpu().numpy()
    assert [p['prop_egl'] for p in prop1] == [float(v) for v in egl]
    # a bank of the caller's is filled in place; 'pseudo' reaches the launch
    mine = al.GradBank.for_dataset(ds)
    _, prop2, met2 = al.run_round(m, ds, copy.deepcopy(new1), data_gt, prop1, 'charades', 2, grad_bank=mine, grad_hyp='pseudo', **kw)
    assert met2['grad_bank'] is mine and same_bits(mine.egl.cpu().numpy(), egl)      # egl does not depend on the hypothesis
    assert not same_bits(mine.desc.cpu().numpy(), bank.desc.cpu().numpy())
    _, prop3, met3 = al.run_round(m, ds, copy.deepcopy(new1), data_gt, prop1, 'charades', 2, **kw)
    assert 'grad_bank' not in met3 and 'prop_egl' not in prop3[0]
    for bad in (dict(grad_bank=al.GradBank(N + 1, device=dev)), dict(grad_bank=object()), dict(grad_bank=True, grad_hyp='truth')):
        with pytest.raises(ValueError):
            al.run_round(m, ds, copy.deepcopy(new1), data_gt, prop1, 'charades', 2, **dict(kw, **bad))
    # the next round: ranked by the records' egl, the asked half drawn in the bank's space
    coff = al.get_coff('charades', 2)
    new2, dbg = al.update_labels(copy.deepcopy(new1), data_gt, prop1, coff, return_debug=True, rank_by='egl', select_by='badge',
                                 descriptors=bank.desc, selection_seed=3)
    np.testing.assert_array_equal(dbg['order'], np.argsort(-egl.astype(np.float64), kind='stable'))
    sel = al.badge_select(bank.desc, math.ceil(N / 2), seed=3)[0]
    assert len(sel) == 10 and sorted(_asked(new2, new1)) == sorted(sel.tolist())
    np.testing.assert_array_equal(dbg['kcenter_picked'], sel)
    # the same through run_round: metrics['diversity'] holds the three keys
    _, _, met4 = al.run_round(m, ds, copy.deepcopy(new1), data_gt, prop1, 'charades', 2, rank_by='egl', select_by='badge',
                              descriptors=bank.desc, selection_seed=3, **kw)
    assert sorted(met4['diversity']) == ['cover_radius', 'kcenter_dist', 'kcenter_picked']
    np.testing.assert_array_equal(met4['diversity']['kcenter_picked'], sel)


def test_the_runner_passes_the_bank_through(dev, tmp_path):
    from hual_amd import al
    from hual_amd.runner import Runner
    vdim = 64
    vis = _videos(8, vdim, 0)
    train, test = _task(24, vis, 1), _task(8, vis, 2)
    cfg = dict(task='synth', train=dict(batch_size=16, droprate=0.1, lr=2e-3, epochs=1, clip_norm=1.0),
               model=dict(vdim=vdim, dim=128, num_heads=8, word_dim=300, char_dim=50, max_vlen=32, attn_layer=2),
               loss=dict(match_lambda=1.0, tau=0.3, no_gumbel=True), num_chars=10)
    wv = np.random.default_rng(0).normal(0, 0.4, size=(40, 300)).astype(np.float32)

    class L:
        def info(self, s):
            pass
    r = Runner(cfg, wv, train, test, vis, ckpt_dir=str(tmp_path / 'ckpt'), logger=L())
    bank = al.GradBank(len(train), device=dev)
    recs, _ = r.infer_trainset(load_best=False, grad_bank=bank)
    egl = bank.egl.cpu().numpy()
    assert len(recs) == len(train) and [p['prop_egl'] for p in recs] == [float(v) for v in egl] and (egl > 0).all()
    assert 'prop_egl' not in r.infer_trainset(load_best=False)[0][0]
