"""GPU: hual_span_expected_iou (expected temporal IoU of proposals, span entropy, minimum-Bayes-risk order) against the float64
reference of its contract (tests/span_conf_ref.py), its edge rows, its in-place reorder, graph capture, and the three places it
lands: Runner.evaluate(rerank=), the records of al.infer_trainset(span_conf=) and al.update_labels(rank_by='span_risk').

The bars (derived from the contract's arithmetic, include/hual_seqpan.h; not tuned):
  expected IoU  1e-6 absolute: three float32 roundings per term (the product p_s * p_e, the ratio inter / union, their product) on
                non-negative terms, float64 accumulation (exact to 1e-16) and one final rounding - at most 5 * 2^-24 = 3e-7 on a value
                that is at most 1; the bar is about three times that.
  entropy       5e-5 bits: with |logit| <= 8 and T <= 256 every |log2 p| <= 16 log2(e) + 8 = 31.1, so two log2f at 2 ulp (2^-19 each
                there) plus the rounding of their float32 sum (|sum| < 64: 2^-19) stay under 1.5e-5 per term, and H is an average of
                such terms over weights that sum to 1, plus the float32 rounding of H itself (< 16: 2^-21); about three times that.
"""
import copy
import functools
import math

import numpy as np
import pytest
import torch

import al_synth
import span_conf_ref as C
import span_topk_ref as R
from span_clip_util import _pads_intact, _sentinel, _task, _videos

pytestmark = pytest.mark.gpu

EI_BAR, ENT_BAR = 1e-6, 5e-5
# SEED: one for which the REFERENCE alone (no device value) gives every row's valid values more than ten bars apart at every (T, k)
# below (the smallest gap is 1.0e-4) and at least 3 of the 16 rows a new slot 0 at T >= 33 (4 to 7): both are asserted again below
B, TS, KS, SEED = 16, (2, 33, 70, 256), (1, 5, 16), 16


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def inputs(T, seed=SEED):
    """logits N(0, sigma = 2) clipped to |x| <= 8, lengths 1, T - 1, T and random ones"""
    g = torch.Generator().manual_seed(1000 * seed + T)
    s = (torch.randn(B, T, generator=g) * 2).clamp(-8, 8)
    e = (torch.randn(B, T, generator=g) * 2).clamp(-8, 8)
    vl = torch.randint(1, T + 1, (B,), generator=g, dtype=torch.int32)
    vl[0], vl[1], vl[2] = 1, max(1, T - 1), T
    return s, e, vl


def _run(dev, s, e, vl, st, en, sc=None, reorder=False):
    """one launch into sentinel-filled outputs; -> numpy (expected_iou, entropy) after checking the memory around them"""
    from hual_amd import lib
    k = st.shape[1]
    ei, ei_w, p1 = _sentinel((s.shape[0], k), torch.float32, dev, 777.0)
    ent, ent_w, p2 = _sentinel((s.shape[0],), torch.float32, dev, 777.0)
    got = lib.span_expected_iou(s, e, vl, st, en, score=sc, reorder=reorder, out=(ei, ent))
    assert got[0] is ei and got[1] is ent
    torch.cuda.synchronize()
    assert _pads_intact(ei_w, p1, 777.0) and _pads_intact(ent_w, p2, 777.0)
    assert not bool((ei == 777.0).any()) and not bool((ent == 777.0).any())          # every slot of [B,k] / [B] was written
    return ei.cpu().numpy(), ent.cpu().numpy()


_CASES = {}


def case(dev, T, k):
    """inputs, the candidates of lib.span_topk at nms_iou 0.5, the float64 reference and the reorder=0 device values: computed once"""
    if (T, k) not in _CASES:
        from hual_amd import lib
        s, e, vl = inputs(T)
        sd, ed, vd = s.to(dev), e.to(dev), vl.to(dev)
        st, en, sc = lib.span_topk(sd, ed, vd, k, nms_iou=0.5)
        keep = (st.clone(), en.clone(), sc.clone())
        ei, ent = _run(dev, sd, ed, vd, st, en, sc, reorder=False)
        for a, b in zip((st, en, sc), keep):                          # reorder=0: the candidate arrays are only read
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        sth, enh = st.cpu().numpy(), en.cpu().numpy()
        ref = C.span_conf_ref(s, e, vl, sth, enh)
        _CASES[(T, k)] = dict(dev=(sd, ed, vd, st, en, sc), st=sth, en=enh, sc=sc.cpu().numpy(), ei=ei, ent=ent, ref=ref)
    return _CASES[(T, k)]


# ---------------------------------------------------------------------------------------------------------------- 1. values
@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('T', TS)
def test_values_against_the_float64_reference(dev, T, k):
    c = case(dev, T, k)
    rei, rent, alive = c['ref']
    assert alive.all()
    valid = c['st'] >= 0
    assert valid[:, 0].all() and (valid == (rei >= 0)).all()
    assert (c['ei'][~valid] == -1.0).all()
    d_ei = float(np.abs(c['ei'][valid].astype(np.float64) - rei[valid]).max())
    d_ent = float(np.abs(c['ent'].astype(np.float64) - rent).max())
    print('T=%d k=%d: max |expected IoU - ref| = %.3e (bar %.0e), max |entropy - ref| = %.3e bits (bar %.0e)' % (T, k, d_ei, EI_BAR, d_ent, ENT_BAR))
    assert d_ei <= EI_BAR
    assert d_ent <= ENT_BAR
    assert (c['ei'][valid] >= 0).all() and (c['ei'][valid] <= 1).all()
    v = np.minimum(inputs(T)[2].numpy().astype(np.int64), T)
    assert (c['ent'] >= 0).all() and (c['ent'] <= np.log2(v * (v + 1) / 2) + ENT_BAR).all()
    assert c['ei'][0, 0] == 1.0 and c['ent'][0] == 0.0              # v == 1, exactly
    # the entropy does not depend on the candidates
    assert (c['ent'].view(np.int32) == case(dev, T, KS[0])['ent'].view(np.int32)).all()


# ---------------------------------------------------------------------------------------------------------------- 2. edge rows
def test_edge_rows_and_untouched_memory(dev):
    T, k = 33, 5
    s, e, vl = (x.clone() for x in inputs(T))
    s[4, 3] = float('nan')                                        # a NaN logit inside the clip (in the host input): row 4 is poisoned
    e[5, 30] = float('nan')                                       # beyond vlen = 20: not read
    vl[3], vl[5], vl[6], vl[7] = 0, 20, T + 9, -2                 # empty; short; read as T; empty
    s[9, :], e[9, :] = -200.0, -200.0                             # row 9 (vlen 20): the start certainly last, the end certainly first -
    s[9, 19], e[9, 0] = 200.0, 200.0                              # every weight with i <= j is exactly 0, Z = 0: as a poisoned row
    s[10, 5] = float('inf')                                       # row 10: an infinite logit makes the probabilities NaN, Z with them
    st = torch.tensor([[0, 0, -1, 1, 0]] + [[2, 9, -1, 0, 5]] * (B - 1), dtype=torch.int64)
    en = torch.tensor([[0, 0, -1, 1, 1]] + [[6, 4, -1, T - 1, 20]] * (B - 1), dtype=torch.int64)       # (9, 4): a > b; (-1, -1): no proposal
    en[8, 2] = 4                                                  # (-1, 4): a negative start alone
    sc = torch.arange(B * k, dtype=torch.float32).view(B, k)
    sd, ed, vd = s.to(dev), e.to(dev), vl.to(dev)
    rei, rent, alive = C.span_conf_ref(s, e, vl, st.numpy(), en.numpy())
    assert int(vl[9]) == 20 and list(np.nonzero(~alive)[0]) == [3, 4, 7, 9, 10]
    for reorder in (False, True):
        std, st_w, p0 = _sentinel((B, k), torch.int64, dev, -99)
        end, en_w, _ = _sentinel((B, k), torch.int64, dev, -99)
        scd, sc_w, _ = _sentinel((B, k), torch.float32, dev, -99.0)
        std.copy_(st), end.copy_(en), scd.copy_(sc)
        ei, ent = _run(dev, sd, ed, vd, std, end, scd, reorder=reorder)
        assert _pads_intact(st_w, p0, -99) and _pads_intact(en_w, p0, -99) and _pads_intact(sc_w, p0, -99.0)
        sth, enh, sch = std.cpu().numpy(), end.cpu().numpy(), scd.cpu().numpy()
        # row 0 (v = 1): (0, 0) is the only valid span, (1, 1) and (0, 1) end beyond the clip
        assert ent[0] == 0.0 and sorted(ei[0]) == [-1.0, -1.0, -1.0, 1.0, 1.0]
        for b in (3, 4, 7, 9, 10):                                    # empty, NaN, empty, Z = 0, Z = NaN: all -1 and never reordered
            assert (ei[b] == -1.0).all() and ent[b] == -1.0
            assert (sth[b] == st[b].numpy()).all() and (enh[b] == en[b].numpy()).all() and (sch[b] == sc[b].numpy()).all()
        if not reorder:
            assert (sth == st.numpy()).all() and (enh == en.numpy()).all() and (sch.view(np.int32) == sc.numpy().view(np.int32)).all()
            assert ((ei == -1.0) == (rei == -1.0)).all()
            assert (ei[1:, 1] == -1.0).all() and (ei[1:, 2] == -1.0).all()                  # a > b, no proposal
            assert ei[5, 3] == -1.0 and ei[5, 4] == -1.0 and ei[5, 0] >= 0                  # b >= vlen = 20
            assert ei[6, 3] >= 0 and ei[2, 3] >= 0 and ei[1, 3] == -1.0                     # vlen read as T; T; T - 1
            ok = rei >= 0
            assert float(np.abs(ei[ok] - rei[ok]).max()) <= EI_BAR and float(np.abs(ent - rent).max()) <= ENT_BAR
        else:
            for b in np.nonzero(alive)[0]:
                o = C.stable_order(rei[b])                            # (row 0: 1.0, 1.0 and three invalid slots - nothing moves)
                vals = np.sort(rei[b][rei[b] >= 0])
                assert b == 0 or len(vals) < 2 or np.diff(vals).min() > 10 * EI_BAR       # the other rows' values are far apart
                assert (sth[b] == st[b].numpy()[o]).all() and (enh[b] == en[b].numpy()[o]).all() and (sch[b] == sc[b].numpy()[o]).all()
                assert ((ei[b] == -1.0) == (rei[b][o] == -1.0)).all()


# ---------------------------------------------------------------------------------------------------------------- 3. reorder
@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('T', TS)
def test_reorder_is_a_stable_sort_by_expected_iou(dev, T, k):
    c = case(dev, T, k)
    sd, ed, vd, st, en, sc = c['dev']
    st2, en2, sc2 = st.clone(), en.clone(), sc.clone()
    ei, ent = _run(dev, sd, ed, vd, st2, en2, sc2, reorder=True)
    assert (ent.view(np.int32) == c['ent'].view(np.int32)).all()
    rei = c['ref'][0]
    changed = 0
    for b in range(B):
        o = C.stable_order(c['ei'][b])                                # host stable sort of the reorder=0 device values
        assert (st2[b].cpu().numpy() == c['st'][b][o]).all() and (en2[b].cpu().numpy() == c['en'][b][o]).all()
        assert (sc2[b].cpu().numpy().view(np.int32) == c['sc'][b][o].view(np.int32)).all()
        assert (ei[b].view(np.int32) == c['ei'][b][o].view(np.int32)).all()
        # ... which is the reference's order: its values are more than ten bars apart in every row of these inputs
        vals = np.sort(rei[b][rei[b] >= 0])
        assert len(vals) < 2 or np.diff(vals).min() > 10 * EI_BAR, (b, np.diff(vals).min())
        assert (o == C.stable_order(rei[b])).all()
        changed += int(o[0] != 0)
    print('T=%d k=%d: %d of %d rows change slot 0' % (T, k, changed, B))
    if T >= 33 and k > 1:
        assert changed >= 3                                           # a different decoder, not a relabelling
    if k == 1:
        assert changed == 0


# ---------------------------------------------------------------------------------------------------------------- 6. capture
def test_expected_iou_in_a_captured_graph(dev):
    from hual_amd import lib
    T, k = 70, 5
    c = case(dev, T, k)
    sd, ed, vd, st, en, sc = c['dev']
    work = (st.clone(), en.clone(), sc.clone())
    out = (torch.empty(B, k, dtype=torch.float32, device=dev), torch.empty(B, dtype=torch.float32, device=dev))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        lib.span_expected_iou(sd, ed, vd, work[0].clone(), work[1].clone(), score=work[2].clone(), reorder=True, out=out)      # (warm-up)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        lib.span_expected_iou(sd, ed, vd, work[0], work[1], score=work[2], reorder=True, out=out)
    eager = (st.clone(), en.clone(), sc.clone())
    want = lib.span_expected_iou(sd, ed, vd, eager[0], eager[1], score=eager[2], reorder=True)
    for _ in range(2):
        for w, src in zip(work, (st, en, sc)):
            w.copy_(src)
        for o in out:
            o.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(work + out, eager + tuple(want)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------- 4. evaluation
def test_reranked_evaluation(tmp_path):
    from hual_amd import al, data
    from hual_amd.runner import Runner
    vdim, k = 64, 5
    vis = _videos(12, vdim, 0)
    train, test = _task(64, vis, 1), _task(48, vis, 2)
    cfg = dict(task='synth', train=dict(batch_size=32, droprate=0.1, lr=2e-3, epochs=1, clip_norm=1.0),
               model=dict(vdim=vdim, dim=128, num_heads=8, word_dim=300, char_dim=50, max_vlen=32, attn_layer=2),
               loss=dict(match_lambda=1.0, tau=0.3, no_gumbel=True), num_chars=10)
    wv = np.random.default_rng(0).normal(0, 0.4, size=(40, 300)).astype(np.float32)
    lines = []

    class L:
        def info(self, s):
            lines.append(str(s))
    r = Runner(cfg, wv, train, test, vis, ckpt_dir=str(tmp_path / 'ckpt'), logger=L())
    r.train_epoch(2e-3)
    t = r.test_epoch()
    plain, props0 = r.evaluate(k=k, nms_iou=0.5, return_proposals=True)
    # without rerank: the keys, values and tuples of before
    assert sorted(plain) == sorted(['R1@0.3', 'R1@0.5', 'R1@0.7', 'R5@0.3', 'R5@0.5', 'R5@0.7', 'mIoU'])
    assert (plain['R1@0.3'], plain['R1@0.5'], plain['R1@0.7'], plain['mIoU']) == t
    assert all(len(x) == 3 for p in props0 for x in p)
    assert r.evaluate(k=k, nms_iou=0.5, rerank=None) == plain
    n_lines = len(lines)
    res, props = r.evaluate(k=k, nms_iou=0.5, rerank='expected_iou', return_proposals=True)
    assert sorted(res) == sorted(list(plain) + ['conf', 'span_entropy'])
    assert any('expected IoU' in l for l in lines[n_lines:])
    for th in ('0.3', '0.5', '0.7'):
        assert res['R5@' + th] == plain['R5@' + th]                   # the same set of proposals
    ds = r.test_set
    first, conf = [], []
    for i, (p0, p) in enumerate(zip(props0, props)):
        assert len(p) == len(p0) == k and all(len(x) == 4 for x in p)
        assert sorted(x[:3] for x in p) == sorted(p0)                 # a permutation of the plain proposals, scores carried along
        vals = [x[3] for x in p]
        assert all(0.0 <= x <= 1.0 for x in vals) and vals == sorted(vals, reverse=True)
        rec = ds.records[i]
        gt = data.index_to_time([rec['s_ind'], rec['e_ind']], rec['v_len'], rec['duration'])
        first.append(al.calculate_iou(p[0][:2], gt))
        conf.append(vals[0])
    m = al.iou_metrics(first)
    assert (res['R1@0.3'], res['R1@0.5'], res['R1@0.7'], res['mIoU']) == m
    assert res['conf'] == float(np.mean(np.asarray(conf, dtype=np.float32), dtype=np.float64))
    assert 0 < res['span_entropy'] <= math.log2(32 * 33 / 2)
    # per clip: the float64 reference on the logits of the same forward
    moved = 0
    for lo in range(0, len(ds), r.batch_size):
        sel = np.arange(lo, min(len(ds), lo + r.batch_size))
        f = ds.assemble(sel, labels=False, min_chars=4)
        o = r.model.forward(f['video'], f['video_seq_len'], f['word_ids'], f['char_ids'], drop_rate=0.0)
        sl, el, vl = o['start_logits'].cpu(), o['end_logits'].cpu(), f['video_seq_len'].cpu()
        st, en, sc = R.span_topk_ref(sl, el, vl, k, nms_iou=0.5)
        rei, _, alive = C.span_conf_ref(sl, el, vl, st, en)
        assert alive.all()
        for row, i in enumerate(sel):
            rec = ds.records[i]
            want = {tuple(float(x) for x in data.index_to_time((a, b), rec['v_len'], rec['duration'])): v for a, b, v in zip(st[row], en[row], rei[row])}
            for x in props[i]:
                assert abs(x[3] - want[x[:2]]) <= EI_BAR
            moved += int(props[i][0][:3] != props0[i][0])
    print('re-ranked evaluation: slot 0 changed in %d of %d clips; conf %.4f, span entropy %.3f bits' % (moved, len(ds), res['conf'], res['span_entropy']))
    with pytest.raises(ValueError, match='rerank'):
        r.evaluate(rerank='score')
    # the records switch through the runner
    recs, _ = r.infer_trainset(load_best=False, span_conf=True)
    assert len(recs) == len(train) and all(0.0 <= p['prop_conf'] <= 1.0 and p['prop_span_entropy'] >= 0.0 for p in recs)
    assert 'prop_conf' not in r.infer_trainset(load_best=False)[0][0]


# ---------------------------------------------------------------------------------------------------------------- 5. records, ranking
@functools.lru_cache(maxsize=None)
def _round_set():
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
    return dict(N=N, recs=recs, data_gt=data_gt, data_old=data_old, model=model, ds=ds)


def _batches(S, bs=16):
    for lo in range(0, S['N'], bs):
        sel = np.arange(lo, min(S['N'], lo + bs))
        f = S['ds'].assemble(sel, labels=False, min_chars=4)
        yield [S['recs'][i] for i in sel], f['video'], f['video_seq_len'], f['word_ids'], f['char_ids']


def test_records_and_ranking(dev):
    from hual_amd import al, lib
    S = _round_set()
    model, N = S['model'], S['N']
    prop0, ious0 = al.infer_trainset(model, _batches(S))
    prop1, ious1 = al.infer_trainset(model, _batches(S), span_conf=True)
    assert ious0 == ious1
    assert set(prop1[0]) == set(prop0[0]) | {'prop_conf', 'prop_span_entropy'}
    for a, b in zip(prop0, prop1):
        for key in a:
            if isinstance(a[key], (list, np.ndarray)) and key != 'psuedo_idx' and key != 'prop_idx':
                np.testing.assert_array_equal(np.asarray(a[key]), np.asarray(b[key]))
            else:
                assert a[key] == b[key]
        assert type(b['prop_conf']) is float and type(b['prop_span_entropy']) is float
        # a direct launch on the recorded logits: the same bits
        sl, el = (torch.from_numpy(np.ascontiguousarray(x))[None].to(dev) for x in b['prop_logits'])
        idx = torch.tensor([b['prop_idx']], dtype=torch.int64, device=dev)
        ei, ent = lib.span_expected_iou(sl, el, torch.tensor([b['v_len']], dtype=torch.int32, device=dev), idx[:, :1].contiguous(),
                                        idx[:, 1:].contiguous())
        assert b['prop_conf'] == float(ei[0, 0]) and b['prop_span_entropy'] == float(ent[0])
        assert 0.0 <= b['prop_conf'] <= 1.0 and b['prop_span_entropy'] >= 0.0
    assert len({p['prop_conf'] for p in prop1}) > N // 2               # the key separates the samples
    # ranking: the default is what it was, span_risk ranks by 1 - prop_conf
    coff = al.get_coff('charades', 1)
    new0, d0 = al.update_labels(copy.deepcopy(S['data_old']), S['data_gt'], prop0, coff, return_debug=True)
    new1, d1 = al.update_labels(copy.deepcopy(S['data_old']), S['data_gt'], prop1, coff, return_debug=True)
    assert sorted(d0) == sorted(d1) == sorted(['order', 'uncert_video', 'observe', 'uncert_frame', 'sprob', 'eprob', 'new_idx', 'gt_idx',
                                                'old_idx', 'updater'])
    for key in d0:
        if key != 'updater':
            np.testing.assert_array_equal(d0[key], d1[key])
    assert new0 == new1
    np.testing.assert_array_equal(d0['order'], np.argsort(d0['uncert_video'], kind='stable'))
    new2, d2 = al.update_labels(copy.deepcopy(S['data_old']), S['data_gt'], prop1, coff, rank_by='span_risk', return_debug=True)
    risk = 1.0 - np.array([p['prop_conf'] for p in prop1], dtype=np.float64)
    np.testing.assert_array_equal(d2['span_risk'], risk)
    np.testing.assert_array_equal(d2['order'], np.argsort(risk, kind='stable'))
    sel = d2['order'][:math.ceil(N / 2)]
    assert not np.array_equal(d2['order'], d0['order'])
    for key in ('uncert_video', 'observe', 'uncert_frame', 'sprob', 'eprob', 'gt_idx', 'old_idx'):      # the scoring itself is unchanged
        np.testing.assert_array_equal(d2[key], d0[key])
    changed = [i for i in range(N) if new2[i][2] != S['data_old'][i][2] or new2[i][4] != {'pos_idx': [], 'neg_idx': []}]
    assert set(changed) <= set(int(i) for i in sel)
    assert all(len(new2[i][4]['pos_idx']) + len(new2[i][4]['neg_idx']) == (1 if i in set(int(x) for x in sel) else 0) for i in range(N))
    with pytest.raises(ValueError, match='prop_conf'):
        al.update_labels(copy.deepcopy(S['data_old']), S['data_gt'], prop0, coff, rank_by='span_risk')
    # the switch reaches the sharded pass and the round (no training epoch: the same model, so the same two floats)
    want = [(p['prop_conf'], p['prop_span_entropy']) for p in prop1]
    prop2, _ = al.infer_trainset_sharded(model, S['ds'], 16, span_conf=True)
    assert [(p['prop_conf'], p['prop_span_entropy']) for p in prop2] == want
    assert 'prop_conf' not in al.infer_trainset_sharded(model, S['ds'], 16)[0][0]
    _, prop3, _ = al.run_round(model, S['ds'], copy.deepcopy(S['data_old']), S['data_gt'], prop1, 'charades', 1, epochs=0, batch_size=16,
                               lr=1e-3, drop_rate=0.1, mc_dropout=None, span_conf=True)
    assert [(p['prop_conf'], p['prop_span_entropy']) for p in prop3] == want
