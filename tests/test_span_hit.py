"""CPU: the enumeration reference of hual_span_hit_prob (tests/span_hit_ref.py) against the identities of the quantity,
al.hit_calibration on hand-made inputs, the threshold conversion of lib.span_hit_prob and the entry point's host-side argument checks
(no GPU needed)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import span_conf_ref as C
import span_hit_ref as H
import span_topk_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THR3 = [(3, 10), (1, 2), (7, 10)]


def _logits(B, T, seed, scale=2.0):
    g = torch.Generator().manual_seed(seed)
    s, e = torch.randn(B, T, generator=g) * scale, torch.randn(B, T, generator=g) * scale
    vl = torch.randint(1, T + 1, (B,), generator=g, dtype=torch.int32)
    vl[0], vl[1] = T, 1
    return s, e, vl


# ---------------------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize('T', [2, 9, 33])
def test_reference_identities(T):
    s, e, vl = _logits(8, T, 70 + T)
    st, en, _ = R.span_topk_ref(s, e, vl, 5, nms_iou=0.5)
    thr = [(1, 1024), (3, 10), (1, 2), (7, 10), (1, 1)]
    hp, alive = H.span_hit_ref(s, e, vl, st, en, thr)
    assert alive.all()
    valid = st >= 0
    assert (hp[valid] >= 0).all() and (hp[valid] <= 1 + 1e-15).all() and (hp[~valid] == -1.0).all()
    assert (np.diff(hp[valid], axis=1) <= 1e-15).all()              # a hit at a higher threshold is a hit at every lower one
    ps, pe, vv, _ = R.probabilities(s, e, vl)
    for b in range(8):
        ii, jj, w = C.span_weights(ps[b], pe[b], int(vv[b]))
        for q in np.nonzero(valid[b])[0]:
            a, z = int(st[b, q]), int(en[b, q])
            p_span = w[(ii == a) & (jj == z)][0] / w.sum()
            p_overlap = w[(ii <= z) & (jj >= a)].sum() / w.sum()
            assert abs(hp[b, q, 4] - p_span) <= 1e-15               # IoU >= 1: the span itself, P(a, b)
            assert abs(hp[b, q, 0] - p_overlap) <= 1e-15            # IoU >= 1 / 1024 with at most 256 frames: any overlap at all
    assert (hp[1, 0] == 1.0).all() and (st[1, 1:] == -1).all()      # v == 1: the one span has probability 1


def test_reference_hit_rule_is_the_integer_rule():
    ii, jj = np.array([0, 0, 2, 4, 5]), np.array([9, 4, 6, 9, 9])
    # candidate [0, 9] (10 frames): inter 10, 5, 5, 6, 5 over union 10 - IoU 1, 0.5, 0.5, 0.6, 0.5
    assert list(H.hits(0, 9, ii, jj, 1, 2)) == [True, True, True, True, True]          # equality counts as a hit
    assert list(H.hits(0, 9, ii, jj, 3, 5)) == [True, False, False, True, False]
    assert list(H.hits(0, 9, ii, jj, 7, 10)) == [True, False, False, False, False]
    assert list(H.hits(3, 3, np.array([0, 3, 4]), np.array([2, 3, 9]), 1, 1024)) == [False, True, False]      # no overlap: never


def test_reference_bayes_span_and_dead_rows():
    s, e, vl = _logits(6, 10, 5)
    vl[:] = torch.tensor([10, 1, 0, 10, 6, 2])
    s[3, 4] = float('nan')                                        # inside the clip: the row is poisoned
    e[4, 8] = float('nan')                                        # beyond vlen = 6: not read
    rows = H.bayes_ref(s, e, vl, THR3 + [(1, 1)])
    assert [r is None for r in rows] == [False, False, True, True, False, False]
    assert len(rows[0]['ii']) == 55 and len(rows[4]['ii']) == 21 and len(rows[5]['ii']) == 3
    assert (rows[1]['top'] == 1.0).all() and (rows[1]['best'] == 0).all() and np.isinf(rows[1]['gap']).all()
    ps, pe, _, _ = R.probabilities(s, e, vl)
    for b in (0, 4, 5):
        r = rows[b]
        assert (r['gap'] >= 0).all() and (np.diff(r['top']) <= 1e-15).all()
        ii, jj, w = C.span_weights(ps[b], pe[b], int(vl[b]))
        assert r['best'][3] == int(np.argmax(w))                    # threshold 1 / 1: the most probable span
        st = np.array([r['ii'][r['best']]])
        en = np.array([r['jj'][r['best']]])                         # the maximisers as proposals: the same values through the other path
        one = H.clip_hit_prob(ps[b], pe[b], int(vl[b]), list(zip(st[0], en[0])), THR3 + [(1, 1)])
        assert np.allclose(np.diag(one), r['top'], rtol=0, atol=1e-15)
    hp, alive = H.span_hit_ref(s, e, vl, np.array([[0, 5, -1, 3]] * 6), np.array([[2, 4, -1, 9]] * 6), THR3)
    assert list(alive) == [True, True, False, False, True, True]
    assert (hp[2] == -1).all() and (hp[3] == -1).all() and (hp[0, 1] == -1).all() and (hp[0, 2] == -1).all() and (hp[4, 3] == -1).all()
    assert (hp[0, 0] > 0).all() and (hp[0, 3] > 0).all()


# ---------------------------------------------------------------------------------------------------------------- hit_calibration
def test_hit_calibration_on_hand_made_inputs():
    from hual_amd import al
    # perfectly calibrated: of 10 entries at 0.2 two hit, of 10 at 0.8 eight
    prob = [0.2] * 10 + [0.8] * 10
    hit = [1, 1] + [0] * 8 + [1] * 8 + [0, 0]
    c = al.hit_calibration(prob, hit)
    assert c['n'] == 20 and list(c['count']) == [0, 0, 10, 0, 0, 0, 0, 0, 10, 0]
    assert abs(c['ece']) <= 1e-15 and abs(c['brier'] - 0.16) <= 1e-15
    assert np.isnan(c['hit_rate'][0]) and abs(c['hit_rate'][2] - 0.2) <= 1e-15 and abs(c['mean_prob'][8] - 0.8) <= 1e-15
    # entries below 0 count out, whatever their hit says
    d = al.hit_calibration(prob + [-1.0, -1.0], hit + [1, 0])
    assert d['n'] == 20 and d['ece'] == c['ece'] and d['brier'] == c['brier'] and (d['count'] == c['count']).all()
    # overconfident by 0.5 everywhere
    o = al.hit_calibration([1.0, 1.0, 1.0, 1.0], [1, 0, 1, 0], bins=4)
    assert list(o['count']) == [0, 0, 0, 4] and o['ece'] == 0.5 and o['brier'] == 0.5
    # bin edges: q / bins belongs to bin q, 1.0 to the last
    e = al.hit_calibration([0.0, 0.25, 0.4999, 0.5, 0.75, 1.0], [0] * 6, bins=4)
    assert list(e['count']) == [1, 2, 1, 2]
    e = al.hit_calibration(np.array([0.0, 0.1, 0.3, 0.7, 0.9, 1.0]), np.zeros(6, dtype=bool))
    assert list(e['count']) == [1, 1, 0, 1, 0, 0, 0, 1, 0, 2]
    # ece is count weighted: bin 0 holds 3 entries 0.1 off, bin 1 one entry 0.4 off
    x = al.hit_calibration([0.1, 0.1, 0.1, 0.6], [0, 0, 0, 1], bins=2)
    assert abs(x['ece'] - (3 * 0.1 + 0.4) / 4) <= 1e-15
    empty = al.hit_calibration([-1.0], [1])
    assert empty['n'] == 0 and np.isnan(empty['ece']) and np.isnan(empty['brier']) and empty['count'].sum() == 0
    with pytest.raises(ValueError, match='same number'):
        al.hit_calibration([0.5, 0.5], [1])
    with pytest.raises(ValueError, match='bins'):
        al.hit_calibration([0.5], [1], bins=0)
    with pytest.raises(ValueError, match='exceed 1'):
        al.hit_calibration([1.5], [1])


# ---------------------------------------------------------------------------------------------------------------- the binding
def test_threshold_conversion():
    from hual_amd import lib
    assert lib.hit_thresholds((0.3, 0.5, 0.7)) == THR3
    assert lib.hit_thresholds([(3, 10), (2, 4), 1.0, 1 / 1024]) == [(3, 10), (1, 2), (1, 1), (1, 1024)]
    assert lib.hit_thresholds([np.float64(0.45), 0.625, 1 / 3]) == [(9, 20), (5, 8), (1, 3)]      # (1 / 3 is within 1e-9 of its double)
    for bad, msg in (((0.3, 0.5, 0.7, 0.9, 1.0), '1 to 4'), ((), '1 to 4'), ((0.0,), r'\(0, 1\]'), ((1.5,), r'\(0, 1\]'), ((-0.5,), r'\(0, 1\]'),
                     ((0.3001234567,), 'denominator'), ((1 / 2048,), 'denominator'), (((1, 2048),), r'\(0, 1\]'), (((3, 2),), r'\(0, 1\]'),
                     (((0, 2),), r'\(0, 1\]'), (((1, 0),), 'pair'), (((1, 2, 3),), 'pair'), (((0.5, 2),), 'pair'), (0.5, 'sequence')):
        with pytest.raises(lib.HualError, match=msg):
            lib.hit_thresholds(bad)


def test_binding_checks_shapes_and_dtypes_without_a_gpu():
    from hual_amd import lib
    s = torch.zeros(3, 8)
    vl = torch.tensor([8, 8, 8], dtype=torch.int32)
    st = torch.zeros(3, 2, dtype=torch.int64)
    P = dict(starts=st, ends=st)
    for args, kw, msg in (((s.double(), s, vl), P, 'float32 logits'), ((s, s[:, :4], vl), P, r'both be \[B,T\]'), ((s, s, vl[:2]), P, 'B = 3 lengths'),
                          ((s, s, vl), dict(starts=st.int(), ends=st), 'starts must be'), ((s, s, vl), dict(starts=st, ends=st[:, :1]), 'ends must be'),
                          ((s, s, vl), dict(starts=st), 'given together'), ((s, s, vl), {}, 'nothing to do'),
                          ((s, s, vl), dict(best=True, reorder_by=0), 'need proposals'), ((s, s, vl), dict(P, reorder_by=3), 'reorder_by'),
                          ((s, s, vl), dict(P, reorder_by=-1), 'reorder_by'), ((s, s, vl), dict(P, thresholds=(0.3001234567,)), 'denominator'),
                          ((s, s, vl), dict(P, score=torch.zeros(3, 2, dtype=torch.float64)), 'score must be'),
                          ((s, s, vl), dict(P, out=(torch.zeros(3, 2, 2), None)), 'out tensors'),
                          ((s, s, vl), dict(P, out=(None, None)), 'out is'), ((s, s, vl), dict(P, best=True, out=(torch.zeros(3, 2, 3), None)), 'out is')):
        with pytest.raises(lib.HualError, match=msg):
            lib.span_hit_prob(*args, **kw)


# ---------------------------------------------------------------------------------------------------------------- the entry point
def test_hit_prob_is_declared_and_exported_at_abi_9():
    from hual_amd import build, lib
    build.build()
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'hual_seqpan.h')).read(), flags=re.S)
    assert re.search(r'\bint hual_span_hit_prob\s*\(', src)
    assert lib.ABI_VERSION == 9 and lib.load().hual_abi_version() == 9
    assert hasattr(ctypes.CDLL(lib.LIB_PATH), 'hual_span_hit_prob')
    assert callable(lib.span_hit_prob) and callable(lib.hit_thresholds)


def test_hit_prob_argument_errors_without_a_gpu():
    """every bad argument returns before any HIP call (the device pointers below are never dereferenced; the thresholds are host memory)"""
    from hual_amd import lib
    l = lib.load()
    p = ctypes.c_void_p(0x1000)
    good = dict(B=4, T=64, M=3, k=5, reorder_by=2)

    def thr_of(pairs):
        return (ctypes.c_int32 * (2 * len(pairs)))(*[x for nd in pairs for x in nd])

    def call(ins=(p, p, p), thr=thr_of(THR3), cands=(p, p), score=p, hp=p, best=(p, p, p), **kw):
        a = dict(good, **kw)
        return l.hual_span_hit_prob(*ins, a['B'], a['T'], thr, a['M'], a['k'], *cands, score, hp, a['reorder_by'], *best, None)
    for kw, msg in ((dict(k=-1), b'k <= 16'), (dict(k=17), b'k <= 16'), (dict(T=0), b'T <= 256'), (dict(T=257), b'T <= 256'), (dict(B=0), b'B >= 1'),
                    (dict(M=0), b'M <= 4'), (dict(M=5), b'M <= 4'), (dict(reorder_by=3), b'reorder_by < M'), (dict(reorder_by=-2), b'reorder_by < M'),
                    (dict(M=2, reorder_by=2), b'reorder_by < M'), (dict(k=0, reorder_by=0), b'reorder_by needs k'),
                    (dict(k=0, reorder_by=-1, best=(None, None, None)), b'nothing to do'),
                    (dict(thr=thr_of([(3, 10), (0, 2), (7, 10)])), b'num <= den'), (dict(thr=thr_of([(3, 10), (3, 2), (7, 10)])), b'num <= den'),
                    (dict(thr=thr_of([(3, 10), (1, 2), (1, 1025)])), b'num <= den'), (dict(thr=thr_of([(-1, 10), (1, 2), (7, 10)])), b'num <= den'),
                    (dict(best=(p, p, None)), b'together'), (dict(best=(None, p, p)), b'together'), (dict(best=(p, None, None)), b'together')):
        rc = call(**kw)
        assert rc == -1 and msg in l.hual_last_error() and b'hual_span_hit_prob' in l.hual_last_error(), (kw, l.hual_last_error())
    for bad in (dict(ins=(None, p, p)), dict(ins=(p, None, p)), dict(ins=(p, p, None)), dict(thr=None), dict(cands=(None, p)),
                dict(cands=(p, None)), dict(hp=None)):
        rc = call(**bad)
        assert rc == -1 and b'null pointer' in l.hual_last_error(), bad
    with pytest.raises(lib.HualError, match='M <= 4'):
        lib.check(call(M=5))
