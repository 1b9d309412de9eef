"""CPU: the float64 reference of hual_span_expected_iou (tests/span_conf_ref.py) against the properties of the quantity, the entry
point's host-side argument checks, its declaration and export, and the rank_by switch of al.update_labels (no GPU needed)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import span_conf_ref as C
import span_topk_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _logits(B, T, seed):
    g = torch.Generator().manual_seed(seed)
    s = (torch.randn(B, T, generator=g) * 2).clamp(-8, 8)
    e = (torch.randn(B, T, generator=g) * 2).clamp(-8, 8)
    vl = torch.randint(1, T + 1, (B,), generator=g, dtype=torch.int32)
    vl[0] = T
    vl[1] = 1
    return s, e, vl


def test_one_hot_distribution_gives_the_iou_with_that_span():
    T = 12
    for (i, j), (a, b) in (((2, 5), (2, 5)), ((2, 5), (4, 9)), ((0, 0), (3, 3)), ((1, 10), (0, 11)), ((7, 7), (0, 11))):
        ps, pe = np.zeros(T, dtype=np.float32), np.zeros(T, dtype=np.float32)
        ps[i], pe[j] = 1.0, 1.0
        got, H = C.distribution_ref(ps, pe, T, [(a, b)])
        inter = max(0, min(b, j) + 1 - max(a, i))
        assert got[0] == inter / ((b - a + 1) + (j - i + 1) - inter)
        assert H == 0.0
    # ... and this is the time IoU of the spans in seconds (data.index_to_time, al.calculate_iou)
    from hual_amd import al, data
    t0 = data.index_to_time((2, 5), T, 30.0)
    t1 = data.index_to_time((4, 9), T, 30.0)
    assert abs(C.span_iou(2, 5, np.array([4]), np.array([9]))[0] - al.calculate_iou(t0, t1)) < 1e-6


@pytest.mark.parametrize('T', [2, 9, 33])
def test_reference_ranges(T):
    s, e, vl = _logits(12, T, 40 + T)
    st, en, _ = R.span_topk_ref(s, e, vl, 5, nms_iou=0.5)
    ei, ent, alive = C.span_conf_ref(s, e, vl, st, en)
    assert alive.all()
    valid = st >= 0
    assert (ei[valid] >= 0).all() and (ei[valid] <= 1).all() and (ei[~valid] == -1.0).all()
    v = np.minimum(vl.numpy().astype(np.int64), T)
    assert (ent >= 0).all() and (ent <= np.log2(v * (v + 1) / 2) + 1e-12).all()
    # v == 1: the one span has probability 1
    assert ei[1, 0] == 1.0 and ent[1] == 0.0 and (st[1, 1:] == -1).all()
    # a proposal's own expected IoU is at least its probability (it overlaps itself fully)
    ps, pe, vv, _ = R.probabilities(s, e, vl)
    for b in range(12):
        ii, jj, w = C.span_weights(ps[b], pe[b], int(vv[b]))
        for q in np.nonzero(valid[b])[0]:
            assert ei[b, q] >= w[(ii == st[b, q]) & (jj == en[b, q])][0] / w.sum() - 1e-15


def test_reference_invalid_slots_and_dead_rows():
    s, e, vl = _logits(6, 10, 3)
    vl[:] = torch.tensor([10, 1, 0, 10, 6, 10])
    s[3, 4] = float('nan')                                        # inside the clip: the row is poisoned
    e[4, 8] = float('nan')                                        # beyond vlen = 6: not read
    st = np.array([[0, 5, -1, 3]] * 6, dtype=np.int64)
    en = np.array([[2, 4, -1, 9]] * 6, dtype=np.int64)            # (5, 4): a > b
    ei, ent, alive = C.span_conf_ref(s, e, vl, st, en)
    assert list(alive) == [True, True, False, False, True, True]
    assert (ei[2] == -1).all() and (ei[3] == -1).all() and ent[2] == -1 and ent[3] == -1
    assert ei[0, 0] > 0 and ei[0, 1] == -1 and ei[0, 2] == -1 and ei[0, 3] > 0
    assert (ei[1] == -1).all() and ent[1] == 0.0                  # vlen 1: (0, 2) and (3, 9) end beyond the clip
    assert ei[4, 0] > 0 and ei[4, 3] == -1                        # (3, 9) ends beyond vlen = 6
    assert list(C.stable_order(ei[0])) == ([0, 3, 1, 2] if ei[0, 0] > ei[0, 3] else [3, 0, 1, 2])
    assert list(C.stable_order([0.5, -1.0, 0.5, -1.0, 0.7])) == [4, 0, 2, 1, 3]


def test_expected_iou_is_declared_and_exported_at_abi_9():
    from hual_amd import build, lib
    build.build()
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'hual_seqpan.h')).read(), flags=re.S)
    assert re.search(r'\bint hual_span_expected_iou\s*\(', src)
    assert lib.ABI_VERSION == 9 and lib.load().hual_abi_version() == 9
    assert hasattr(ctypes.CDLL(lib.LIB_PATH), 'hual_span_expected_iou')
    assert callable(lib.span_expected_iou)


def test_expected_iou_argument_errors_without_a_gpu():
    """every bad argument returns before any HIP call (the pointers below are never dereferenced)"""
    from hual_amd import lib
    l = lib.load()
    p = ctypes.c_void_p(0x1000)
    good = dict(B=4, T=64, k=5)

    def call(ins=(p, p, p), cands=(p, p), score=p, ei=p, ent=p, reorder=1, **kw):
        a = dict(good, **kw)
        return l.hual_span_expected_iou(*ins, a['B'], a['T'], a['k'], *cands, score, ei, ent, reorder, None)
    for kw, msg in ((dict(k=0), b'k <= 16'), (dict(k=17), b'k <= 16'), (dict(T=0), b'T <= 256'), (dict(T=257), b'T <= 256'),
                    (dict(B=0), b'B >= 1')):
        rc = call(**kw)
        assert rc == -1 and msg in l.hual_last_error() and b'hual_span_expected_iou' in l.hual_last_error(), (kw, l.hual_last_error())
    for bad in (dict(ins=(None, p, p)), dict(ins=(p, None, p)), dict(ins=(p, p, None)), dict(cands=(None, p)), dict(cands=(p, None)),
                dict(ei=None)):
        rc = call(**bad)
        assert rc == -1 and b'null pointer' in l.hual_last_error(), bad
    with pytest.raises(lib.HualError, match='T <= 256'):
        lib.check(call(T=257))


def test_binding_checks_shapes_and_dtypes_without_a_gpu():
    from hual_amd import lib
    s = torch.zeros(3, 8)
    vl = torch.tensor([8, 8, 8], dtype=torch.int32)
    st = torch.zeros(3, 2, dtype=torch.int64)
    for args, kw, msg in (((s.double(), s, vl, st, st), {}, 'float32 logits'), ((s, s[:, :4], vl, st, st), {}, r'both be \[B,T\]'),
                          ((s, s, vl[:2], st, st), {}, 'B = 3 lengths'), ((s, s, vl, st.int(), st), {}, 'starts must be'),
                          ((s, s, vl, st, st[:, :1]), {}, 'ends must be'), ((s, s, vl, st.t().contiguous().t(), st), {}, 'starts must be'),
                          ((s, s, vl, st, st), dict(score=torch.zeros(3, 2, dtype=torch.float64)), 'score must be'),
                          ((s, s, vl, st, st), dict(out=(torch.zeros(3, 3), None)), 'out tensors')):
        with pytest.raises(lib.HualError, match=msg):
            lib.span_expected_iou(*args, **kw)


def test_rank_by_span_risk_needs_prop_conf():
    from hual_amd import al
    data = [['v0', 10.0, [1.0, 4.0], 'a b'], ['v1', 12.0, [2.0, 6.0], 'c d']]
    prop = [dict(vid='v0', v_len=8), dict(vid='v1', v_len=8, prop_conf=0.5)]
    with pytest.raises(ValueError, match='prop_conf'):
        al.update_labels([list(r) for r in data], data, prop, al.get_coff('charades', 1), rank_by='span_risk')
    with pytest.raises(ValueError, match='rank_by'):
        al.update_labels([list(r) for r in data], data, prop, al.get_coff('charades', 1), rank_by='nonsense')
    assert list(al.span_risk([dict(prop_conf=0.25), dict(prop_conf=1.0)])) == [0.75, 0.0]
    assert math.isclose(al.span_risk([dict(prop_conf=np.float32(0.1))])[0], 1.0 - float(np.float32(0.1)))
