"""CPU: hual_span_topk's host-side argument checks, the R@k helper and the reference's greedy NMS (no GPU needed)."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

import span_topk_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_topk_is_exported_at_abi_9():
    from hual_amd import build, lib
    build.build()
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'hual_seqpan.h')).read(), flags=re.S)
    assert re.search(r'\bint hual_span_topk\s*\(', src)
    assert lib.ABI_VERSION == 9 and lib.load().hual_abi_version() == 9
    assert hasattr(ctypes.CDLL(lib.LIB_PATH), 'hual_span_topk')


def test_topk_argument_errors_without_a_gpu():
    """every bad argument returns before any HIP call (the pointers below are never dereferenced)"""
    from hual_amd import lib
    l = lib.load()
    p = ctypes.c_void_p(0x1000)
    good = dict(B=4, T=64, k=5, max_len=0, nms_iou=0.5)

    def call(outs=(p, p, p), **kw):
        a = dict(good, **kw)
        return l.hual_span_topk(p, p, p, a['B'], a['T'], a['k'], a['max_len'], ctypes.c_float(a['nms_iou']), *outs, None)
    for kw, msg in ((dict(k=0), b'k <= 16'), (dict(k=17), b'k <= 16'), (dict(T=0), b'T <= 256'), (dict(T=257), b'T <= 256'),
                    (dict(nms_iou=0.0), b'nms_iou'), (dict(nms_iou=1.5), b'nms_iou'), (dict(nms_iou=float('nan')), b'nms_iou'),
                    (dict(max_len=-1), b'max_len'), (dict(B=0), b'B >= 1')):
        rc = call(**kw)
        assert rc == -1 and msg in l.hual_last_error(), (kw, l.hual_last_error())      # HUAL_ERR_INVALID
    for outs in ((None, p, p), (p, None, p), (p, p, None)):
        rc = call(outs=outs)
        assert rc < 0 and b'null pointer' in l.hual_last_error()
    rc = l.hual_span_topk(None, p, p, 4, 64, 5, 0, ctypes.c_float(0.5), p, p, p, None)
    assert rc < 0 and b'null pointer' in l.hual_last_error()
    with pytest.raises(lib.HualError, match='k <= 16'):
        lib.check(call(k=17))


def _records(n, seed):
    g = np.random.default_rng(seed)
    recs = []
    for _ in range(n):
        v = int(g.integers(4, 40))
        s = int(g.integers(0, v))
        e = int(g.integers(s, v))
        recs.append(dict(v_len=v, duration=float(g.uniform(5, 60)), s_ind=s, e_ind=e))
    return recs


def _proposals(recs, k, seed):
    g = np.random.default_rng(seed)
    st = np.full((len(recs), k), -1, dtype=np.int64)
    en = np.full((len(recs), k), -1, dtype=np.int64)
    for n, r in enumerate(recs):
        m = int(g.integers(1, k + 1)) if n % 3 else k        # every third row full, the others padded with -1
        for c in range(m):
            a = int(g.integers(0, r['v_len']))
            b = int(g.integers(a, r['v_len']))
            st[n, c], en[n, c] = a, b
    st[0, :], en[0, :] = recs[0]['s_ind'], recs[0]['e_ind']      # an exact hit
    return st, en


def test_recall_at_k_matches_the_scalar_loop():
    from hual_amd import al, data
    recs = _records(200, 1)
    st, en = _proposals(recs, 5, 2)
    best = []
    for r, srow, erow in zip(recs, st, en):
        gt = data.index_to_time([r['s_ind'], r['e_ind']], r['v_len'], r['duration'])
        ious = [0.0 if s < 0 else al.calculate_iou(data.index_to_time([s, e], r['v_len'], r['duration']), gt) for s, e in zip(srow, erow)]
        best.append(max(ious))
    want = tuple(float(np.mean(np.asarray(best) >= t) * 100.0) for t in (0.3, 0.5, 0.7))
    assert al.recall_at_k(recs, st, en) == want
    assert al.recall_at_k(recs, st, en, thresholds=(0.1,)) == (float(np.mean(np.asarray(best) >= 0.1) * 100.0),)
    # R@k never falls as columns are added
    prev = (0.0, 0.0, 0.0)
    for c in range(1, 6):
        cur = al.recall_at_k(recs, st[:, :c], en[:, :c])
        assert all(a >= b for a, b in zip(cur, prev))
        prev = cur
    assert prev == want


def test_recall_at_1_is_iou_metrics():
    from hual_amd import al
    recs = _records(300, 3)
    st, en = _proposals(recs, 4, 4)
    assert (st[:, 0] >= 0).all()
    assert al.recall_at_k(recs, st[:, :1], en[:, :1]) == al.iou_metrics(al.ious_of_spans(recs, st[:, 0], en[:, 0]))[:3]
    assert al.recall_at_k(recs, st[:, 0], en[:, 0]) == al.iou_metrics(al.ious_of_spans(recs, st[:, 0], en[:, 0]))[:3]


def _brute_force(ps, pe, v, k, max_len, nms_iou):
    """the contract written out plainly: every pair, python's sort, the classic NMS loop"""
    f32 = np.float32
    cands = [(-float(f32(ps[i]) * f32(pe[j])), i * 256 + j, i, j) for i in range(v) for j in range(i, v) if max_len <= 0 or j - i < max_len]
    cands.sort()
    picked = []
    for negs, _, i, j in cands:
        ok = True
        for (a, b) in picked:
            inter = max(0, min(b, j) + 1 - max(a, i))
            union = (b - a + 1) + (j - i + 1) - inter
            if f32(inter) >= f32(nms_iou) * f32(union):
                ok = False
                break
        if ok:
            picked.append((i, j))
            if len(picked) == k:
                break
    return picked


@pytest.mark.parametrize('T', [1, 2, 5, 9])
def test_reference_nms_is_the_brute_force_definition(T):
    g = torch.Generator().manual_seed(T)
    B = 24
    s = torch.randn(B, T, generator=g) * 2
    e = torch.randn(B, T, generator=g) * 2
    s[:4] = 0.25                                                  # plateaus: every candidate of a row ties with its neighbours
    e[2:6, :] = e[2:6, :1]
    vl = torch.randint(0, T + 2, (B,), generator=g)               # (0 = empty clip, T + 1 reads as T)
    for k, ml, iou in itertools.product((1, 3, 16), (0, 2), (1.0, 0.5, 0.3)):
        st, en, sc = R.span_topk_ref(s, e, vl, k, max_len=ml, nms_iou=iou)
        ps, pe, v, _ = R.probabilities(s, e, vl)
        for b in range(B):
            want = _brute_force(ps[b], pe[b], int(v[b]), k, ml, iou)
            got = [(int(i), int(j)) for i, j in zip(st[b], en[b]) if i >= 0]
            assert got == want, (b, k, ml, iou)
            assert (st[b, len(got):] == -1).all() and (en[b, len(got):] == -1).all() and (sc[b, len(got):] == -1.0).all()
            if got:
                assert all(sc[b, r] == np.float32(ps[b, i]) * np.float32(pe[b, j]) for r, (i, j) in enumerate(got))


def test_reference_nan_row_and_top1_of_a_plateau():
    s = torch.zeros(3, 8)
    e = torch.zeros(3, 8)
    s[1, 2] = float('nan')                                        # inside the clip: the row is poisoned
    s[2, 6] = float('nan')                                        # beyond vlen: not read
    st, en, sc = R.span_topk_ref(s, e, torch.tensor([8, 8, 5]), 4, nms_iou=1.0)
    assert (st[1] == -1).all() and (sc[1] == -1.0).all()
    # a flat plateau: every pair has the same score, so the order is the key order (0,0), (0,1), ...
    assert [(int(a), int(b)) for a, b in zip(st[0], en[0])] == [(0, 0), (0, 1), (0, 2), (0, 3)]
    assert [(int(a), int(b)) for a, b in zip(st[2], en[2])] == [(0, 0), (0, 1), (0, 2), (0, 3)]
    ps, pe, v, _ = R.probabilities(s, e, torch.tensor([8, 8, 5]))
    assert not R.non_product_tie(ps[0], pe[0], 8)
