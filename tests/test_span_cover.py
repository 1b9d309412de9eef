"""CPU: the enumeration reference of hual_span_hit_cover (tests/span_cover_ref.py) against the identities of the coverage and the
greedy theorem on an exhaustive optimum, the binding's argument checks and the entry point's host-side argument checks (no GPU needed)."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

import span_cover_ref as V
import span_hit_ref as H

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
    s, e, vl = _logits(8, T, 90 + T)
    thr = THR3 + [(1, 1)]
    rows, bayes = V.clips(s, e, vl, thr), H.bayes_ref(s, e, vl, thr)
    K = 5
    for b, (c, r) in enumerate(zip(rows, bayes)):
        assert c is not None and r is not None
        for m in range(len(thr)):
            spans, prob, best, gap = c.greedy(m, K, 0.0)
            # step 0 is the Bayes span of span_hit_ref, span and value
            assert spans[0] == (int(r['ii'][r['best'][m]]), int(r['jj'][r['best'][m]])) and abs(prob[0] - r['top'][m]) <= 1e-15
            assert (np.diff(prob) >= 0).all() and prob[-1] <= 1 + 1e-15 and (np.diff(best) <= 1e-15).all()       # gains do not grow: submodular
            taken = [x for x in spans if x[0] >= 0]
            assert len(set(taken)) == len(taken) and abs(best.sum() - prob[-1]) <= 1e-14
            # the coverage of a one-span set is its hit probability
            for a, z in taken[:2] + [(0, c.v - 1)]:
                flat = int(np.nonzero((r['ii'] == a) & (r['jj'] == z))[0][0])
                assert abs(c.coverage(m, [(a, z)])[0] - r['prob'][flat, m]) <= 1e-15
            # invalid slots add nothing, 0.0 before the first valid one
            cum = c.coverage(m, [(-1, -1), (3, 2), taken[0], (0, c.v), taken[0]])
            assert cum[0] == 0.0 and cum[1] == 0.0 and cum[2] == prob[0] and cum[3] == cum[2] and cum[4] == cum[2]
        # at (1, 1) a span hits only itself: the greedy set is the K heaviest spans, its coverage their sum
        spans, prob, _, _ = c.greedy(3, K, 0.0)
        order = np.argsort(-c.w, kind='stable')[:K]
        want = [(int(c.ii[x]), int(c.jj[x])) for x in order if c.w[x] > 0]
        assert [x for x in spans if x[0] >= 0] == want
        assert abs(prob[-1] - c.w[order].sum() / c.Z) <= 1e-15
    assert rows[1].greedy(0, 3, 0.0)[0] == [(0, 0), (-1, -1), (-1, -1)] and (rows[1].greedy(0, 3, 0.0)[1] == 1.0).all()      # v == 1


def test_reference_stops_and_dead_rows():
    s, e, vl = _logits(6, 10, 5)
    vl[:] = torch.tensor([10, 1, 0, 10, 6, 2])
    s[3, 4] = float('nan')                                        # inside the clip: the row is poisoned
    e[4, 8] = float('nan')                                        # beyond vlen = 6: not read
    rows = V.clips(s, e, vl, THR3)
    assert [r is None for r in rows] == [False, False, True, True, False, False]
    c = rows[0]
    spans, prob, best, _ = c.greedy(2, 16, 0.05)
    n = len(best)
    assert 1 <= n < 16 and (best > 0.05).all() and spans[n:] == [(-1, -1)] * (16 - n) and (prob[n:] == prob[n - 1]).all()
    assert c.gains(2, spans[:n]).max() <= 0.05
    spans, prob, best, _ = c.greedy(2, 4, 0.999)                   # step 0 already stops
    assert spans == [(-1, -1)] * 4 and (prob == 0.0).all() and len(best) == 0
    # a larger K extends a smaller one
    a, b = c.greedy(0, 3, 1e-6), c.greedy(0, 7, 1e-6)
    assert a[0] == b[0][:3] and (a[1] == b[1][:3]).all()


@pytest.mark.parametrize('T', [5, 7])
def test_greedy_against_the_exhaustive_optimum(T):
    """K = 2 over all pairs of spans on 16 seeded rows: greedy >= 1 - (1 - 1/2)^2 = 3/4 of the optimum (the theorem)"""
    g = torch.Generator().manual_seed(400 + T)
    s, e = torch.randn(16, T, generator=g) * 2, torch.randn(16, T, generator=g) * 2
    rows = V.clips(s, e, torch.full((16,), T, dtype=torch.int32), THR3)
    worst = 1.0
    for c in rows:
        spans_all = list(zip(c.ii.tolist(), c.jj.tolist()))
        for m in range(3):
            hit = c.hit(m)
            opt = max((c.w[hit[x] | hit[y]].sum() / c.Z for x, y in itertools.combinations(range(len(spans_all)), 2)))
            got = c.greedy(m, 2, 0.0)[1][-1]
            assert got <= opt + 1e-15 and got >= 0.75 * opt
            worst = min(worst, got / opt)
    print('T=%d K=2: worst greedy / optimum over 16 rows x 3 thresholds = %.4f (theorem: >= 0.75)' % (T, worst))


# ---------------------------------------------------------------------------------------------------------------- the binding
def test_binding_checks_shapes_and_dtypes_without_a_gpu():
    from hual_amd import lib
    s = torch.zeros(3, 8)
    vl = torch.tensor([8, 8, 8], dtype=torch.int32)
    st = torch.zeros(3, 2, dtype=torch.int64)
    P = dict(starts=st, ends=st)
    for args, kw, msg in (((s.double(), s, vl), P, 'float32 logits'), ((s, s[:, :4], vl), P, r'both be \[B,T\]'), ((s, s, vl[:2]), P, 'B = 3 lengths'),
                          ((s, s, vl), dict(starts=st.int(), ends=st), 'starts must be'), ((s, s, vl), dict(starts=st, ends=st[:, :1]), 'ends must be'),
                          ((s, s, vl), dict(starts=st), 'given together'), ((s, s, vl), {}, 'nothing to do'),
                          ((s, s, vl), dict(K=17), 'K <= 16'), ((s, s, vl), dict(K=-1), 'K <= 16'), ((s, s, vl), dict(K=2, min_gain=1.0), 'min_gain'),
                          ((s, s, vl), dict(K=2, min_gain=-0.1), 'min_gain'), ((s, s, vl), dict(P, thresholds=(0.3001234567,)), 'denominator'),
                          ((s, s, vl), dict(P, out=(torch.zeros(3, 2, 2), None)), 'out tensors'), ((s, s, vl), dict(P, out=(None, None)), 'out is'),
                          ((s, s, vl), dict(P, K=2, out=(torch.zeros(3, 2, 3), None)), 'out is'),
                          ((s, s, vl), dict(K=2, out=(None, (torch.zeros(3, 3, 2, dtype=torch.int64),) * 3)), 'out tensors')):
        with pytest.raises(lib.HualError, match=msg):
            lib.span_hit_cover(*args, **kw)


# ---------------------------------------------------------------------------------------------------------------- the entry point
def test_hit_cover_is_declared_and_exported_at_abi_9():
    from hual_amd import build, lib
    build.build()
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'hual_seqpan.h')).read(), flags=re.S)
    assert re.search(r'\bint hual_span_hit_cover\s*\(', src)
    assert lib.ABI_VERSION == 9 and lib.load().hual_abi_version() == 9
    assert hasattr(ctypes.CDLL(lib.LIB_PATH), 'hual_span_hit_cover')
    assert lib.load().hual_span_hit_cover.argtypes is not None and len(lib.load().hual_span_hit_cover.argtypes) == 17
    assert callable(lib.span_hit_cover)


def test_hit_cover_argument_errors_without_a_gpu():
    """every bad argument returns before any HIP call (the device pointers below are never dereferenced; the thresholds are host memory)"""
    from hual_amd import lib
    l = lib.load()
    p = ctypes.c_void_p(0x1000)
    good = dict(B=4, T=64, M=3, k=5, K=5, min_gain=1e-6)

    def thr_of(pairs):
        return (ctypes.c_int32 * (2 * len(pairs)))(*[x for nd in pairs for x in nd])

    def call(ins=(p, p, p), thr=thr_of(THR3), cands=(p, p), sp=p, cover=(p, p, p), **kw):
        a = dict(good, **kw)
        return l.hual_span_hit_cover(*ins, a['B'], a['T'], thr, a['M'], a['k'], *cands, sp, a['K'], a['min_gain'], *cover, None)
    for kw, msg in ((dict(k=-1), b'k <= 16'), (dict(k=17), b'k <= 16'), (dict(K=-1), b'K <= 16'), (dict(K=17), b'K <= 16'), (dict(T=0), b'T <= 256'),
                    (dict(T=257), b'T <= 256'), (dict(B=0), b'B >= 1'), (dict(M=0), b'M <= 4'), (dict(M=5), b'M <= 4'),
                    (dict(k=0, K=0), b'nothing to do'), (dict(k=0, K=0, cover=(None, None, None)), b'nothing to do'),
                    (dict(min_gain=-1e-3), b'min_gain < 1'), (dict(min_gain=1.0), b'min_gain < 1'), (dict(min_gain=float('nan')), b'min_gain < 1'),
                    (dict(thr=thr_of([(3, 10), (0, 2), (7, 10)])), b'num <= den'), (dict(thr=thr_of([(3, 10), (3, 2), (7, 10)])), b'num <= den'),
                    (dict(thr=thr_of([(3, 10), (1, 2), (1, 1025)])), b'num <= den'), (dict(thr=thr_of([(-1, 10), (1, 2), (7, 10)])), b'num <= den'),
                    (dict(cover=(p, p, None)), b'together'), (dict(cover=(None, p, p)), b'together'), (dict(K=0, cover=(p, None, None)), b'together')):
        rc = call(**kw)
        assert rc == -1 and msg in l.hual_last_error() and b'hual_span_hit_cover' in l.hual_last_error(), (kw, l.hual_last_error())
    for bad in (dict(ins=(None, p, p)), dict(ins=(p, None, p)), dict(ins=(p, p, None)), dict(thr=None), dict(cands=(None, p)),
                dict(cands=(p, None)), dict(sp=None), dict(cover=(None, None, None))):
        rc = call(**bad)
        assert rc == -1 and b'null pointer' in l.hual_last_error() and b'hual_span_hit_cover' in l.hual_last_error(), bad
    with pytest.raises(lib.HualError, match='K <= 16'):
        lib.check(call(K=17))
