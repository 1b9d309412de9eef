"""GPU: hual_span_hit_prob (hit probability of proposals at exact rational IoU thresholds, their order by one of them, the Bayes span
of each threshold) against the float64 enumeration of its contract (tests/span_hit_ref.py), its edge rows, its in-place reorder,
repeat launches and graph capture, and where it lands: Runner.evaluate(rerank='hit_prob', bayes_spans=True).

The bar: 1e-6 absolute on every probability, the project's bar for float64-accumulated probabilities stored as float32
(hual_span_expected_iou, hual_al_query).  The kernel sums exact float64 products of float32 probabilities; its prefix differences and
the order of its sums are worth a few 2^-53, and the one float32 rounding of a value <= 1 is at most 2^-25 = 3e-8.
Span equality with the enumeration's first maximiser is asked wherever the enumeration's runner-up lies at least 1e-5 (ten bars) below
its maximum; the other (row, threshold) cases may be at most 5 % - asserted on the enumeration alone, before any device value is read."""
import functools

import numpy as np
import pytest
import torch

import span_conf_ref as C
import span_hit_ref as H
import span_topk_ref as R
from span_clip_util import _pads_intact, _sentinel, _task, _videos

pytestmark = pytest.mark.gpu

BAR, GAP, EXEMPT = 1e-6, 1e-5, 0.05
B, TS, KS, SCALES, SEED = 8, (2, 33, 70, 256), (1, 5, 16), (1, 3), 7
# the launches of every case and the columns of the one reference they are checked against
REF_THR = [(1, 1024), (3, 10), (1, 2), (7, 10), (1, 1)]
LAUNCHES = {'three': [(3, 10), (1, 2), (7, 10)], 'one': [(1, 1)], 'four': [(1, 1024), (3, 10), (1, 2), (7, 10)]}
COLS = {name: [REF_THR.index(t) for t in thr] for name, thr in LAUNCHES.items()}


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def inputs(T, scale, seed=SEED):
    """logits scale * N(0, 1); lengths T, T - 1 (255 at T = 256), 1, 2 and random ones"""
    g = torch.Generator().manual_seed(1000 * seed + 10 * T + scale)
    s, e = torch.randn(B, T, generator=g) * scale, torch.randn(B, T, generator=g) * scale
    vl = torch.randint(1, T + 1, (B,), generator=g, dtype=torch.int32)
    vl[0], vl[1], vl[2], vl[3] = T, max(1, T - 1), 1, min(T, 2)
    return s, e, vl


def _run(dev, s, e, vl, thr, st=None, en=None, sc=None, reorder_by=None, best=False):
    """one launch into sentinel-filled outputs; -> numpy (hit_prob [B,k,M] or None, (best_start, best_end, best_prob) or None) after
    checking the memory around them and that every element was written"""
    from hual_amd import lib
    n, M = s.shape[0], len(thr)
    outs, guards = [None, None], []
    if st is not None:
        hp, whole, pad = _sentinel((n, st.shape[1], M), torch.float32, dev, 777.0)
        outs[0] = hp
        guards.append((hp, whole, pad, 777.0))
    if best:
        trio = []
        for dt, val in ((torch.int64, -99), (torch.int64, -99), (torch.float32, 777.0)):
            x, whole, pad = _sentinel((n, M), dt, dev, val)
            trio.append(x)
            guards.append((x, whole, pad, val))
        outs[1] = tuple(trio)
    got = lib.span_hit_prob(s, e, vl, thr, starts=st, ends=en, score=sc, reorder_by=reorder_by, best=best, out=tuple(outs))
    assert got[0] is outs[0] and (got[1] is None) == (not best)
    torch.cuda.synchronize()
    for x, whole, pad, val in guards:
        assert _pads_intact(whole, pad, val)
        assert not bool((x == val).any())                              # every element was written
    return (None if outs[0] is None else outs[0].cpu().numpy()), (tuple(x.cpu().numpy() for x in outs[1]) if best else None)


_CASES = {}


def case(dev, T, k, scale):
    """inputs, the candidates of lib.span_topk at nms_iou 0.5 with three hand-placed invalid slots, the enumeration and the device values
    of the three launches without reorder: computed once"""
    key = (T, k, scale)
    if key not in _CASES:
        from hual_amd import lib
        s, e, vl = inputs(T, scale)
        sd, ed, vd = s.to(dev), e.to(dev), vl.to(dev)
        st, en, sc = lib.span_topk(sd, ed, vd, k, nms_iou=0.5)
        st[4, k // 2], en[4, k // 2] = -1, -1                         # no proposal
        st[5, k - 1], en[5, k - 1] = 1, 0                             # a > b
        en[6, 0] = T                                                  # b >= v
        keep = (st.clone(), en.clone(), sc.clone())
        got = {name: _run(dev, sd, ed, vd, thr, st, en, sc)[0] for name, thr in LAUNCHES.items()}
        for a, b in zip((st, en, sc), keep):                          # reorder_by None: the candidate arrays are only read
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        sth, enh = st.cpu().numpy(), en.cpu().numpy()
        ref, alive = H.span_hit_ref(s, e, vl, sth, enh, REF_THR)
        _CASES[key] = dict(dev=(sd, ed, vd, st, en, sc), st=sth, en=enh, sc=sc.cpu().numpy(), got=got, ref=ref, alive=alive)
    return _CASES[key]


# ---------------------------------------------------------------------------------------------------------------- 1. values
@pytest.mark.parametrize('scale', SCALES)
@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('T', TS)
def test_values_against_the_enumeration(dev, T, k, scale):
    c = case(dev, T, k, scale)
    assert c['alive'].all()
    vl = np.minimum(inputs(T, scale)[2].numpy(), T)
    valid = (c['st'] >= 0) & (c['st'] <= c['en']) & (c['en'] < vl[:, None])
    assert not valid[4, k // 2] and not valid[5, k - 1] and not valid[6, 0] and valid[:4, 0].all()
    worst = 0.0
    for name, cols in COLS.items():
        got, ref = c['got'][name], c['ref'][:, :, cols]
        assert got.shape == (B, k, len(cols))
        assert (got[~valid] == -1.0).all() and (ref[~valid] == -1.0).all()
        assert (got[valid] >= 0).all() and (got[valid] <= 1).all()
        d = float(np.abs(got[valid].astype(np.float64) - ref[valid]).max())
        worst = max(worst, d)
        assert d <= BAR, (name, d)
        # a threshold's column does not depend on the launch it is part of
        for other, ocols in COLS.items():
            for x, col in enumerate(cols):
                if col in ocols:
                    assert (got[:, :, x].view(np.int32) == c['got'][other][:, :, ocols.index(col)].view(np.int32)).all()
    print('T=%d k=%d scale=%d: max |hit_prob - enumeration| = %.3e (bar %.0e)' % (T, k, scale, worst, BAR))
    four = c['got']['four'][valid].astype(np.float64)
    assert (np.diff(four, axis=1) <= BAR).all()                       # columns do not increase with the threshold
    row = c['got']['three'][2]                                        # v == 1: (0, 0) with probability exactly 1
    assert valid[2, 0] and (c['st'][2, 0], c['en'][2, 0]) == (0, 0) and (row[0] == 1.0).all() and (row[1:] == -1.0).all()


# ---------------------------------------------------------------------------------------------------------------- 2. Bayes spans
@functools.lru_cache(maxsize=None)
def bayes_rows(T, scale):
    s, e, vl = inputs(T, scale)
    return H.bayes_ref(s, e, vl, REF_THR)


def _best(dev, T, scale):
    s, e, vl = inputs(T, scale)
    sd, ed, vd = s.to(dev), e.to(dev), vl.to(dev)
    return {name: _run(dev, sd, ed, vd, thr, best=True)[1] for name, thr in LAUNCHES.items()}


@pytest.mark.parametrize('scale', SCALES)
@pytest.mark.parametrize('T', (2, 33, 70))
def test_bayes_span_against_the_full_enumeration(dev, T, scale):
    rows = bayes_rows(T, scale)
    assert all(r is not None for r in rows)
    # on the enumeration alone: the (row, threshold) cases too close to call are few
    gaps = np.array([r['gap'] for r in rows])
    close = gaps < GAP
    three, exact = COLS['three'], REF_THR.index((1, 1))
    n_close = int(close[:, three].sum())
    print('T=%d scale=%d: %d of %d (row, threshold) cases have a runner-up within %.0e of the maximum' % (T, scale, n_close, B * 3, GAP))
    assert n_close <= EXEMPT * B * 3
    assert (gaps[:, exact] > 1e-12).all()                             # no two spans of a row are equally probable
    got = _best(dev, T, scale)
    worst = 0.0
    for name, cols in COLS.items():
        bs, be, bp = got[name]
        assert bs.shape == be.shape == bp.shape == (B, len(cols))
        for b, r in enumerate(rows):
            n = len(r['ii'])
            for x, col in enumerate(cols):
                a, z = int(bs[b, x]), int(be[b, x])
                assert 0 <= a <= z and n == (r['jj'].max() + 1) * (r['jj'].max() + 2) // 2 and z <= r['jj'].max()
                flat = int(np.nonzero((r['ii'] == a) & (r['jj'] == z))[0][0])
                d1 = abs(float(bp[b, x]) - r['prob'][flat, col])      # (1) the reported probability is that of the reported span
                d2 = r['top'][col] - r['prob'][flat, col]             # (2) which is the enumeration's maximum
                worst = max(worst, d1, d2)
                assert d1 <= BAR and d2 <= BAR, (name, b, col, d1, d2)
                # (3) and the enumeration's first maximiser.  (At 1 / 1024 - any overlap - the long spans all but tie: values only.)
                if (col in three and not close[b, col]) or col == exact:
                    assert flat == r['best'][col], (name, b, col, (a, z), (r['ii'][r['best'][col]], r['jj'][r['best'][col]]))
    print('T=%d scale=%d: max distance of best_prob from the enumeration %.3e (bar %.0e)' % (T, scale, worst, BAR))
    # identities on the kernel's output: 1 / 1 is the most probable span, columns do not increase, v == 1 is (0, 0) exactly
    ps, pe, v, _ = R.probabilities(*inputs(T, scale))
    bs, be, bp = got['one']
    for b in range(B):
        ii, jj, w = C.span_weights(ps[b], pe[b], int(v[b]))
        assert (int(bs[b, 0]), int(be[b, 0])) == (int(ii[np.argmax(w)]), int(jj[np.argmax(w)]))
    assert (np.diff(got['four'][2].astype(np.float64), axis=1) <= BAR).all()
    for name in LAUNCHES:
        assert (got[name][0][2] == 0).all() and (got[name][1][2] == 0).all() and (got[name][2][2] == 1.0).all()
    # the same bits with the proposals scored in the same launch, and the proposals' with the Bayes spans searched
    c = case(dev, T, 5, scale)
    sd, ed, vd, st, en, sc = c['dev']
    hp, both = _run(dev, sd, ed, vd, LAUNCHES['three'], st, en, sc, best=True)
    assert (hp.view(np.int32) == c['got']['three'].view(np.int32)).all()
    for x, y in zip(both, got['three']):
        assert (x.view(np.int32) == y.view(np.int32)).all()


@pytest.mark.parametrize('scale', SCALES)
def test_bayes_span_at_256_frames(dev, scale):
    """the square enumeration is too slow here: the reported probability is that of the reported span, and no span of a broad field -
    the mode, the 16 proposals of hual_span_topk, the best of them by expected IoU, 2,000 random spans per row - does better"""
    from hual_amd import lib
    T, thr = 256, LAUNCHES['three']
    s, e, vl = inputs(T, scale)
    sd, ed, vd = s.to(dev), e.to(dev), vl.to(dev)
    bs, be, bp = _run(dev, sd, ed, vd, thr, best=True)[1]
    mode = lib.span_topk(sd, ed, vd, 1)
    st, en, sc = lib.span_topk(sd, ed, vd, 16, nms_iou=0.5)
    lib.span_expected_iou(sd, ed, vd, st, en, score=sc, reorder=True)
    field = np.concatenate([np.stack([mode[0].cpu().numpy(), mode[1].cpu().numpy()], axis=2),
                            np.stack([st.cpu().numpy(), en.cpu().numpy()], axis=2)], axis=1)              # [B, 17, 2]; slot 1: best expected IoU
    ps, pe, v, _ = R.probabilities(s, e, vl)
    g = np.random.default_rng(100 * SEED + scale)
    worst1, worst2 = 0.0, -1.0
    for b in range(4):                                                # v = 256, 255, 1, 2: the long rows cost the reference a second each
        n = int(v[b])
        x = g.integers(0, n, size=(2000, 2))
        cands = np.concatenate([np.stack([bs[b], be[b]], axis=1), field[b], np.sort(x, axis=1)])
        ref = H.clip_hit_prob(ps[b], pe[b], n, cands, thr)
        own = ref[np.arange(3), np.arange(3)]                         # the reference value of each threshold's own span
        assert (own >= 0).all()
        d1 = float(np.abs(bp[b].astype(np.float64) - own).max())
        d2 = float((ref[3:].max(axis=0) - own).max())
        worst1, worst2 = max(worst1, d1), max(worst2, d2)
        assert d1 <= BAR and d2 <= BAR, (b, d1, d2)
    print('T=256 scale=%d: max |best_prob - enumeration| = %.3e, best field span above the kernel\'s by at most %.3e (bar %.0e)' % (scale, worst1, worst2, BAR))
    assert (bs[2] == 0).all() and (be[2] == 0).all() and (bp[2] == 1.0).all()


# ---------------------------------------------------------------------------------------------------------------- 3. edge rows
def test_edge_rows_and_untouched_memory(dev):
    T, k, thr = 33, 5, LAUNCHES['three']
    s, e, vl = (x.clone() for x in inputs(T, 1))
    vl[:] = torch.tensor([T, 20, 1, 0, T, 20, T + 9, -2])             # row 3 empty; row 6 read as T; row 7 empty
    s[4, 3] = float('nan')                                        # a NaN logit inside the clip: row 4 is poisoned
    e[5, 30] = float('nan')                                       # beyond vlen = 20: not read
    s[1, :], e[1, :] = -200.0, -200.0                             # row 1 (vlen 20): the start certainly last, the end certainly first -
    s[1, 19], e[1, 0] = 200.0, 200.0                              # every weight with i <= j is exactly 0, Z = 0: as a poisoned row
    s[0, 5] = float('inf')                                        # row 0: an infinite logit makes the probabilities NaN, Z with them
    st = torch.tensor([[2, 9, -1, 0, 5]] * B, dtype=torch.int64)
    en = torch.tensor([[6, 4, -1, T - 1, 20]] * B, dtype=torch.int64)           # (9, 4): a > b; (-1, -1): no proposal
    st[2], en[2] = torch.tensor([0, 0, -1, 1, 0]), torch.tensor([0, 0, -1, 1, 1])      # v = 1: (0, 0) twice, the rest beyond the clip
    st[6], en[6] = torch.tensor([-1, 9, 4, 3, -5]), torch.tensor([4, 4, T, -1, -5])    # every slot invalid
    en[5, 3] = 19                                                 # row 5 (vlen 20): (2, 6) and the whole clip (0, 19) are valid
    sc = torch.arange(B * k, dtype=torch.float32).view(B, k)
    sd, ed, vd = s.to(dev), e.to(dev), vl.to(dev)
    ref, alive = H.span_hit_ref(s, e, vl, st.numpy(), en.numpy(), thr)
    dead = [0, 1, 3, 4, 7]
    assert list(np.nonzero(~alive)[0]) == dead
    rows = H.bayes_ref(s, e, vl, thr)
    for reorder_by in (None, 1):
        std, st_w, p0 = _sentinel((B, k), torch.int64, dev, -99)
        end, en_w, _ = _sentinel((B, k), torch.int64, dev, -99)
        scd, sc_w, _ = _sentinel((B, k), torch.float32, dev, -99.0)
        std.copy_(st), end.copy_(en), scd.copy_(sc)
        hp, (bs, be, bp) = _run(dev, sd, ed, vd, thr, std, end, scd, reorder_by=reorder_by, best=True)
        assert _pads_intact(st_w, p0, -99) and _pads_intact(en_w, p0, -99) and _pads_intact(sc_w, p0, -99.0)
        sth, enh, sch = std.cpu().numpy(), end.cpu().numpy(), scd.cpu().numpy()
        for b in dead:                                                # all -1 and never reordered
            assert (hp[b] == -1.0).all() and (bs[b] == -1).all() and (be[b] == -1).all() and (bp[b] == -1.0).all()
            assert (sth[b] == st[b].numpy()).all() and (enh[b] == en[b].numpy()).all() and (sch[b] == sc[b].numpy()).all()
        assert (hp[6] == -1.0).all() and (bs[6] >= 0).all() and (bp[6] > 0).all()       # all slots invalid: the Bayes spans do not mind
        assert (sth[6] == st[6].numpy()).all() and (enh[6] == en[6].numpy()).all()
        assert (bs[2] == 0).all() and (be[2] == 0).all() and (bp[2] == 1.0).all()        # v = 1
        assert sorted(hp[2, :, 0]) == [-1.0, -1.0, -1.0, 1.0, 1.0]
        for b in (2, 5, 6):                                           # the Bayes spans of the live rows (row 5 reads 20 frames only)
            r = rows[b]
            for m in range(3):
                flat = int(np.nonzero((r['ii'] == bs[b, m]) & (r['jj'] == be[b, m]))[0][0])
                assert abs(float(bp[b, m]) - r['prob'][flat, m]) <= BAR and r['top'][m] - r['prob'][flat, m] <= BAR
            assert r['jj'].max() == (0, 19, T - 1)[(2, 5, 6).index(b)]
        if reorder_by is None:
            assert (sth == st.numpy()).all() and (enh == en.numpy()).all() and (sch.view(np.int32) == sc.numpy().view(np.int32)).all()
            assert ((hp == -1.0) == (ref == -1.0)).all()
            assert (hp[5, 1] == -1.0).all() and (hp[5, 2] == -1.0).all() and (hp[5, 4] == -1.0).all()         # a > b, none, b >= vlen = 20
            ok = ref >= 0
            assert ok[5, 0].all() and ok[5, 3].all() and float(np.abs(hp[ok] - ref[ok]).max()) <= BAR
        else:
            assert ref[5, 3, reorder_by] > ref[5, 0, reorder_by] + 10 * BAR                  # row 5: the whole clip goes first
            for b in np.nonzero(alive)[0]:
                o = H.stable_order(ref[b][:, reorder_by])
                assert b != 5 or list(o) == [3, 0, 1, 2, 4]
                assert (sth[b] == st[b].numpy()[o]).all() and (enh[b] == en[b].numpy()[o]).all() and (sch[b] == sc[b].numpy()[o]).all()
                assert ((hp[b] == -1.0) == (ref[b][o] == -1.0)).all()
    # proposals only (best_* NULL) and the Bayes spans only (k = 0): the same bits as together
    hp1, none = _run(dev, sd, ed, vd, thr, st.to(dev), en.to(dev), sc.to(dev))
    none2, best2 = _run(dev, sd, ed, vd, thr, best=True)
    hp0, best0 = _run(dev, sd, ed, vd, thr, st.to(dev), en.to(dev), sc.to(dev), best=True)
    assert none is None and none2 is None and (hp1.view(np.int32) == hp0.view(np.int32)).all()
    for x, y in zip(best2, best0):
        assert (x.view(np.int32) == y.view(np.int32)).all()


# ---------------------------------------------------------------------------------------------------------------- 4. reorder
@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('T', TS)
def test_reorder_is_a_stable_sort_by_one_column(dev, T, k):
    scale, thr = 3, LAUNCHES['three']
    c = case(dev, T, k, scale)
    sd, ed, vd, st, en, sc = c['dev']
    base, ref = c['got']['three'], c['ref'][:, :, COLS['three']]
    compared = 0
    for m in range(3):
        st2, en2, sc2 = st.clone(), en.clone(), sc.clone()
        hp = _run(dev, sd, ed, vd, thr, st2, en2, sc2, reorder_by=m)[0]
        for b in range(B):
            o = H.stable_order(base[b][:, m])                         # host stable sort of the device values without reorder
            assert (st2[b].cpu().numpy() == c['st'][b][o]).all() and (en2[b].cpu().numpy() == c['en'][b][o]).all()
            assert (sc2[b].cpu().numpy().view(np.int32) == c['sc'][b][o].view(np.int32)).all()
            assert (hp[b].view(np.int32) == base[b][o].view(np.int32)).all()              # all M columns, alike
            # ... which is the enumeration's order wherever its values in this column are ten bars apart
            vals = np.sort(ref[b][:, m][ref[b][:, m] >= 0])
            if len(vals) < 2 or np.diff(vals).min() > 10 * BAR:
                assert (o == H.stable_order(ref[b][:, m])).all()
                compared += 1
    print('T=%d k=%d: %d of %d (row, column) orders compared with the enumeration\'s' % (T, k, compared, 3 * B))
    assert compared >= 3 * B // 2
    # reorder_by None leaves the proposals bit-equal: asserted where the case is built (case())


# ---------------------------------------------------------------------------------------------------------------- 5. repeat, capture
def test_second_launch_and_captured_graph(dev):
    from hual_amd import lib
    T, k, thr = 70, 5, LAUNCHES['three']
    c = case(dev, T, k, 1)
    sd, ed, vd, st, en, sc = c['dev']

    def outs():
        return (torch.empty(B, k, 3, dtype=torch.float32, device=dev),
                (torch.empty(B, 3, dtype=torch.int64, device=dev), torch.empty(B, 3, dtype=torch.int64, device=dev),
                 torch.empty(B, 3, dtype=torch.float32, device=dev)))

    def flat(work, out):
        return tuple(work) + (out[0],) + tuple(out[1])
    eager = (st.clone(), en.clone(), sc.clone())
    want = outs()
    lib.span_hit_prob(sd, ed, vd, thr, eager[0], eager[1], score=eager[2], reorder_by=2, best=True, out=want)
    again = (st.clone(), en.clone(), sc.clone())
    got = outs()
    lib.span_hit_prob(sd, ed, vd, thr, again[0], again[1], score=again[2], reorder_by=2, best=True, out=got)
    torch.cuda.synchronize()
    for a, b in zip(flat(again, got), flat(eager, want)):            # a second launch: equal bits
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert not torch.equal(eager[0], st)                              # (the reorder moved something)
    work, out = (st.clone(), en.clone(), sc.clone()), outs()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        lib.span_hit_prob(sd, ed, vd, thr, work[0].clone(), work[1].clone(), score=work[2].clone(), reorder_by=2, best=True, out=outs())      # (warm-up)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        lib.span_hit_prob(sd, ed, vd, thr, work[0], work[1], score=work[2], reorder_by=2, best=True, out=out)
    for _ in range(2):
        for w, src in zip(work, (st, en, sc)):
            w.copy_(src)
        for o in flat((), out):
            o.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(flat(work, out), flat(eager, want)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------- 6. evaluation
def test_hit_prob_evaluation(tmp_path, monkeypatch):
    from hual_amd import al, lib
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
    plain, props0 = r.evaluate(k=k, nms_iou=0.5, return_proposals=True)
    # the default call: the keys, values and tuples of before, and no launch of the new entry point
    assert sorted(plain) == sorted(['R1@0.3', 'R1@0.5', 'R1@0.7', 'R5@0.3', 'R5@0.5', 'R5@0.7', 'mIoU'])
    assert all(len(x) == 3 for p in props0 for x in p)
    with monkeypatch.context() as mp:
        def unavailable(*a, **kw):
            raise AssertionError('the default evaluation launched hual_span_hit_prob')
        mp.setattr(lib, 'span_hit_prob', unavailable)
        assert r.evaluate(k=k, nms_iou=0.5) == plain
        assert r.evaluate(k=k, nms_iou=0.5, rerank=None, hit_iou=0.5, bayes_spans=False) == plain
        ei = r.evaluate(k=k, nms_iou=0.5, rerank='expected_iou')
        assert sorted(ei) == sorted(list(plain) + ['conf', 'span_entropy'])
    ds = r.test_set
    for hit_iou in (0.7, 0.5):
        n_lines = len(lines)
        res, props = r.evaluate(k=k, nms_iou=0.5, rerank='hit_prob', hit_iou=hit_iou, return_proposals=True)
        tag = '@%g' % hit_iou
        assert sorted(res) == sorted(list(plain) + ['hit_conf', 'ece' + tag, 'brier' + tag])
        assert any('hit probability' in l for l in lines[n_lines:])
        for th in ('0.3', '0.5', '0.7'):
            assert res['R5@' + th] == plain['R5@' + th]               # the same set of proposals
        assert all(np.isfinite(res[x]) for x in ('hit_conf', 'ece' + tag, 'brier' + tag))
        assert 0 <= res['hit_conf'] <= 1 and 0 <= res['ece' + tag] <= 1 and 0 <= res['brier' + tag] <= 1
        first, conf, S, E = [], [], [], []
        for i, (p0, p) in enumerate(zip(props0, props)):
            assert len(p) == len(p0) == k and all(len(x) == 4 for x in p)
            assert sorted(x[:3] for x in p) == sorted(p0)             # a permutation of the plain proposals, scores carried along
            vals = [x[3] for x in p]
            assert all(0.0 <= x <= 1.0 for x in vals) and vals == sorted(vals, reverse=True)      # slot 0: the maximal hit probability
            conf.append(vals[0])
        # per clip: the enumeration on the logits of the same forward; the metrics recomputed from the returned proposals
        for lo in range(0, len(ds), r.batch_size):
            sel = np.arange(lo, min(len(ds), lo + r.batch_size))
            f = ds.assemble(sel, labels=False, min_chars=4)
            o = r.model.forward(f['video'], f['video_seq_len'], f['word_ids'], f['char_ids'], drop_rate=0.0)
            sl, el, vl = o['start_logits'].cpu(), o['end_logits'].cpu(), f['video_seq_len'].cpu()
            st, en, sc = R.span_topk_ref(sl, el, vl, k, nms_iou=0.5)
            ref, alive = H.span_hit_ref(sl, el, vl, st, en, lib.hit_thresholds((hit_iou,)))
            assert alive.all()
            from hual_amd import data
            for row, i in enumerate(sel):
                rec = ds.records[i]
                back = {tuple(float(x) for x in data.index_to_time((a, b), rec['v_len'], rec['duration'])): (a, b, v[0])
                        for a, b, v in zip(st[row], en[row], ref[row])}
                for x in props[i]:
                    assert abs(x[3] - back[x[:2]][2]) <= BAR
                S.append(back[props[i][0][:2]][0])
                E.append(back[props[i][0][:2]][1])
        ious = np.asarray(al.ious_of_spans(ds.records, S, E), dtype=np.float64)
        assert (res['R1@0.3'], res['R1@0.5'], res['R1@0.7'], res['mIoU']) == al.iou_metrics(ious)
        cal = al.hit_calibration(np.asarray(conf, dtype=np.float32), ious >= hit_iou)
        assert res['ece' + tag] == cal['ece'] and res['brier' + tag] == cal['brier']
        assert res['hit_conf'] == float(np.mean(np.asarray(conf, dtype=np.float32), dtype=np.float64))
    # the Bayes spans: R@1 of each threshold's own span, recomputed on the host from a direct launch on the same logits
    res = r.evaluate(k=k, nms_iou=0.5, bayes_spans=True)
    keys = ['R1_bayes@0.3', 'R1_bayes@0.5', 'R1_bayes@0.7', 'bayes_conf@0.3', 'bayes_conf@0.5', 'bayes_conf@0.7']
    assert sorted(res) == sorted(list(plain) + keys) and all(res[x] == plain[x] for x in plain)
    BS, BE, BP = [], [], []
    for lo in range(0, len(ds), r.batch_size):
        sel = np.arange(lo, min(len(ds), lo + r.batch_size))
        f = ds.assemble(sel, labels=False, min_chars=4)
        o = r.model.forward(f['video'], f['video_seq_len'], f['word_ids'], f['char_ids'], drop_rate=0.0)
        _, (bs, be, bp) = lib.span_hit_prob(o['start_logits'], o['end_logits'], f['video_seq_len'], (0.3, 0.5, 0.7), best=True)
        BS.append(bs.cpu().numpy()), BE.append(be.cpu().numpy()), BP.append(bp.cpu().numpy())
    BS, BE, BP = np.concatenate(BS), np.concatenate(BE), np.concatenate(BP)
    assert (BS >= 0).all() and (BS <= BE).all()
    for c, m in enumerate((0.3, 0.5, 0.7)):
        ious = np.asarray(al.ious_of_spans(ds.records, BS[:, c], BE[:, c]), dtype=np.float64)
        assert res['R1_bayes@%g' % m] == float(np.mean(ious >= m) * 100.0)
        assert res['bayes_conf@%g' % m] == float(np.mean(BP[:, c], dtype=np.float64))
    both = r.evaluate(k=k, nms_iou=0.5, rerank='hit_prob', bayes_spans=True)
    assert sorted(both) == sorted(list(plain) + keys + ['hit_conf', 'ece@0.7', 'brier@0.7']) and all(both[x] == res[x] for x in keys)
    print('hit-probability evaluation: R1@0.7 %.2f plain, %.2f of the Bayes span; hit conf %.4f, ECE %.4f' % (
        plain['R1@0.7'], res['R1_bayes@0.7'], both['hit_conf'], both['ece@0.7']))
    with pytest.raises(ValueError, match='rerank'):
        r.evaluate(rerank='score')
    with pytest.raises(lib.HualError, match='denominator'):
        r.evaluate(rerank='hit_prob', hit_iou=0.3001234567)
