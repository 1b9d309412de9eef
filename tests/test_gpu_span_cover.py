"""GPU: hual_span_hit_cover (the cumulative coverage of proposals and, per exact rational IoU threshold, the greedy set of maximal
coverage) against the float64 enumeration of its contract (tests/span_cover_ref.py), its identities with hual_span_hit_prob and
hual_span_topk, its edge rows, repeat launches and graph capture, and where it lands: Runner.evaluate(bayes_sets=True).

The bar: 1e-6 absolute on every probability, the project's bar for float64-accumulated probabilities stored as float32.  The kernel sums
exact float64 products of float32 probabilities; its prefix differences and the order of its sums are worth a few 2^-53 per term, and
the one float32 rounding of a value <= 1 is at most 2^-25 = 3e-8.
Regret, with no exemptions: at every step, given the kernel's own earlier picks, the enumeration's best gain minus the enumeration's gain
of the kernel's pick is <= 2e-6 - two bars, one for each side's rounding.  The pick is the enumeration's first maximiser wherever its
runner-up lies >= 1e-5 (ten bars) below; stop decisions are equal wherever the enumeration's best gain is >= 2e-6 away from min_gain.
The steps too close to call may be at most 5 % in the scale-1, K = 5 cases - asserted on the enumeration alone, before a device value
is read (late steps at scale 3 have tiny gains and all but tie: no cap there).  At 256 frames all (candidate, truth) pairs are too many:
the candidates are a field - the kernel's own picks, the mode, the proposals and random spans - against all truths."""
import functools

import numpy as np
import pytest
import torch

import span_cover_ref as V
import span_topk_ref as R
from span_clip_util import _pads_intact, _sentinel, _task, _videos

pytestmark = pytest.mark.gpu

BAR, GAP, EXEMPT, REGRET, STOP = 1e-6, 1e-5, 0.05, 2e-6, 2e-6
B, TS, KS, SCALES, SEED = 8, (2, 33, 70, 256), (1, 5, 16), (1, 3), 7
NB = B + 2                                                            # + one poisoned row (8) and one empty row (9)
MIN_GAINS = (1e-6, 0.05)
FIELD = 200                                                           # random spans per row in the field at 256 frames
# the launches of every case and the columns of the one reference they are checked against (those of test_gpu_span_hit.py)
REF_THR = [(1, 1024), (3, 10), (1, 2), (7, 10), (1, 1)]
LAUNCHES = {'three': [(3, 10), (1, 2), (7, 10)], 'one': [(1, 1)], 'four': [(1, 1024), (3, 10), (1, 2), (7, 10)]}
COLS = {name: [REF_THR.index(t) for t in thr] for name, thr in LAUNCHES.items()}


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def inputs(T, scale, seed=SEED):
    """the B rows of test_gpu_span_hit.py - logits scale * N(0, 1); lengths T, T - 1, 1, 2 and random ones - then row 0 again with a
    NaN logit and row 1 again with length 0"""
    g = torch.Generator().manual_seed(1000 * seed + 10 * T + scale)
    s, e = torch.randn(B, T, generator=g) * scale, torch.randn(B, T, generator=g) * scale
    vl = torch.randint(1, T + 1, (B,), generator=g, dtype=torch.int32)
    vl[0], vl[1], vl[2], vl[3] = T, max(1, T - 1), 1, min(T, 2)
    s, e, vl = torch.cat([s, s[:2]]), torch.cat([e, e[:2]]), torch.cat([vl, vl[:2]])
    e[B, T // 2] = float('nan')
    vl[B + 1] = 0
    return s, e, vl


@functools.lru_cache(maxsize=None)
def refs(T, scale):
    """the enumeration of every row over the whole triangle (T <= 70)"""
    return V.clips(*inputs(T, scale), REF_THR)


def _run(dev, s, e, vl, thr, st=None, en=None, K=0, min_gain=1e-6):
    """one launch into sentinel-filled outputs; -> numpy (set_prob [n,k,M] or None, (cover_start, cover_end, cover_prob) [n,M,K] or None)
    after checking the memory around them and that every element was written"""
    from hual_amd import lib
    n, M = s.shape[0], len(thr)
    outs, guards = [None, None], []
    if st is not None:
        sp, whole, pad = _sentinel((n, st.shape[1], M), torch.float32, dev, 777.0)
        outs[0] = sp
        guards.append((sp, whole, pad, 777.0))
    if K:
        trio = []
        for dt, val in ((torch.int64, -99), (torch.int64, -99), (torch.float32, 777.0)):
            x, whole, pad = _sentinel((n, M, K), dt, dev, val)
            trio.append(x)
            guards.append((x, whole, pad, val))
        outs[1] = tuple(trio)
    got = lib.span_hit_cover(s, e, vl, thr, starts=st, ends=en, K=K, min_gain=min_gain, out=tuple(outs))
    assert got[0] is outs[0] and (got[1] is None) == (K == 0)
    torch.cuda.synchronize()
    for x, whole, pad, val in guards:
        assert _pads_intact(whole, pad, val)
        assert not bool((x == val).any())                              # every element was written
    return (None if outs[0] is None else outs[0].cpu().numpy()), (tuple(x.cpu().numpy() for x in outs[1]) if K else None)


_CASES = {}


def case(dev, T, k, scale):
    """inputs, the proposals of lib.span_topk at nms_iou 0.5 with three hand-placed invalid slots, and the device values of every
    launch with K = k at both min_gain: computed once"""
    key = (T, k, scale)
    if key not in _CASES:
        from hual_amd import lib
        s, e, vl = inputs(T, scale)
        sd, ed, vd = s.to(dev), e.to(dev), vl.to(dev)
        st, en, sc = lib.span_topk(sd, ed, vd, k, nms_iou=0.5)
        st[4, k // 2], en[4, k // 2] = -1, -1                         # no proposal
        st[5, k - 1], en[5, k - 1] = 1, 0                             # a > b
        en[6, 0] = T                                                  # b >= v
        keep = (st.clone(), en.clone())
        got = {(name, mg): _run(dev, sd, ed, vd, thr, st, en, K=k, min_gain=mg) for name, thr in LAUNCHES.items() for mg in MIN_GAINS}
        for a, b in zip((st, en), keep):                              # the proposal arrays are only read
            assert torch.equal(a, b)
        _CASES[key] = dict(dev=(sd, ed, vd, st, en, sc), st=st.cpu().numpy(), en=en.cpu().numpy(), got=got)
    return _CASES[key]


def _walk(c, m, cs, ce, cp, min_gain, exact, stats):
    """one (row, threshold): the kernel's set cs / ce / cp [K] against the ClipCover c at its column m, step by step given the kernel's
    own earlier picks"""
    picks, stopped = [], False
    for s in range(len(cs)):
        a, z = int(cs[s]), int(ce[s])
        prev = float(cp[s - 1]) if s else 0.0
        if stopped:
            assert (a, z) == (-1, -1) and float(cp[s]) == prev, (m, s)
            continue
        g = c.gains(m, picks)
        x = int(np.argmax(g))
        best = float(g[x])
        if abs(best - min_gain) >= STOP:                              # the stop decision
            assert (a < 0) == (best <= min_gain), (m, s, best, min_gain, (a, z))
        if a < 0:
            assert z == -1 and float(cp[s]) == prev, (m, s)
            stopped = True
            continue
        assert c.valid(a, z), (m, s, (a, z))
        y = c.index(a, z)
        regret = best - float(g[y])
        stats['regret'] = max(stats['regret'], regret)
        assert regret <= REGRET, (m, s, (a, z), regret)
        stats['steps'] += 1
        if exact:
            runner = float(np.delete(g, x).max()) if len(g) > 1 else -np.inf
            if best - runner >= GAP:
                assert y == x, (m, s, (a, z), (int(c.ca[x]), int(c.cb[x])))
            else:
                stats['close'] += 1
        picks.append((a, z))
        d = abs(float(cp[s]) - c.coverage(m, picks)[-1])
        stats['prob'] = max(stats['prob'], d)
        assert d <= BAR and 0.0 <= float(cp[s]) <= 1.0 and float(cp[s]) >= prev, (m, s, d)


def _dead_rows(sp, cover):
    for b in (B, B + 1):                                              # the poisoned and the empty row
        assert sp is None or (sp[b] == -1.0).all()
        assert (cover[0][b] == -1).all() and (cover[1][b] == -1).all() and (cover[2][b] == -1.0).all()


# ---------------------------------------------------------------------------------------------------------------- 1. values, picks, stops
@pytest.mark.parametrize('scale', SCALES)
@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('T', (2, 33, 70))
def test_sets_against_the_full_enumeration(dev, T, k, scale):
    rows = refs(T, scale)
    assert all(r is not None for r in rows[:B]) and rows[B] is None and rows[B + 1] is None
    if scale == 1 and k == 5:
        # on the enumeration alone: the steps of its own greedy sets with a runner-up too close to call are few
        steps = close = 0
        for r in rows[:B]:
            for m in COLS['three']:
                gap = r.greedy(m, k, MIN_GAINS[0])[3]
                steps, close = steps + len(gap), close + int((gap < GAP).sum())
        print('T=%d scale=%d K=%d: %d of %d steps have a runner-up within %.0e of the best gain' % (T, scale, k, close, steps, GAP))
        assert close <= EXEMPT * steps
    c = case(dev, T, k, scale)
    stats = dict(regret=0.0, prob=0.0, steps=0, close=0)
    worst_set = 0.0
    for (name, mg), (sp, cover) in c['got'].items():
        cols = COLS[name]
        assert sp.shape == (NB, k, len(cols)) and all(x.shape == (NB, len(cols), k) for x in cover)
        _dead_rows(sp, cover)
        for b, r in enumerate(rows[:B]):
            props = list(zip(c['st'][b], c['en'][b]))
            for x, m in enumerate(cols):
                want = r.coverage(m, props)
                d = float(np.abs(sp[b, :, x].astype(np.float64) - want).max())
                worst_set = max(worst_set, d)
                assert d <= BAR, (name, b, m, d)
                _walk(r, m, cover[0][b, x], cover[1][b, x], cover[2][b, x], mg, True, stats)
        # a threshold's column does not depend on the launch it is part of
        for other, ocols in COLS.items():
            for x, col in enumerate(cols):
                if col in ocols:
                    y = ocols.index(col)
                    assert (sp[:, :, x].view(np.int32) == c['got'][(other, mg)][0][:, :, y].view(np.int32)).all()
                    for u, w in zip(cover, c['got'][(other, mg)][1]):
                        assert (u[:, x] == w[:, y]).all()
    print('T=%d k=K=%d scale=%d: max |set_prob - enumeration| %.3e, |cover_prob - enumeration| %.3e, regret %.3e (bars %.0e / %.0e); '
          '%d of %d steps too close to call' % (T, k, scale, worst_set, stats['prob'], stats['regret'], BAR, REGRET, stats['close'], stats['steps']))
    # invalid slots add nothing; v == 1 is (0, 0) with probability exactly 1, then stopped slots
    sp, cover = c['got'][('three', MIN_GAINS[0])]
    if k > 1:
        assert (sp[4, k // 2] == sp[4, k // 2 - 1]).all() and (sp[5, k - 1] == sp[5, k - 2]).all()
    assert (sp[6, 0] == 0.0).all()                                    # no valid slot seen yet
    assert (sp[2] == 1.0).all() and (cover[0][2, :, 0] == 0).all() and (cover[1][2, :, 0] == 0).all() and (cover[2][2] == 1.0).all()
    assert (cover[0][2, :, 1:] == -1).all() and (cover[1][2, :, 1:] == -1).all()
    assert all(len(np.nonzero(cover[0][3, x] >= 0)[0]) <= 3 for x in range(3))      # v == 2 has three spans
    if k > 1:                                                         # stops occur (row 2 has one span)
        assert all((cv[0][:B, :, 1:] < 0).any() for (_, mg), (_, cv) in c['got'].items())


@pytest.mark.parametrize('scale', SCALES)
def test_sets_at_256_frames(dev, scale):
    from hual_amd import lib
    T, K, thr = 256, 16, LAUNCHES['three']
    s, e, vl = inputs(T, scale)
    c = case(dev, T, K, scale)
    sd, ed, vd, st, en, sc = c['dev']
    mode = lib.span_topk(sd, ed, vd, 1)
    mode = np.stack([mode[0].cpu().numpy(), mode[1].cpu().numpy()], axis=2)                     # [NB, 1, 2]
    ps, pe, v, _ = R.probabilities(s, e, vl)
    g = np.random.default_rng(100 * SEED + scale)
    stats = dict(regret=0.0, prob=0.0, steps=0, close=0)
    worst_set = 0.0
    for mg in MIN_GAINS:
        _dead_rows(*c['got'][('three', mg)])
    for b in range(B):
        n = int(v[b])
        own = [np.stack([c['got'][('three', mg)][1][0][b].ravel(), c['got'][('three', mg)][1][1][b].ravel()], axis=1) for mg in MIN_GAINS]
        field = np.concatenate(own + [mode[b], np.stack([c['st'][b], c['en'][b]], axis=1), np.sort(g.integers(0, n, size=(FIELD, 2)), axis=1)])
        field = np.unique(field[(field[:, 0] >= 0) & (field[:, 0] <= field[:, 1]) & (field[:, 1] < n)], axis=0)
        r = V.ClipCover(ps[b], pe[b], n, thr, cands=field)
        assert r.alive
        for k in KS:                                                  # the proposals' cumulative coverage at every k
            ck = case(dev, T, k, scale)
            sp = ck['got'][('three', MIN_GAINS[0])][0]
            for m in range(3):
                d = float(np.abs(sp[b, :, m].astype(np.float64) - r.coverage(m, list(zip(ck['st'][b], ck['en'][b])))).max())
                worst_set = max(worst_set, d)
                assert d <= BAR, (k, b, m, d)
        for mg in MIN_GAINS:
            cover = c['got'][('three', mg)][1]
            for m in range(3):
                _walk(r, m, cover[0][b, m], cover[1][b, m], cover[2][b, m], mg, False, stats)
    for k in KS[:-1]:                                                 # a smaller K: the first columns, bit for bit
        for mg in MIN_GAINS:
            for u, w in zip(case(dev, T, k, scale)['got'][('three', mg)][1], c['got'][('three', mg)][1]):
                assert (u.view(np.int32) == np.ascontiguousarray(w[:, :, :k]).view(np.int32)).all()
    print('T=256 scale=%d: max |set_prob - enumeration| %.3e, |cover_prob - enumeration| %.3e, best field span above the kernel\'s pick by '
          'at most %.3e over %d steps (bars %.0e / %.0e)' % (scale, worst_set, stats['prob'], stats['regret'], stats['steps'], BAR, REGRET))


# ---------------------------------------------------------------------------------------------------------------- 2. identities on the device
@pytest.mark.parametrize('scale', SCALES)
@pytest.mark.parametrize('T', TS)
def test_identities_with_hit_prob_and_topk(dev, T, scale):
    from hual_amd import lib
    c5, c16 = case(dev, T, 5, scale), case(dev, T, 16, scale)
    sd, ed, vd, st, en, sc = c16['dev']
    for name, thr in LAUNCHES.items():
        # step 0 at min_gain = 0 is the Bayes search of hual_span_hit_prob, bit for bit
        hp, best = lib.span_hit_prob(sd, ed, vd, thr, starts=st, ends=en, best=True)
        sp, cover = _run(dev, sd, ed, vd, thr, st, en, K=1, min_gain=0.0)
        for u, w in zip(cover, best):
            assert (np.ascontiguousarray(u[:, :, 0]).view(np.int32) == w.cpu().numpy().view(np.int32)).all(), name
        # column 0 of a valid slot is its hit probability
        hp = hp.cpu().numpy()
        ok = hp[:, 0, :] >= 0
        assert ok[:4].all() and not ok[6].any() and float(np.abs(sp[:, 0, :][ok] - hp[:, 0, :][ok]).max()) <= BAR
        assert (sp[:B, 0, :][~ok[:B]] == 0.0).all() and (sp[B:] == -1.0).all()
        for mg in MIN_GAINS:
            # K = 5 is the first five columns of K = 16, bit for bit
            for u, w in zip(c5['got'][(name, mg)][1], c16['got'][(name, mg)][1]):
                assert (u.view(np.int32) == np.ascontiguousarray(w[:, :, :5]).view(np.int32)).all()
            # the cover set as proposals: set_prob is cover_prob
            cs, ce, cp = c16['got'][(name, mg)][1]
            for x in range(len(thr)):
                fed = _run(dev, sd, ed, vd, thr, torch.from_numpy(np.ascontiguousarray(cs[:, x])).to(dev),
                           torch.from_numpy(np.ascontiguousarray(ce[:, x])).to(dev))[0]
                assert float(np.abs(fed[:, :, x].astype(np.float64) - cp[:, x].astype(np.float64)).max()) <= BAR
        # the theorem against the NMS set: the greedy set covers at least 1 - (1 - 1/K)^K of what ANY K spans cover
        for K, ck in ((5, c5), (16, c16), (1, case(dev, T, 1, scale))):
            sp, cover = ck['got'][(name, MIN_GAINS[0])]
            assert (cover[2][:B, :, K - 1] >= (1 - (1 - 1 / K) ** K) * sp[:B, K - 1, :] - BAR).all()
    # at 1 / 1 a span hits only itself: the set is the most probable spans, those of hual_span_topk without NMS
    cs, ce, cp = c16['got'][('one', MIN_GAINS[0])][1]
    ts, te, tsc = (x.cpu().numpy() for x in lib.span_topk(sd, ed, vd, 16, nms_iou=1.0))
    compared = 0
    for b in range(B):
        for q in range(15):
            if cs[b, 0, q] < 0 or ts[b, q + 1] < 0:
                break
            lo, hi = tsc[b, q + 1], tsc[b, q - 1] if q else np.inf
            if tsc[b, q] - lo >= 1e-5 * tsc[b, q] and hi - tsc[b, q] >= 1e-5 * tsc[b, q]:
                assert (cs[b, 0, q], ce[b, 0, q]) == (ts[b, q], te[b, q]), (b, q)
                compared += 1
    assert compared >= (1 if T == 2 else B)


# ---------------------------------------------------------------------------------------------------------------- 3. edge rows
def test_edge_rows(dev):
    T, k, thr = 33, 5, LAUNCHES['three']
    s, e, vl = (x[:B].clone() for x in inputs(T, 1))
    vl[:] = torch.tensor([T, 20, 1, 0, T, 20, T + 9, -2])             # row 3 empty; row 6 read as T; row 7 empty
    s[4, 3] = float('nan')                                        # a NaN logit inside the clip: row 4 is poisoned
    e[5, 30] = float('nan')                                       # beyond vlen = 20: not read
    s[1, :], e[1, :] = -200.0, -200.0                             # row 1 (vlen 20): the start certainly last, the end certainly first -
    s[1, 19], e[1, 0] = 200.0, 200.0                              # every weight with i <= j is exactly 0, Z = 0: as a poisoned row
    s[0, 5] = float('inf')                                        # row 0: an infinite logit makes the probabilities NaN, Z with them
    st = torch.tensor([[2, 9, -1, 0, 5]] * B, dtype=torch.int64)
    en = torch.tensor([[6, 4, -1, T - 1, 20]] * B, dtype=torch.int64)           # (9, 4): a > b; (-1, -1): no proposal
    st[2], en[2] = torch.tensor([-1, 0, 0, 1, 0]), torch.tensor([-1, 0, 0, 1, 1])      # v = 1: (0, 0) twice, the rest beyond the clip
    st[6], en[6] = torch.tensor([-1, 9, 4, 3, -5]), torch.tensor([4, 4, T, -1, -5])    # every slot invalid
    rows = V.clips(s, e, vl, thr)
    dead = [0, 1, 3, 4, 7]
    assert [b for b, r in enumerate(rows) if r is None] == dead
    sd, ed, vd = s.to(dev), e.to(dev), vl.to(dev)
    std, st_w, p0 = _sentinel((B, k), torch.int64, dev, -99)
    end, en_w, _ = _sentinel((B, k), torch.int64, dev, -99)
    std.copy_(st), end.copy_(en)
    sp, (cs, ce, cp) = _run(dev, sd, ed, vd, thr, std, end, K=k)
    assert _pads_intact(st_w, p0, -99) and _pads_intact(en_w, p0, -99) and torch.equal(std.cpu(), st) and torch.equal(end.cpu(), en)
    for b in dead:
        assert (sp[b] == -1.0).all() and (cs[b] == -1).all() and (ce[b] == -1).all() and (cp[b] == -1.0).all()
    assert (sp[6] == 0.0).all() and (cs[6, :, 0] >= 0).all() and (cp[6] > 0).all()             # all slots invalid: the greedy set does not mind
    assert (sp[2, 0] == 0.0).all() and (sp[2, 1:] == 1.0).all()                                # v = 1: nothing, then (0, 0)
    assert (cs[2, :, 0] == 0).all() and (ce[2, :, 0] == 0).all() and (cp[2] == 1.0).all() and (cs[2, :, 1:] == -1).all() and (ce[2, :, 1:] == -1).all()
    stats = dict(regret=0.0, prob=0.0, steps=0, close=0)
    for b in (2, 5, 6):                                               # the live rows (row 5 reads 20 frames only) against the enumeration
        r = rows[b]
        assert r.v == (1, 20, T)[(2, 5, 6).index(b)]
        for m in range(3):
            assert float(np.abs(sp[b, :, m] - r.coverage(m, list(zip(st[b].tolist(), en[b].tolist())))).max()) <= BAR
            _walk(r, m, cs[b, m], ce[b, m], cp[b, m], 1e-6, False, stats)
    # the proposals only (cover_* NULL) and the sets only (k = 0): the same bits as together
    sp1, none = _run(dev, sd, ed, vd, thr, std, end)
    none2, cover2 = _run(dev, sd, ed, vd, thr, K=k)
    assert none is None and none2 is None and (sp1.view(np.int32) == sp.view(np.int32)).all()
    for x, y in zip(cover2, (cs, ce, cp)):
        assert (x.view(np.int32) == y.view(np.int32)).all()


# ---------------------------------------------------------------------------------------------------------------- 4. repeat, capture
def test_second_launch_and_captured_graph(dev):
    from hual_amd import lib
    T, k, thr = 70, 5, LAUNCHES['three']
    c = case(dev, T, k, 1)
    sd, ed, vd, st, en, sc = c['dev']

    def outs():
        return (torch.empty(NB, k, 3, dtype=torch.float32, device=dev),
                (torch.empty(NB, 3, k, dtype=torch.int64, device=dev), torch.empty(NB, 3, k, dtype=torch.int64, device=dev),
                 torch.empty(NB, 3, k, dtype=torch.float32, device=dev)))

    def flat(out):
        return (out[0],) + tuple(out[1])
    want, got = outs(), outs()
    lib.span_hit_cover(sd, ed, vd, thr, st, en, K=k, out=want)
    lib.span_hit_cover(sd, ed, vd, thr, st, en, K=k, out=got)
    torch.cuda.synchronize()
    for a, b in zip(flat(got), flat(want)):                           # a second launch: equal bits
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    for a, b in zip(flat(want), (c['got'][('three', 1e-6)][0],) + c['got'][('three', 1e-6)][1]):
        assert (a.cpu().numpy().view(np.int32) == b.view(np.int32)).all()
    out = outs()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        lib.span_hit_cover(sd, ed, vd, thr, st, en, K=k, out=outs())      # (warm-up)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        lib.span_hit_cover(sd, ed, vd, thr, st, en, K=k, out=out)
    for _ in range(2):
        for o in flat(out):
            o.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(flat(out), flat(want)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------- 5. evaluation
def test_bayes_sets_evaluation(tmp_path, monkeypatch):
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
    plain = r.evaluate(k=k, nms_iou=0.5)
    assert sorted(plain) == sorted(['R1@0.3', 'R1@0.5', 'R1@0.7', 'R5@0.3', 'R5@0.5', 'R5@0.7', 'mIoU'])
    with monkeypatch.context() as mp:                                 # the default call: the dict of before, and no launch of the new entry point
        def unavailable(*a, **kw):
            raise AssertionError('the default evaluation launched hual_span_hit_cover')
        mp.setattr(lib, 'span_hit_cover', unavailable)
        assert r.evaluate(k=k, nms_iou=0.5) == plain
        assert r.evaluate(k=k, nms_iou=0.5, bayes_sets=False) == plain
    n_lines = len(lines)
    res = r.evaluate(k=k, nms_iou=0.5, bayes_sets=True)
    ms = (0.3, 0.5, 0.7)
    keys = [x % m for m in ms for x in ('R5_bayes@%g', 'bayes_set_conf@%g', 'set_conf@%g', 'set_ece@%g', 'set_brier@%g')]
    assert sorted(res) == sorted(list(plain) + keys) and all(res[x] == plain[x] for x in plain)
    assert all(np.isfinite(res[x]) for x in keys) and any('Bayes sets' in l for l in lines[n_lines:])
    assert all(0 <= res[x % m] <= 1 for m in ms for x in ('bayes_set_conf@%g', 'set_conf@%g', 'set_ece@%g', 'set_brier@%g'))
    # recomputed on the host from a direct launch on the same logits
    ds = r.test_set
    CS, CE, CP, SP, S, E = [], [], [], [], [], []
    for lo in range(0, len(ds), r.batch_size):
        sel = np.arange(lo, min(len(ds), lo + r.batch_size))
        f = ds.assemble(sel, labels=False, min_chars=4)
        o = r.model.forward(f['video'], f['video_seq_len'], f['word_ids'], f['char_ids'], drop_rate=0.0)
        st, en, _ = lib.span_topk(o['start_logits'], o['end_logits'], f['video_seq_len'], k, nms_iou=0.5)
        sp, (cs, ce, cp) = lib.span_hit_cover(o['start_logits'], o['end_logits'], f['video_seq_len'], ms, st, en, K=k)
        for acc, x in zip((CS, CE, CP, SP, S, E), (cs, ce, cp, sp, st, en)):
            acc.append(x.cpu().numpy())
    CS, CE, CP, SP, S, E = (np.concatenate(x) for x in (CS, CE, CP, SP, S, E))
    assert (CS[:, :, 0] >= 0).all() and (SP >= 0).all()
    counted = al.topk_ious(ds.records, S, E).max(axis=1)
    for c, m in enumerate(ms):
        ious = al.topk_ious(ds.records, CS[:, c], CE[:, c])
        assert res['R5_bayes@%g' % m] == float(np.mean(ious.max(axis=1) >= m) * 100.0)
        assert res['bayes_set_conf@%g' % m] == float(np.mean(CP[:, c, k - 1], dtype=np.float64))
        assert res['set_conf@%g' % m] == float(np.mean(SP[:, k - 1, c], dtype=np.float64))
        cal = al.hit_calibration(SP[:, k - 1, c], counted >= m)
        assert res['set_ece@%g' % m] == cal['ece'] and res['set_brier@%g' % m] == cal['brier']
        assert res['R5@%g' % m] == float(np.mean(counted >= m) * 100.0)
        assert (CP[:, c, k - 1] >= (1 - (1 - 1 / k) ** k) * SP[:, k - 1, c] - BAR).all()
    both = r.evaluate(k=k, nms_iou=0.5, rerank='hit_prob', bayes_spans=True, bayes_sets=True)
    assert all(both[x] == res[x] for x in keys if x.startswith(('R5_bayes', 'bayes_set_conf')))
    assert all(abs(both[x] - res[x]) <= BAR for x in keys if x.startswith('set_conf'))                   # (the proposals come re-ordered)
    assert all(x in both for x in keys + ['R1_bayes@0.7', 'hit_conf'])
    print('Bayes-set evaluation: R5 %s plain, %s of the greedy sets; set conf %s, greedy set conf %s' % tuple(
        ' / '.join('%.2f' % res[x % m] for m in ms) for x in ('R5@%g', 'R5_bayes@%g', 'set_conf@%g', 'bayes_set_conf@%g')))
