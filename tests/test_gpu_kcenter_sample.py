"""GPU: hual_kcenter_sample against the float64 statement of its contract (tests/kcenter_sample_ref.py) - the off switches against
hual_kcenter_greedy, the origin center, D^2 sampling on exact lattice sets, on random sets and against its law - and the places it
lands: al.badge_select and al.update_labels(select_by='badge').

The bars (from the contract's arithmetic, include/hual_seqpan.h; not tuned), u = 2^-24:
  lattice sets   features integers in [-8, 8], D <= 130, weights in {0, 1/4, 1/2, 1}: mind and w * mind are exact in float32, so the
                 kernel's score differs from the reference's by the one rounding of the division (and the float64 logarithm's last
                 bit, far below it).  The pick equals the reference's wherever the reference's runner-up lies 1e-5 relative below
                 its best - 170 u, so a compared step cannot legitimately differ - and at most 5 % of the steps may go uncompared.
  regret         random sets, teacher-forced on the kernel's own earlier picks: the reference score of the kernel's pick lies within
                 2 (D + 6) u relative of the reference's best - k-center's 2 (D + 4) u with one more u per score for the division
                 and one for the rounding of E to float32.
  values         mind and pick_dist within (D + 3) u relative of the reference: k-center's own bar."""
import copy
import math

import numpy as np
import pytest
import torch

import al_synth
import kcenter_sample_ref as SR
from span_clip_util import _pads_intact, _sentinel

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
FILL, IFILL = 777.0, 777
KEYS = ('picked', 'pick_dist', 'mind', 'assign')


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def run_ks(dev, x, n_select, weight=None, init=None, ld=None, greedy_call=False, **switches):
    """one selection into sentinel-filled, padded outputs -> dict of numpy arrays, after checking the memory around them; ld: the
    row stride x is laid out with on the device (the columns beyond D hold NaN: nothing may read them); greedy_call: through
    lib.kcenter_select (hual_kcenter_greedy) instead"""
    from hual_amd import lib
    N, D = x.shape
    ld = D if ld is None else ld
    whole = torch.full((N, ld), float('nan'), dtype=torch.float32, device=dev)
    whole[:, :D] = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)
    xd = whole[:, :D]
    wd = None if weight is None else torch.from_numpy(np.ascontiguousarray(weight, dtype=np.float32)).to(dev)
    bufs = [_sentinel((n_select,), torch.int32, dev, IFILL), _sentinel((n_select,), torch.float32, dev, FILL),
            _sentinel((N,), torch.float32, dev, FILL), _sentinel((N,), torch.int32, dev, IFILL)]
    out = tuple(b[0] for b in bufs)
    if greedy_call:
        got = lib.kcenter_select(xd, n_select, weight=wd, init=init, out=out)
    else:
        got = lib.kcenter_sample(xd, n_select, weight=wd, init=init, out=out, **switches)
    assert all(g is o for g, o in zip(got, out))
    torch.cuda.synchronize()
    for b, fill in zip(bufs, (IFILL, FILL, FILL, IFILL)):
        assert _pads_intact(b[1], b[2], fill)
    return dict(zip(KEYS, (o.cpu().numpy() for o in out)))


def lattice(N, D, seed):
    """integer features in [-8, 8] with 7 duplicated rows (as many as N allows), weights from {0, 1/4, 1/2, 1}, the duplicates'
    weights equal to their source's for every other one: exact ties in score, in (score, w) and none (the sets of the k-center tests,
    restated)"""
    g = np.random.default_rng(seed)
    x = g.integers(-8, 9, size=(N, D)).astype(np.float32)
    w = g.choice(np.array([0.0, 0.25, 0.5, 1.0], dtype=np.float32), size=N)
    for j in range(min(7, N - 1)):
        dst, src = (int(v) for v in g.choice(N, size=2, replace=False))
        x[dst] = x[src]
        if j % 2 == 0:
            w[dst] = w[src]
    return x, w


# ---------------------------------------------------------------------------------------------------------------- 1. the off switches
@pytest.mark.parametrize('N', [1, 2, 65, 300, 1031])
@pytest.mark.parametrize('D', [1, 4, 130])
def test_both_switches_off_is_the_greedy_call_bit_for_bit(dev, N, D):
    x, w = lattice(N, D, seed=1000 * N + D)
    g = np.random.default_rng(N + D)
    for n_init in sorted({0, min(5, N)}):
        init = g.choice(N, size=n_init, replace=False).tolist()
        for n_select in sorted({1, math.ceil(N / 2), N}):
            for ld in (D, D + 3):
                want = run_ks(dev, x, n_select, w, init=init, ld=ld, greedy_call=True)
                got = run_ks(dev, x, n_select, w, init=init, ld=ld, seed=99, offset=7, sample=False, origin=False)
                for key in KEYS:
                    assert same_bits(got[key], want[key]), (N, D, ld, n_select, n_init, key)


@pytest.mark.parametrize('N,D,ld', [(1, 1, 1), (65, 4, 4), (65, 4, 7), (300, 130, 130), (300, 130, 133), (257, 1000, 1000)])
def test_origin_opens_with_the_distance_to_zero(dev, N, D, ld):
    """mind after the opening equals d(i, 0) bit for bit, on rows of random floats: a greedy call whose only center is an appended
    zero row computes d(i, zero row) with the distance routine itself, scores the same rows with the same weights, and must then
    make the same first pick and leave the same mind after the same closing update.  The first pick is the row of maximal
    (w |x|^2, w, -i)"""
    g = np.random.default_rng(N + D + ld)
    x = g.standard_normal((N, D)).astype(np.float32)
    w = g.uniform(0.1, 1, size=N).astype(np.float32)
    if N >= 65:
        x[7] = x[40]                                                       # bit-equal rows: bit-equal distances
        w[7] = w[40]
        x[9] = 0.0                                                         # a row on the origin
    x0 = np.concatenate([x, np.zeros((1, D), dtype=np.float32)])
    w0 = np.concatenate([w, np.ones(1, dtype=np.float32)])
    via_row = run_ks(dev, x0, 1, w0, init=[N], ld=ld, greedy_call=True)
    r = run_ks(dev, x, 1, w, ld=ld, sample=False, origin=True)
    assert same_bits(r['picked'], via_row['picked']) and same_bits(r['pick_dist'], via_row['pick_dist'])
    assert same_bits(r['mind'], via_row['mind'][:N])
    np.testing.assert_array_equal(r['assign'], np.where(via_row['assign'][:N] == N, -1, via_row['assign'][:N]))
    first = int(r['picked'][0])
    ref = SR.run(x, 1, w, sample=False, origin=True)
    assert abs(float(r['pick_dist'][0]) - ref['open_mind'][first]) <= (D + 3) * U * ref['open_mind'][first]
    score = w.astype(np.float64) * ref['open_mind']
    assert score[first] >= score.max() * (1 - 2 * (D + 4) * U)
    if N >= 65:
        assert (r['assign'] == -1).any() and r['mind'][9] == 0.0 and r['assign'][9] == -1
        assert same_bits(r['mind'][[7]], r['mind'][[40]])


def test_origin_on_lattice_sets_equals_the_reference(dev):
    """exact arithmetic: all four outputs equal the reference with the origin center, greedy"""
    for N, D in ((65, 4), (300, 130)):
        x, w = lattice(N, D, seed=1000 * N + D + 1)
        for init in ([], [3, 11]):
            n_select = math.ceil(N / 2)
            ref = SR.run(x, n_select, w, init=init, sample=False, origin=True)
            r = run_ks(dev, x, n_select, w, init=init, ld=D + 3, sample=False, origin=True)
            np.testing.assert_array_equal(r['picked'], ref['picked'])
            np.testing.assert_array_equal(r['pick_dist'].astype(np.float64), ref['pick_dist'])
            np.testing.assert_array_equal(r['mind'].astype(np.float64), ref['mind'])
            np.testing.assert_array_equal(r['assign'], ref['assign'])
            assert (r['assign'] == -1).any()                               # some rows stay nearest to the origin


# ---------------------------------------------------------------------------------------------------------------- 2. sampling, lattice sets
GAP = 1e-5


@pytest.mark.parametrize('N', [1, 2, 65, 300])
@pytest.mark.parametrize('D', [1, 4, 130])
def test_sampling_on_lattice_sets_follows_the_reference(dev, N, D):
    """teacher-forced on the kernel's picks: wherever the reference's runner-up lies 1e-5 relative below its best, the pick is the
    reference's; mind is exact, so every state after the walk equals the reference's"""
    x, w = lattice(N, D, seed=1000 * N + D)
    w[w == 0] = 0.25
    total = compared = 0
    for origin, init, seed in ((True, [], 5), (False, [min(3, N - 1)], 6), (False, [], 7)):
        n_select = N - len(init)
        if n_select == 0:                                                  # (N = 1 with its row in init: nothing is owed)
            continue
        for ld in (D, D + 3):
            r = run_ks(dev, x, n_select, w, init=init, ld=ld, seed=seed, offset=3, sample=True, origin=origin)
            st = SR.State(x, w, init, seed=seed, offset=3, sample=True, origin=origin)
            for s, c in enumerate(r['picked'].tolist()):
                best, dist, gap = st.best()
                score, el = st.scores()
                assert c >= 0 and el[c], (N, D, ld, s, c)
                total += 1
                if gap > GAP:
                    compared += 1
                    assert c == best, (N, D, ld, origin, s, c, best, gap)
                # a zero-mass row (a duplicate of a center) is taken only when no positive mass is left
                m, _ = st.mass()
                assert m[c] > 0 or not (m[el] > 0).any()
                assert float(r['pick_dist'][s]) == st.mind[c]
                st.advance(c)
            np.testing.assert_array_equal(r['mind'].astype(np.float64), st.mind)
            if compared == total:
                np.testing.assert_array_equal(r['assign'], st.assign)
    print('N %d D %d: %d of %d steps compared (%.1f %%)' % (N, D, compared, total, 100.0 * compared / total))
    assert compared >= 0.95 * total


# ---------------------------------------------------------------------------------------------------------------- 3. sampling, random sets
def forced(x, w, init, r, D, **switches):
    """teacher-forced walk along the kernel's picks -> (max regret, max relative error of pick_dist, the final State)"""
    st = SR.State(x, w, init, **switches)
    regret, dist_err = 0.0, 0.0
    for s, c in enumerate(r['picked'].tolist()):
        score, el = st.scores()
        assert c >= 0 and el[c], (s, c)
        top = score[el].max()
        regret = max(regret, (top - score[c]) / top if top > 0 else 0.0)
        want, got = st.mind[c], float(r['pick_dist'][s])
        dist_err = max(dist_err, 0.0 if want == got else abs(got - want) / want)
        st.advance(c)
    return regret, dist_err, st


@pytest.mark.parametrize('N', [300, 1031])
@pytest.mark.parametrize('origin', [False, True])
def test_sampling_on_random_sets_follows_the_reference(dev, N, origin):
    D = 130
    g = np.random.default_rng(7 * N + origin)
    x = g.standard_normal((N, D)).astype(np.float32)
    w = g.uniform(0, 1, size=N).astype(np.float32) if origin else None
    init = g.choice(N, size=3, replace=False).tolist() if origin else []
    n_select = math.ceil(N / 2)
    sw = dict(seed=(1 << 40) + 17, offset=2, sample=True, origin=origin)
    r = run_ks(dev, x, n_select, w, init=init, **sw)
    regret, dist_err, st = forced(x, w, init, r, D, **sw)
    err = float((np.abs(r['mind'].astype(np.float64) - st.mind) / np.maximum(st.mind, 1e-300)).max())
    print('N %d D %d origin %d: max regret %.3e (bar %.3e); max rel err mind %.3e, pick_dist %.3e (bar %.3e)'
          % (N, D, origin, regret, 2 * (D + 6) * U, err, dist_err, (D + 3) * U))
    assert regret <= 2 * (D + 6) * U
    assert err <= (D + 3) * U and dist_err <= (D + 3) * U
    assert len(set(r['picked'].tolist())) == n_select
    other = run_ks(dev, x, n_select, w, init=init, **dict(sw, seed=sw['seed'] + 1))
    assert other['picked'].tolist() != r['picked'].tolist()                # another seed, another draw


# ---------------------------------------------------------------------------------------------------------------- 4. the law
def test_sampling_follows_its_law(dev):
    """the 2,000-seed chi-square case of tests/test_grad_embed.py on the device: n_select = 1, six rows of pairwise distinct mass"""
    from hual_amd import lib
    x, w, init, mass = SR.law_case()
    xd, wd = torch.from_numpy(x).to(dev), torch.from_numpy(w).to(dev)
    init_d = torch.tensor(init, dtype=torch.int32, device=dev)
    N = len(x)
    ws = torch.empty(lib.kcenter_workspace_bytes(N), dtype=torch.uint8, device=dev)
    picked = torch.full((SR.LAW_SEEDS, 1), -1, dtype=torch.int32, device=dev)
    out = (torch.empty(1, device=dev), torch.empty(N, device=dev), torch.empty(N, dtype=torch.int32, device=dev))
    for j in range(SR.LAW_SEEDS):
        lib.kcenter_sample(xd, 1, weight=wd, init=init_d, seed=SR.LAW_SEED_BASE + j, sample=True, origin=False,
                           out=(picked[j],) + out, workspace=ws, validate=False)
    got = picked.cpu().numpy()[:, 0]
    compared = 0
    for j in range(SR.LAW_SEEDS):
        ref = SR.run(x, 1, w, init=init, seed=SR.LAW_SEED_BASE + j, sample=True, origin=False)
        if ref['gap'][0] > GAP:
            compared += 1
            assert got[j] == ref['picked'][0], j
    counts = np.bincount(got, minlength=N)[1:]
    stat = SR.chi_square(counts, mass)
    print('chi-square %.2f (bar %.1f), counts %s; %d of %d picks compared with the reference' % (stat, SR.LAW_BAR, counts.tolist(), compared, SR.LAW_SEEDS))
    assert got.min() >= 1 and compared >= 0.95 * SR.LAW_SEEDS
    assert stat < SR.LAW_BAR


# ---------------------------------------------------------------------------------------------------------------- 5. edges
def test_rows_that_are_never_drawn(dev):
    N, D = 65, 4
    x, w = lattice(N, D, seed=5)
    w[w == 0] = 0.25
    w[[3, 17, 40]] = -1.0
    w[[8, 64]] = np.nan
    x[[21, 50]] = np.nan
    x[33, 2] = np.inf
    bad = {3, 17, 40, 8, 64, 21, 50, 33}
    for origin in (False, True):
        r = run_ks(dev, x, N, w, seed=12, sample=True, origin=origin)
        assert not set(r['picked'].tolist()) & bad
        live = N - len(bad)
        assert (r['picked'][:live] >= 0).all() and len(set(r['picked'][:live].tolist())) == live
        assert (r['picked'][live:] == -1).all() and (r['pick_dist'][live:] == -1.0).all()      # an exhausted selection
        # a NaN row moves no other row: the selection without those rows, same draws per row index -> the same state on the others
        st = SR.State(x, w, [], seed=12, sample=True, origin=origin)
        for c in r['picked'][:live].tolist():
            assert st.scores()[1][c]
            st.advance(c)
        good = np.isfinite(x).all(axis=1)
        np.testing.assert_array_equal(r['mind'][good].astype(np.float64), st.mind[good])
        assert np.isnan(r['mind'][21]) and np.isnan(r['mind'][50])
    r = run_ks(dev, x, 9, w, init=np.random.default_rng(6).permutation(N).tolist(), seed=1)
    assert (r['picked'] == -1).all() and (r['pick_dist'] == -1.0).all()    # every row in init
    r = run_ks(dev, x, 0, w, seed=1)
    assert r['picked'].shape == (0,) and (r['mind'] == FILL).all() and (r['assign'] == IFILL).all()      # nothing owed, nothing written


def test_second_call_and_graph_replays_return_equal_bits(dev):
    from hual_amd import lib
    N, D, n_select = 1031, 130, 64
    g = np.random.default_rng(21)
    x = g.standard_normal((N, D)).astype(np.float32)
    x[5] = x[900]
    w = g.uniform(0, 1, size=N).astype(np.float32)
    init = [17, 333]
    sw = dict(seed=(7 << 32) + 5, offset=9, sample=True, origin=True)
    want = run_ks(dev, x, n_select, w, init=init, **sw)
    again = run_ks(dev, x, n_select, w, init=init, **sw)
    for key in want:
        assert same_bits(again[key], want[key]), key
    xd, wd = torch.from_numpy(x).to(dev), torch.from_numpy(w).to(dev)
    init_d = torch.tensor(init, dtype=torch.int32, device=dev)
    ws = torch.empty(lib.kcenter_workspace_bytes(N), dtype=torch.uint8, device=dev)

    def outs():
        return (torch.full((n_select,), IFILL, dtype=torch.int32, device=dev), torch.full((n_select,), FILL, device=dev),
                torch.full((N,), FILL, device=dev), torch.full((N,), IFILL, dtype=torch.int32, device=dev))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        lib.kcenter_sample(xd, n_select, weight=wd, init=init_d, out=outs(), workspace=ws, validate=False, **sw)      # (warm-up)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    out = outs()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        lib.kcenter_sample(xd, n_select, weight=wd, init=init_d, out=out, workspace=ws, validate=False, **sw)
    for _ in range(2):
        for o in out:
            o.fill_(5)
        ws.fill_(255)                                            # (the workspace's contents are irrelevant on entry)
        graph.replay()
        torch.cuda.synchronize()
        for o, key in zip(out, KEYS):
            assert same_bits(o.cpu().numpy(), want[key]), key


# ---------------------------------------------------------------------------------------------------------------- 6. the round
def _synth(dev):
    """al_synth.make_trainset(N = 24, 8 videos) with random logits as records, truthful answers of earlier rounds on every other sample,
    and random gradient-like descriptors with two certain samples (zero rows) and one poisoned one (a NaN row)"""
    from hual_amd import al
    N = 24
    recs, vis, data_gt, data_old = al_synth.make_trainset(N, 8, 16, 40, seed=31)
    g = torch.Generator().manual_seed(31)
    rng = np.random.default_rng(31)
    prop = []
    for r in recs:
        s, e = (torch.randn(r['v_len'], generator=g) * 2).numpy(), (torch.randn(r['v_len'], generator=g) * 2).numpy()
        prop.append({'vid': r['vid'], 'v_len': int(r['v_len']), 'prop_logits': (s, e), 'prop_logits1': (s, e), 'prop_logits2': (s, e)})
    for i, (old, gt, r) in enumerate(zip(data_old, data_gt, recs)):
        pts = {'pos_idx': [], 'neg_idx': []}
        if i % 2 == 0:
            a, b = (al._round_half_even_index(t, gt[1], r['v_len']) for t in gt[2])
            f = int(rng.integers(0, r['v_len']))
            pts['pos_idx' if a <= f <= b else 'neg_idx'].append(f)
        old.append(pts)
    desc = rng.standard_normal((N, 256)).astype(np.float32) * rng.uniform(0.1, 2.0, size=(N, 1)).astype(np.float32)
    desc[[4, 19]] = 0.0
    desc[7] = np.nan
    return N, prop, data_gt, data_old, torch.from_numpy(desc).to(dev), desc


def _asked(new, old):
    n = lambda r: len(r[4]['pos_idx']) + len(r[4]['neg_idx'])
    return [i for i in range(len(new)) if n(new[i]) > n(old[i])]


def test_badge_select_is_the_sampler_from_the_origin(dev):
    from hual_amd import al, lib
    N, _, _, _, desc, x = _synth(dev)
    sel, picked, dist, mind = al.badge_select(desc, 12, seed=3)
    assert sel.dtype.kind == 'i' and len(sel) == len(set(sel.tolist())) == 12 and 7 not in sel
    assert not {4, 19} & set(sel.tolist())                                 # a certain sample sits on the origin: never drawn while others remain
    want = lib.kcenter_sample(desc, 12, seed=3, sample=True, origin=True)
    assert same_bits(picked.cpu().numpy(), want[0].cpu().numpy()) and same_bits(mind.cpu().numpy(), want[2].cpu().numpy())
    np.testing.assert_array_equal(sel, picked.cpu().numpy())
    np.testing.assert_array_equal(al.badge_select(desc, 12, seed=3)[0], sel)
    assert al.badge_select(desc, 12, seed=4)[0].tolist() != sel.tolist()
    # greedy from the origin: the largest gradient first
    first = al.badge_select(desc, 1, sample=False)[0]
    norms = np.where(np.isfinite(x).all(1), (x.astype(np.float64) ** 2).sum(1), -1)
    assert first.tolist() == [int(np.argmax(norms))]
    # the whole set: the zero rows come last, the NaN row never
    every = al.badge_select(desc, N, seed=3)[0]
    assert len(every) == N - 1 and sorted(every[-2:].tolist()) == [4, 19]
    around = al.badge_select(desc, N, seed=3, init=[0, 1, 2])[0]
    assert len(around) == N - 4 and not set(around.tolist()) & {0, 1, 2, 7}
    for bad in (dict(init=[N]), dict(init=[1, 1]), dict(seed=-1), dict(weight=np.ones(N - 1))):
        with pytest.raises(ValueError):
            al.badge_select(desc, 4, **bad)


def test_round_asks_the_badge_half(dev):
    from hual_amd import al
    N, prop, data_gt, data_old, desc, _ = _synth(dev)
    coff = al.get_coff('charades', 1)
    new0, d0 = al.update_labels(copy.deepcopy(data_old), data_gt, prop, coff, return_debug=True)
    new1, d1 = al.update_labels(copy.deepcopy(data_old), data_gt, prop, coff, return_debug=True, select_by='badge', descriptors=desc,
                                selection_seed=5)
    np.testing.assert_array_equal(d1['order'], d0['order'])
    sel = al.badge_select(desc, math.ceil(N / 2), seed=5)[0]
    assert sorted(_asked(new1, data_old)) == sorted(sel.tolist()) and len(sel) == 12
    np.testing.assert_array_equal(d1['kcenter_picked'], sel)
    assert sorted(d1) == sorted(list(d0) + ['kcenter_picked', 'kcenter_dist', 'cover_radius'])
    assert d1['kcenter_dist'].shape == (12,) and isinstance(d1['cover_radius'], float)
    # the default seed is 0; another seed asks another half
    new2 = al.update_labels(copy.deepcopy(data_old), data_gt, prop, coff, select_by='badge', descriptors=desc)
    assert sorted(_asked(new2, data_old)) == sorted(al.badge_select(desc, 12, seed=0)[0].tolist())
    # around the answered clips: none of the 12 samples that hold an active point is asked while others remain; the 12 others hold
    # one NaN row, which is never drawn: the half is filled from the ranking, best first
    new3, d3 = al.update_labels(copy.deepcopy(data_old), data_gt, prop, coff, return_debug=True, select_by='badge', descriptors=desc,
                                diversity_init='answered', selection_seed=5)
    answered = [i for i in range(N) if i % 2 == 0]
    drawn = al.badge_select(desc, 12, seed=5, init=answered)[0]
    assert sorted(drawn.tolist()) == [i for i in range(N) if i % 2 == 1 and i != 7]
    fill = [i for i in d3['order'].tolist() if i not in set(drawn.tolist())][0]
    assert sorted(_asked(new3, data_old)) == sorted(drawn.tolist() + [fill])
    # rank_by='egl': the records' own scalar, largest first
    egl = np.random.default_rng(2).uniform(0, 3, size=N)
    egl[5] = -1.0
    for p, v in zip(prop, egl):
        p['prop_egl'] = float(v)
    new4, d4 = al.update_labels(copy.deepcopy(data_old), data_gt, prop, coff, return_debug=True, rank_by='egl')
    np.testing.assert_array_equal(d4['order'], np.argsort(-egl, kind='stable'))
    assert d4['order'][-1] == 5 and sorted(_asked(new4, data_old)) == sorted(d4['order'][:12].tolist())
    np.testing.assert_array_equal(d4['egl'], egl)
    # the errors the round raises before anything is touched
    for kw in (dict(select_by='badge'), dict(select_by='badge', descriptors=desc[:5]), dict(selection_seed=1),
               dict(select_by='badge', descriptors=desc, selection_seed=-1)):
        mine = copy.deepcopy(data_old)
        with pytest.raises(ValueError):
            al.update_labels(mine, data_gt, prop, coff, **kw)
        assert mine == data_old


def test_round_without_the_switches_is_the_round_it_was(dev):
    from hual_amd import al
    N, prop, data_gt, data_old, _, _ = _synth(dev)
    coff = al.get_coff('charades', 1)
    for extra in ({}, dict(renew_by='posterior', observe_by='info_gain')):
        new0, d0 = al.update_labels(copy.deepcopy(data_old), data_gt, prop, coff, return_debug=True, **extra)
        new1, d1 = al.update_labels(copy.deepcopy(data_old), data_gt, prop, coff, return_debug=True, select_by=None, descriptors=None,
                                    diversity_init=None, selection_seed=None, **extra)
        assert new0 == new1 and list(d0) == list(d1)
        assert all(np.array_equal(d0[k], d1[k]) for k in d0 if k != 'updater')
        np.testing.assert_array_equal(d0['order'][:12], sorted(_asked(new0, data_old), key=list(d0['order']).index))
