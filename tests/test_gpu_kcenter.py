"""GPU: core-set clip selection - hual_kcenter_greedy against the float64 statement of its contract (tests/kcenter_ref.py),
hual_clip_mean_features against the float64 mean, and the places they land: DeviceDataset.clip_descriptors, al.diverse_select and
al.update_labels(select_by='kcenter').

The bars (from the contract's arithmetic, include/hual_seqpan.h; not tuned), u = 2^-24:
  lattice sets   features integers in [-8, 8], D <= 130, weights in {0, 1/4, 1/2, 1}: every float32 difference, square, sum (<= 130 *
                 256 < 2^24) and product is exact in any order, so all four outputs EQUAL the reference.
  regret         random sets, teacher-forced on the kernel's own earlier picks: the reference score of the kernel's pick lies within
                 2 (D + 4) u relative of the reference's best.  One rounding for the difference, one for the square, at most D - 1
                 for the additions: (D + 2) u per distance; one more for the weight: (D + 3) u per score; doubled because two scores
                 are compared (the bar keeps one u of slack per score).
  identity       the pick is the reference's first maximiser wherever the reference's runner-up lies more than that margin below;
                 gated at D = 130 (at least 95 % of the steps are then compared), printed at D = 1,024.
  values         mind and pick_dist within (D + 3) u relative of the reference; assign equal wherever the row's two nearest centers
                 differ by more than that.
  descriptors    |mean - float64 mean| <= T u mean_t |x| per entry (any float32 summation order of T terms, and the division);
                 unit rows within 4 ulp (2^-23) of norm 1."""
import copy
import math

import numpy as np
import pytest
import torch

import al_synth
import kcenter_ref as KR
from span_clip_util import _pads_intact, _sentinel

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
FILL, IFILL = 777.0, 777


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def run_kc(dev, x, n_select, weight=None, init=None, ld=None):
    """one selection into sentinel-filled, padded outputs -> dict of numpy arrays, after checking the memory around them; ld: the
    row stride x is laid out with on the device (the columns beyond D hold NaN: nothing may read them)"""
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
    got = lib.kcenter_select(xd, n_select, weight=wd, init=init, out=out)
    assert all(g is o for g, o in zip(got, out))
    torch.cuda.synchronize()
    for b, fill in zip(bufs, (IFILL, FILL, FILL, IFILL)):
        assert _pads_intact(b[1], b[2], fill)
    return dict(zip(('picked', 'pick_dist', 'mind', 'assign'), (o.cpu().numpy() for o in out)))


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


# ---------------------------------------------------------------------------------------------------------------- 1. exact lattice sets
def lattice(N, D, seed):
    """integer features in [-8, 8] with 7 duplicated rows (as many as N allows), weights from {0, 1/4, 1/2, 1}, the duplicates'
    weights equal to their source's for every other one: exact ties in score, in (score, w) and none"""
    g = np.random.default_rng(seed)
    x = g.integers(-8, 9, size=(N, D)).astype(np.float32)
    w = g.choice(np.array([0.0, 0.25, 0.5, 1.0], dtype=np.float32), size=N)
    for j in range(min(7, N - 1)):
        dst, src = (int(v) for v in g.choice(N, size=2, replace=False))
        x[dst] = x[src]
        if j % 2 == 0:
            w[dst] = w[src]
    return x, w


@pytest.mark.parametrize('N', [1, 2, 65, 300, 1031])
@pytest.mark.parametrize('D', [1, 4, 130])
def test_lattice_sets_equal_the_reference(dev, N, D):
    """N = 65, 300, 1031: 5, 19 and 65 workgroups of 16 rows, none a multiple of 16; ld = D + 3 takes the unaligned load path"""
    x, w = lattice(N, D, seed=1000 * N + D)
    g = np.random.default_rng(N + D)
    selects = sorted({1, math.ceil(N / 2), N})
    for n_init in sorted({0, min(1, N), min(5, N)}):
        init = g.choice(N, size=n_init, replace=False).tolist()
        ref = KR.greedy(x, N, w, init=init, snapshots=selects)
        for n_select in selects:
            for ld in (D, D + 3):
                r = run_kc(dev, x, n_select, w, init=init, ld=ld)
                what = (N, D, ld, n_select, n_init)
                np.testing.assert_array_equal(r['picked'], ref['picked'][:n_select], err_msg=str(what))
                np.testing.assert_array_equal(r['pick_dist'].astype(np.float64), ref['pick_dist'][:n_select], err_msg=str(what))
                mind, assign = ref['state'][n_select]
                np.testing.assert_array_equal(r['mind'].astype(np.float64), mind, err_msg=str(what))
                np.testing.assert_array_equal(r['assign'], assign, err_msg=str(what))
    if N >= 65:                                                  # all three keys decided picks somewhere in the last full selection
        st, by = KR.State(x, w, init=init), {'score': 0, 'weight': 0, 'index': 0}
        for c in ref['picked']:
            if c < 0:
                break
            score, el = st.scores()
            tie = el & (score == score[c])
            by['score' if tie.sum() == 1 else 'weight' if (tie & (st.w == st.w[c])).sum() == 1 else 'index'] += 1
            st.add(int(c))
        assert all(by.values()), by


# ---------------------------------------------------------------------------------------------------------------- 2. random sets
def forced(x, w, init, r, D):
    """teacher-forced walk along the kernel's picks -> (max regret, steps compared for identity, steps where the pick differed
    there, max relative error of pick_dist, the final State)"""
    margin = 2 * (D + 4) * U
    st = KR.State(x, w, init)
    regret, compared, differed, dist_err = 0.0, 0, 0, 0.0
    for s, c in enumerate(r['picked'].tolist()):
        score, el = st.scores()
        assert c >= 0 and el[c], (s, c)
        top = np.sort(score[el])[::-1]
        best, _ = st.best()
        regret = max(regret, (top[0] - score[c]) / top[0] if top[0] > 0 else 0.0)
        if len(top) == 1 or top[1] < top[0] * (1 - margin):
            compared += 1
            differed += int(c != best)
        want = st.mind[c]
        got = float(r['pick_dist'][s])
        dist_err = max(dist_err, 0.0 if want == got else abs(got - want) / want)
        st.add(c)
    return regret, compared, differed, dist_err, st


def check_values(st, x, r, D):
    """mind within (D + 3) u of the teacher-forced reference; assign equal wherever the two nearest centers differ by more"""
    bar = (D + 3) * U
    mind = r['mind'].astype(np.float64)
    err = float((np.abs(mind - st.mind) / np.maximum(st.mind, 1e-300)).max())
    x64 = np.asarray(x, dtype=np.float64)
    c = np.array(st.centers)
    d = (x64 ** 2).sum(1)[:, None] + (x64[c] ** 2).sum(1)[None, :] - 2.0 * x64 @ x64[c].T
    two = np.sort(d, axis=1)[:, :2]
    clear = two[:, 1] - two[:, 0] > bar * two[:, 1]
    assert clear.mean() > 0.9
    assert (r['assign'][clear] == st.assign[clear]).all()
    assert (r['assign'][c] == c).all()                           # a center is its own nearest center (no duplicates here)
    return err


@pytest.mark.parametrize('N', [300, 1031])
@pytest.mark.parametrize('weighted', [False, True])
def test_random_sets_follow_the_reference(dev, N, weighted):
    D = 130
    g = np.random.default_rng(7 * N + weighted)
    x = g.standard_normal((N, D)).astype(np.float32)
    w = g.uniform(0, 1, size=N).astype(np.float32) if weighted else None
    init = g.choice(N, size=3, replace=False).tolist() if weighted else []
    n_select = math.ceil(N / 2)
    r = run_kc(dev, x, n_select, w, init=init)
    regret, compared, differed, dist_err, st = forced(x, w, init, r, D)
    err = check_values(st, x, r, D)
    print('N %d D %d %s: max regret %.3e (bar %.3e); identity compared on %d of %d steps (%.1f %%), %d differ; max rel err mind %.3e, '
          'pick_dist %.3e (bar %.3e)' % (N, D, 'weighted' if weighted else 'unweighted', regret, 2 * (D + 4) * U, compared, n_select,
                                         100.0 * compared / n_select, differed, err, dist_err, (D + 3) * U))
    assert regret <= 2 * (D + 4) * U
    assert compared >= 0.95 * n_select and differed == 0
    assert err <= (D + 3) * U and dist_err <= (D + 3) * U


@pytest.mark.parametrize('weighted', [False, True])
def test_random_sets_at_1024_columns(dev, weighted):
    """the margin is wide here (8 to 45 % of unweighted steps are near-ties): the regret bar alone, the share compared is printed"""
    N, D = 300, 1024
    g = np.random.default_rng(11 + weighted)
    x = g.standard_normal((N, D)).astype(np.float32)
    w = g.uniform(0, 1, size=N).astype(np.float32) if weighted else None
    n_select = N // 2
    r = run_kc(dev, x, n_select, w)
    regret, compared, differed, dist_err, st = forced(x, w, [], r, D)
    err = check_values(st, x, r, D)
    print('N %d D %d %s: max regret %.3e (bar %.3e); identity compared on %.1f %% of the steps, %d differ; max rel err mind %.3e, '
          'pick_dist %.3e (bar %.3e)' % (N, D, 'weighted' if weighted else 'unweighted', regret, 2 * (D + 4) * U, 100.0 * compared / n_select,
                                         differed, err, dist_err, (D + 3) * U))
    assert regret <= 2 * (D + 4) * U
    assert err <= (D + 3) * U and dist_err <= (D + 3) * U


# ---------------------------------------------------------------------------------------------------------------- 3. edges
def test_rows_that_are_never_asked(dev):
    N, D = 65, 4
    x, w = lattice(N, D, seed=5)
    w[w == 0] = 0.25
    w[[3, 17, 40]] = -1.0
    w[[8, 64]] = np.nan
    r = run_kc(dev, x, N, w)
    ref = KR.greedy(x, N, w)
    np.testing.assert_array_equal(r['picked'], ref['picked'])
    assert not set(r['picked'].tolist()) & {3, 17, 40, 8, 64}
    assert (r['picked'][:N - 5] >= 0).all() and (r['picked'][N - 5:] == -1).all() and (r['pick_dist'][N - 5:] == -1.0).all()
    np.testing.assert_array_equal(r['mind'].astype(np.float64), ref['mind'])
    np.testing.assert_array_equal(r['assign'], ref['assign'])


def test_every_row_in_init(dev):
    N, D = 65, 4
    x, w = lattice(N, D, seed=6)
    init = np.random.default_rng(6).permutation(N).tolist()
    r = run_kc(dev, x, 9, w, init=init)
    assert (r['picked'] == -1).all() and (r['pick_dist'] == -1.0).all()
    ref = KR.greedy(x, 0, w, init=init)
    np.testing.assert_array_equal(r['mind'].astype(np.float64), ref['mind'])
    np.testing.assert_array_equal(r['assign'], ref['assign'])


def test_selecting_nothing_writes_nothing(dev):
    x, w = lattice(65, 4, seed=7)
    r = run_kc(dev, x, 0, w, init=[1, 2])
    assert r['picked'].shape == (0,) and (r['mind'] == FILL).all() and (r['assign'] == IFILL).all()


def test_a_nan_row_is_never_picked_and_changes_no_other_pick(dev):
    N, D = 300, 130
    x, w = lattice(N, D, seed=8)
    w[w == 0] = 0.25
    base = run_kc(dev, x, N - 1, w)
    assert (base['picked'] >= 0).all()
    ghost = int(base['picked'][0])                               # the row that would be picked first
    rest = np.delete(np.arange(N), ghost)
    want = run_kc(dev, x[rest], N - 1, w[rest])                  # the selection without that row
    xn = x.copy()
    xn[ghost] = np.nan
    r = run_kc(dev, xn, N, w)
    assert ghost not in r['picked'].tolist() and r['picked'][-1] == -1 and r['pick_dist'][-1] == -1.0
    np.testing.assert_array_equal(r['picked'][:-1], rest[want['picked']])
    np.testing.assert_array_equal(r['pick_dist'][:-1], want['pick_dist'])
    assert np.isnan(r['mind'][ghost]) and r['assign'][ghost] == -1
    np.testing.assert_array_equal(r['mind'][rest], want['mind'])
    ref = KR.greedy(xn, N, w)
    np.testing.assert_array_equal(r['picked'], ref['picked'])


def test_an_init_row_out_of_range_is_refused_on_the_host(dev):
    from hual_amd import lib
    x = torch.zeros(8, 4, device=dev)
    for init in ([8], [-1], [0, 0], torch.tensor([3, 9], dtype=torch.int32, device=dev)):
        with pytest.raises(ValueError):
            lib.kcenter_select(x, 2, init=init)
    with pytest.raises(ValueError):
        lib.kcenter_select(x, 9)


# ---------------------------------------------------------------------------------------------------------------- 4. determinism and capture
def test_second_call_and_graph_replay_return_equal_bits(dev):
    from hual_amd import lib
    N, D, n_select = 1031, 130, 64
    g = np.random.default_rng(21)
    x = g.standard_normal((N, D)).astype(np.float32)
    x[5] = x[900]
    w = g.uniform(0, 1, size=N).astype(np.float32)
    init = [17, 333]
    want = run_kc(dev, x, n_select, w, init=init)
    again = run_kc(dev, x, n_select, w, init=init)
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
        lib.kcenter_select(xd, n_select, weight=wd, init=init_d, out=outs(), workspace=ws, validate=False)      # (warm-up)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    out = outs()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        lib.kcenter_select(xd, n_select, weight=wd, init=init_d, out=out, workspace=ws, validate=False)
    for _ in range(2):
        for o in out:
            o.fill_(5)
        ws.fill_(255)                                            # (the workspace's contents are irrelevant on entry)
        graph.replay()
        torch.cuda.synchronize()
        for o, key in zip(out, ('picked', 'pick_dist', 'mind', 'assign')):
            assert same_bits(o.cpu().numpy(), want[key]), key


# ---------------------------------------------------------------------------------------------------------------- 5. descriptors
@pytest.mark.parametrize('vdim', [130, 1024])
def test_clip_mean_features(dev, vdim):
    from hual_amd import lib
    frames = [1, 2, 33, 70, 256]
    g = np.random.default_rng(vdim)
    bank = g.standard_normal((sum(frames), vdim)).astype(np.float32)
    off = np.concatenate([[0], np.cumsum(frames)]).astype(np.int64)
    bank[off[2]:off[3]] = 0.0                                    # the video of 33 frames: a zero row
    bank_d, off_d = torch.from_numpy(bank).to(dev), torch.from_numpy(off).to(dev)
    V = len(frames)
    outs = {}
    for normalize in (False, True):
        view, whole, pad = _sentinel((V, vdim), torch.float32, dev, FILL)
        got = lib.clip_mean_features(bank_d, off_d, normalize=normalize, out=view)
        torch.cuda.synchronize()
        assert got is view and _pads_intact(whole, pad, FILL)
        outs[normalize] = view.cpu().numpy()
        again = lib.clip_mean_features(bank_d, off_d, normalize=normalize)
        assert same_bits(again.cpu().numpy(), outs[normalize])
    worst = 0.0
    for v, T in enumerate(frames):
        rows = bank[off[v]:off[v + 1]].astype(np.float64)
        bound = T * U * np.abs(rows).mean(axis=0)
        d = np.abs(outs[False][v].astype(np.float64) - rows.mean(axis=0))
        assert (d <= bound).all(), (v, T, float((d - bound).max()))
        worst = max(worst, float((d / np.maximum(bound, 1e-300)).max()))
    norms = np.sqrt((outs[True].astype(np.float64) ** 2).sum(axis=1))
    print('vdim %d: max |mean - ref| / bound = %.3f; max |norm - 1| = %.2f ulp (bar 4)' % (vdim, worst, float(np.abs(np.delete(norms, 2) - 1).max() / 2.0 ** -23)))
    assert (outs[True][2] == 0).all() and (outs[False][2] == 0).all()
    assert (np.abs(np.delete(norms, 2) - 1.0) <= 4 * 2.0 ** -23).all()
    unit = outs[False].astype(np.float64) / np.maximum(np.sqrt((outs[False].astype(np.float64) ** 2).sum(axis=1)), 1e-300)[:, None]
    assert np.abs(outs[True] - unit).max() <= 4 * 2.0 ** -23


def _synth(dev):
    """al_synth.make_trainset(N = 24, 8 videos) as a DeviceDataset, random logits as records, and truthful answers of earlier rounds
    on every other sample"""
    from hual_amd import al
    from hual_amd.dataset import DeviceDataset
    N = 24
    recs, vis, data_gt, data_old = al_synth.make_trainset(N, 8, 16, 40, seed=31)
    ds = DeviceDataset(recs, vis, device=dev)
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
    return N, ds, recs, vis, prop, data_gt, data_old


def test_dataset_descriptors(dev):
    N, ds, recs, vis, _, _, _ = _synth(dev)
    desc = ds.clip_descriptors()
    raw = ds.clip_descriptors(normalize=False).cpu().numpy()
    assert desc.dtype == torch.float32 and tuple(desc.shape) == (N, 16) and desc.is_contiguous()
    d = desc.cpu().numpy()
    shared = 0
    for i in range(N):
        f = vis[recs[i]['vid']].astype(np.float64)
        assert (np.abs(raw[i] - f.mean(axis=0)) <= len(f) * U * np.abs(f).mean(axis=0)).all()
        for j in range(i):
            if recs[i]['vid'] == recs[j]['vid']:
                shared += 1
                assert same_bits(d[i], d[j]) and same_bits(raw[i], raw[j])
    assert shared >= 8
    assert (np.abs(np.sqrt((d.astype(np.float64) ** 2).sum(1)) - 1) <= 4 * 2.0 ** -23).all()


# ---------------------------------------------------------------------------------------------------------------- 6. the round
def _asked(new, old):
    n = lambda r: len(r[4]['pos_idx']) + len(r[4]['neg_idx'])
    return [i for i in range(len(new)) if n(new[i]) > n(old[i])]


def test_diverse_select_is_the_reference_on_rank_weights(dev):
    from hual_amd import al
    N, ds, recs, _, _, _, _ = _synth(dev)
    desc = ds.clip_descriptors()
    order = np.random.default_rng(3).permutation(N)
    x = desc.cpu().numpy()
    picks = al.diverse_select(desc, order, 12)
    assert picks.dtype.kind == 'i' and picks[0] == order[0] and len(set(picks.tolist())) == 12
    # nv videos, 24 samples: the first nv picks are nv different videos (a duplicate's score is an exact zero), each its video's
    # best-ranked sample (the second key)
    nv = len({r['vid'] for r in recs})
    assert 4 <= nv <= 8
    rank = {int(i): k for k, i in enumerate(order)}
    first = picks[:nv].tolist()
    assert len({recs[i]['vid'] for i in first}) == nv
    for i in first:
        assert all(rank[i] < rank[j] for j in range(N) if j != i and recs[j]['vid'] == recs[i]['vid'])
    st = KR.State(x, al.rank_weights(order))
    for s, c in enumerate(picks.tolist()):                       # teacher-forced: no other row scores more than the margin above the pick
        score, el = st.scores()
        assert el[c] and score[c] >= score[el].max() * (1 - 2 * (16 + 4) * U), s
        st.add(c)
    plain = al.diverse_select(desc, order, nv, weighted=False)
    assert plain[0] == order[0] and len({recs[i]['vid'] for i in plain.tolist()}) == nv
    around = al.diverse_select(desc, order, N, init=first)
    assert len(around) == N - nv and not set(around.tolist()) & set(first)
    np.testing.assert_array_equal(al.diverse_select(desc, order, 12), picks)
    for bad in (dict(order=order[:-1]), dict(order=np.zeros(N, dtype=np.int64)), dict(init=[N]), dict(init=[1, 1])):
        with pytest.raises(ValueError):
            al.diverse_select(desc, **dict(dict(order=order, n_select=4), **bad))


def test_round_asks_the_diverse_half(dev):
    from hual_amd import al
    N, ds, recs, _, prop, data_gt, data_old = _synth(dev)
    desc = ds.clip_descriptors()
    coff = al.get_coff('charades', 1)
    new0, d0 = al.update_labels(copy.deepcopy(data_old), data_gt, prop, coff, return_debug=True)
    new1, d1 = al.update_labels(copy.deepcopy(data_old), data_gt, prop, coff, return_debug=True, select_by='kcenter', descriptors=desc)
    np.testing.assert_array_equal(d1['order'], d0['order'])
    picks = al.diverse_select(desc, d1['order'], math.ceil(N / 2))
    assert sorted(_asked(new1, data_old)) == sorted(picks.tolist()) and len(picks) == 12
    np.testing.assert_array_equal(d1['kcenter_picked'], picks)
    assert sorted(d1) == sorted(list(d0) + ['kcenter_picked', 'kcenter_dist', 'cover_radius'])
    assert d1['kcenter_dist'].shape == (12,) and d1['kcenter_dist'][0] == np.inf and isinstance(d1['cover_radius'], float)
    vids = lambda ids: len({recs[i]['vid'] for i in ids})
    assert vids(picks.tolist()) == vids(range(N)) >= vids(_asked(new0, data_old))      # every video is asked about
    # around the answered clips: none of the 12 samples that hold an active point is asked while the 12 others remain
    new2, d2 = al.update_labels(copy.deepcopy(data_old), data_gt, prop, coff, return_debug=True, select_by='kcenter', descriptors=desc,
                                diversity_init='answered')
    answered = [i for i in range(N) if i % 2 == 0]
    assert sorted(_asked(new2, data_old)) == [i for i in range(N) if i % 2 == 1]
    np.testing.assert_array_equal(d2['kcenter_picked'], al.diverse_select(desc, d2['order'], 12, init=answered))
    # the errors the round raises before anything is touched
    for kw in (dict(select_by='kcenter'), dict(descriptors=desc), dict(select_by='kcenter', descriptors=desc[:5]), dict(select_by='topk', descriptors=desc)):
        mine = copy.deepcopy(data_old)
        with pytest.raises(ValueError):
            al.update_labels(mine, data_gt, prop, coff, **kw)
        assert mine == data_old


def test_round_without_the_switch_is_the_round_it_was(dev):
    from hual_amd import al
    N, ds, _, _, prop, data_gt, data_old = _synth(dev)
    coff = al.get_coff('charades', 1)
    for extra in ({}, dict(renew_by='posterior', observe_by='info_gain')):
        new0, d0 = al.update_labels(copy.deepcopy(data_old), data_gt, prop, coff, return_debug=True, **extra)
        new1, d1 = al.update_labels(copy.deepcopy(data_old), data_gt, prop, coff, return_debug=True, select_by=None, descriptors=None,
                                    diversity_init=None, **extra)
        assert new0 == new1 and list(d0) == list(d1)
        assert all(np.array_equal(d0[k], d1[k]) for k in d0 if k != 'updater')
        np.testing.assert_array_equal(d0['order'][:12], sorted(_asked(new0, data_old), key=list(d0['order']).index))
