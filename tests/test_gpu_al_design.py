"""GPU: hual_al_design (question sets for an annotator who is not in the loop: M frames per clip in one launch) against the float64
enumeration of its contract (tests/al_design_ref.py) - forced to the reference's whole design, teacher-forced step by step, and
free-running -, against hual_al_query in its first column, its edge rows and the memory it must not touch, and the three places it
lands: LabelUpdater.design, al.update_labels(questions_at_once=) and al.run_round(questions_at_once=).

The bars are the family's (tests/test_gpu_al_query.py): info and post_entropy within 5e-5 bits of the enumeration - the first term of
info is hual_al_query's float32 gain, every later term a float64 sum whose only float32 inputs are p_s and p_e -; a chosen frame,
evaluated by the enumeration, within 1e-5 bits of the enumeration's best (the near-tie threshold), and the reference's own frame
wherever its runner-up lies more than that below; the stop decision equal wherever the best marginal gain is not within 1e-5 bits of
min_gain.  No case is excused by index."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import al_design_ref as D
import al_query_ref as Q
import al_session_ref as S
from test_gpu_al_query import _answers, _pads_intact, _prof, _round_set, _sentinel, make_set, pad_logits

pytestmark = pytest.mark.gpu

INFO_BAR, ENT_BAR, NEAR = 5e-5, 5e-5, D.NEAR
MIN_GAIN = 0.02               # the teacher-forced comparison's: a design with nothing left to learn (gain 0) is 0.02 bits away, so it is compared
FILL = {'frames': -7, 'info': 777.0, 'post_entropy': 777.0, 'n_design': -7, 'stop_reason': -7}      # no design holds these
NAMES = ('frames', 'info', 'post_entropy', 'n_design', 'stop_reason')


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def _i32(dev, x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).to(dev)


def _specs(N, M):
    i32, f32 = torch.int32, torch.float32
    return [((N, M), i32), ((N, M), f32), ((N,), f32), ((N,), i32), ((N,), i32)]


def run_design(dev, s, e, vlen, tlen, aps, mmax, sel=None, forced=None, min_gain=0.0, stop_entropy=-1.0, selected=None):
    """one launch into sentinel-filled outputs -> dict of numpy arrays, after checking the memory around them, that the rows outside
    `selected` (default: all) keep their fill and that every slot of a selected row was written"""
    from hual_amd import lib
    N, ld = s.shape
    aset, keep = make_set(dev, vlen, tlen, aps, ld)
    bufs = [_sentinel(shape, dt, dev, FILL[k]) for k, (shape, dt) in zip(NAMES, _specs(N, mmax))]
    out = tuple(b[0] for b in bufs)
    got = lib.al_design(aset, s, e, np.asarray(tlen), mmax, sel=_i32(dev, sel), forced=_i32(dev, forced), min_gain=min_gain,
                        stop_entropy=stop_entropy, out=out)
    assert all(a is b for a, b in zip(got, out))
    torch.cuda.synchronize()
    rows = np.zeros(N, dtype=bool)
    rows[list(range(N)) if selected is None else list(selected)] = True
    r = {}
    for k, b in zip(NAMES, bufs):
        assert _pads_intact(b[1], b[2], FILL[k]), k
        r[k] = b[0].cpu().numpy()
        assert (r[k][~rows] == FILL[k]).all(), k                      # rows that are not selected keep their fill
        assert not (r[k][rows] == FILL[k]).any(), k                   # every slot of a selected row was written
    for n in np.flatnonzero(rows):                                    # unused slots hold -1
        nd = int(r['n_design'][n])
        assert 0 <= nd <= mmax and (r['frames'][n, nd:] == -1).all() and (r['info'][n, nd:] == -1).all()
        assert (r['frames'][n, :nd] >= 0).all()
    return r


def run_query(dev, s, e, vlen, tlen, aps):
    from hual_amd import lib
    aset, keep = make_set(dev, vlen, tlen, aps, s.shape[1])
    out = lib.al_query(aset, s, e, np.asarray(tlen), frames=False)
    torch.cuda.synchronize()
    return dict(query_point=out[2].cpu().numpy(), query_gain=out[3].cpu().numpy(), post_entropy=out[4].cpu().numpy())


def assert_same_design(got, want, rows=None):
    for k in NAMES:
        a, b = got[k], want[k]
        if rows is not None:
            a, b = a[rows], b[rows]
        if a.dtype == np.float32:
            a, b = a.view(np.int32), b.view(np.int32)                 # bit for bit
        np.testing.assert_array_equal(a, b, err_msg=k)


_LOGITS = {}


def case_logits(dev, T, extra=7):
    if (T, extra) not in _LOGITS:
        c = Q.case(T)
        _LOGITS[(T, extra)] = (pad_logits(dev, c['s'], T + extra, 1), pad_logits(dev, c['e'], T + extra, 2))
    return _LOGITS[(T, extra)]


def sizes(T):
    return (1, 6, 16) if T in (33, 70) else (1, 6)


def forced_of(designs, M, upto=None):
    """int32 [16, M]: per row the first `upto` (default: all) frames of its reference design, -1 behind them and on rows without one"""
    f = np.full((Q.N_ROWS, M), -1, dtype=np.int32)
    for n, d in designs.items():
        k = d['n_design'] if upto is None else min(upto, d['n_design'])
        f[n, :k] = d['frames'][:k]
    return f


CASES = [(T, h) for T in Q.TS for h in Q.HISTORIES]


# ---------------------------------------------------------------------------------------------------------------- 1. forced to the reference's design
@pytest.mark.parametrize('T,h', CASES)
def test_forced_to_the_references_whole_design(dev, T, h):
    c = Q.case(T)
    s, e = case_logits(dev, T)
    vlen, tlen, rows = c['vlen'].numpy(), [T] * Q.N_ROWS, list(D.rows_of(T))
    worst = dict(info=0.0, ent=0.0)
    placed = 0
    for M in sizes(T):
        ref = {n: D.case_design(T, h, n, M) for n in rows}
        forced = forced_of(ref, M)
        got = run_design(dev, s, e, vlen, tlen, c['aps'][h], M, sel=rows, forced=forced, selected=rows)
        for n in rows:
            d, nd = ref[n], ref[n]['n_design']
            assert got['n_design'][n] >= nd
            np.testing.assert_array_equal(got['frames'][n, :nd], forced[n, :nd])
            if nd:
                worst['info'] = max(worst['info'], float(np.abs(got['info'][n, :nd].astype(np.float64) - np.array(d['info'])).max()))
            worst['ent'] = max(worst['ent'], abs(float(got['post_entropy'][n]) - d['post_entropy']))
            placed += nd
    print('T=%d answers=%d: max |info - enumeration| = %.3e bits (bar %.0e), |post_entropy - enumeration| = %.3e bits (bar %.0e); '
          '%d frames' % (T, h, worst['info'], INFO_BAR, worst['ent'], ENT_BAR, placed))
    assert worst['info'] <= INFO_BAR and worst['ent'] <= ENT_BAR and (placed > 0 or T == 2)


# ---------------------------------------------------------------------------------------------------------------- 2. teacher-forced choice
@pytest.mark.parametrize('T,h', CASES)
def test_teacher_forced_choice_and_stop(dev, T, h):
    c = Q.case(T)
    s, e = case_logits(dev, T)
    vlen, tlen, rows = c['vlen'].numpy(), [T] * Q.N_ROWS, list(D.rows_of(T))
    Mx = sizes(T)[-1]
    ref = {n: D.case_design(T, h, n, Mx, MIN_GAIN) for n in rows}
    lost, chosen, same, ties, stops, near_stop = 0.0, 0, 0, 0, 0, 0
    for m in range(Mx):                                               # the decision at step m, on the reference's first m frames
        live = [n for n in rows if m in ref[n]['cand']]
        if not live:
            break
        got = run_design(dev, s, e, vlen, tlen, c['aps'][h], m + 1, sel=live, forced=forced_of(ref, m + 1, upto=m), min_gain=MIN_GAIN,
                         selected=live)
        for n in live:
            d = ref[n]
            cand, base, best = d['cand'][m], d['base'][m], d['best'][m]
            np.testing.assert_array_equal(got['frames'][n, :m], d['frames'][:m])
            placed = int(got['n_design'][n]) == m + 1
            if abs(best - MIN_GAIN) > NEAR:                           # the stop decision
                assert placed == (best > MIN_GAIN), (n, m, best)
                assert int(got['stop_reason'][n]) == (D.BUDGET if placed else D.GAIN)
                stops += 1
            else:
                near_stop += 1
            if not placed:
                continue
            f = int(got['frames'][n, m])
            assert 0 <= f < int(c['v'][n])
            lost = max(lost, float(cand.max() - cand[f]))             # the kernel's frame, evaluated by the enumeration
            chosen += 1
            first = int(np.argmax(cand))
            others = np.delete(cand, first)
            if len(others) == 0 or cand[first] - others.max() > NEAR:
                assert f == first, (n, m, f, first)
                same += 1
            else:
                ties += 1
            assert abs(float(got['info'][n, m]) - float(cand[f])) <= INFO_BAR
    print('T=%d answers=%d: enumerated information lost at the chosen frame = %.3e bits (bar %.0e) over %d choices; %d equal the '
          'reference\'s frame, %d had a runner-up within %.0e bits; %d stop decisions compared, %d near min_gain'
          % (T, h, lost, NEAR, chosen, same, ties, NEAR, stops, near_stop))
    assert lost <= NEAR and stops > 0 and (chosen > 0 or T == 2)


# ---------------------------------------------------------------------------------------------------------------- 3. free-running
@pytest.mark.parametrize('T,h', CASES)
def test_free_running_design(dev, T, h):
    c = Q.case(T)
    s, e = case_logits(dev, T)
    vlen, tlen, rows = c['vlen'].numpy(), [T] * Q.N_ROWS, list(D.rows_of(T))
    worst, lengths = 0.0, []
    for M in sizes(T):
        got = run_design(dev, s, e, vlen, tlen, c['aps'][h], M)
        again = run_design(dev, s, e, vlen, tlen, c['aps'][h], M)
        assert_same_design(again, got)                                # a second launch gives equal bits
        fed = run_design(dev, s, e, vlen, tlen, c['aps'][h], M, forced=got['frames'])
        assert_same_design(fed, got)                                  # the design fed back as forced returns itself
        same_length = 0
        for n in rows:
            row, nd = D.case_row(T, h, n), int(got['n_design'][n])
            frames = [int(f) for f in got['frames'][n, :nd]]
            assert len(set(frames)) == nd and not set(frames) & row.answered
            info = got['info'][n, :nd].astype(np.float64)
            assert (np.diff(info) >= 0).all() and (info <= np.minimum(np.arange(1, nd + 1), row.H) + INFO_BAR).all()
            for k in range(nd):
                worst = max(worst, abs(row.info(frames[:k + 1]) - info[k]))
            assert int(got['stop_reason'][n]) == (D.BUDGET if nd == M else D.GAIN)
            # as long as the enumeration's own greedy design: where one of the two goes on, its further frames carry next to nothing
            ref = D.case_design(T, h, n, M)
            k = min(nd, ref['n_design'])
            same_length += nd == ref['n_design']
            beyond = ref['info'][-1] - (ref['info'][k - 1] if k else 0.0) if ref['info'] else 0.0
            assert row.info(frames) - row.info(frames[:k]) <= NEAR and beyond <= NEAR, (n, M, nd, ref['n_design'])
        assert same_length > 0
        lengths.append('%d of %d at M = %d' % (same_length, len(rows), M))
    print('T=%d answers=%d: max |info - enumeration at the kernel\'s frames| = %.3e bits (bar %.0e); designs as long as the enumeration\'s: %s'
          % (T, h, worst, INFO_BAR, ', '.join(lengths)))
    assert worst <= INFO_BAR


# ---------------------------------------------------------------------------------------------------------------- 4. column 0 is the query
@pytest.mark.parametrize('tilted', [False, True])
@pytest.mark.parametrize('T', Q.TS)
def test_column_zero_is_the_query(dev, T, tilted):
    from hual_amd import lib
    c = Q.case(T)
    s, e = case_logits(dev, T)
    vlen, tlen = c['vlen'].numpy(), [T] * Q.N_ROWS
    for h in ('flipped3',) if tilted else Q.HISTORIES:
        aps = S.start_list(T, h) if tilted else c['aps'][h]
        if tilted:                                                    # eps = 0.1 on answers flipped at rate 0.3; the set without answers
            aset, keep = make_set(dev, vlen, tlen, aps, T + 7)
            s, e, _ = lib.al_noisy_tilt(aset, s, e, np.asarray(tlen), 0.1)
            aps = [[] for _ in range(Q.N_ROWS)]
        q = run_query(dev, s, e, vlen, tlen, aps)
        for M in sizes(T):
            got = run_design(dev, s, e, vlen, tlen, aps, M)
            np.testing.assert_array_equal(got['post_entropy'].view(np.int32), q['post_entropy'].view(np.int32))
            asks = q['query_gain'] > 0
            assert (got['n_design'] > 0).tolist() == asks.tolist()
            np.testing.assert_array_equal(got['frames'][asks, 0], q['query_point'][asks])
            np.testing.assert_array_equal(got['info'][asks, 0].view(np.int32), q['query_gain'][asks].view(np.int32))
            assert asks.any() or T == 2


# ---------------------------------------------------------------------------------------------------------------- 5. edges
def _edge_set(dev):
    """seven rows of case(33), ld = 40: 0 plain | 1 a NaN logit | 2 v = 1 | 3 contradictory answers | 4 answered at 5 (neg) and 20
    (pos) | 5 v = 20 | 6 plain"""
    c = Q.case(33)
    pick = [0, 1, 8, 2, 3, 4, 5]
    s, e = c['s'][pick].clone(), c['e'][pick].clone()
    s[1, 2] = float('nan')
    vlen = c['vlen'].numpy()[pick].copy()
    assert vlen[2] == 1
    vlen[5] = 20
    aps = [[], [], [], [(5, True), (9, True), (7, False)], [(5, False), (20, True)], [], []]
    return pad_logits(dev, s, 40, 3), pad_logits(dev, e, 40, 4), vlen, [33] * 7, aps


def test_edge_rows(dev):
    s, e, vlen, tlen, aps = _edge_set(dev)
    got = run_design(dev, s, e, vlen, tlen, aps, 6)
    np.testing.assert_array_equal(got['stop_reason'][1:4], [D.POISONED, D.GAIN, D.CONTRADICTORY])
    np.testing.assert_array_equal(got['n_design'][1:4], [0, 0, 0])
    assert got['post_entropy'][1] == -1.0 and abs(got['post_entropy'][2]) <= ENT_BAR and got['post_entropy'][3] == -1.0
    assert got['n_design'][0] == 6 and got['stop_reason'][0] == D.BUDGET
    assert not set(got['frames'][4, :got['n_design'][4]].tolist()) & {5, 20} and (got['frames'][5, :got['n_design'][5]] < 20).all()
    # stop_entropy: the expected entropy left, post_entropy - info, ends the design
    H = got['post_entropy'].astype(np.float64)
    bar = float(H[0] - 0.5 * (got['info'][0, 1] + got['info'][0, 2]))  # between the second and the third frame of row 0
    early = run_design(dev, s, e, vlen, tlen, aps, 6, stop_entropy=bar)
    assert early['stop_reason'][0] == D.ENTROPY and early['n_design'][0] == 3
    np.testing.assert_array_equal(early['frames'][0, :3], got['frames'][0, :3])
    assert H[0] - early['info'][0, 2] <= bar < H[0] - early['info'][0, 1]
    np.testing.assert_array_equal(early['stop_reason'][1:4], [D.POISONED, D.ENTROPY, D.CONTRADICTORY])
    # min_gain ends it with _GAIN, before the budget
    gains = np.diff(np.concatenate([[0.0], got['info'][0].astype(np.float64)]))
    stop = run_design(dev, s, e, vlen, tlen, aps, 6, min_gain=float(0.5 * (gains[2] + gains[3])))
    assert stop['stop_reason'][0] == D.GAIN and 1 <= stop['n_design'][0] < 6
    # sel: a subset, with a repeated id and ids outside the set
    part = run_design(dev, s, e, vlen, tlen, aps, 6, sel=[5, 0, 77, 0, -3, 2], selected=[0, 2, 5])
    assert_same_design(part, got, rows=[0, 2, 5])


def test_forced_frames(dev):
    s, e, vlen, tlen, aps = _edge_set(dev)
    free = run_design(dev, s, e, vlen, tlen, aps, 6)
    forced = np.full((7, 6), -1, dtype=np.int32)
    forced[0, :5] = [4, 99, 12, 33, 4]                                # 99 and 33 lie outside [0, v): ignored; 4 repeats: 0 bits, stays
    forced[4, :3] = [5, 20, 25]                                       # 5 and 20 are answered: 0 bits, they stay
    forced[5, :2] = [20, 3]                                           # v = 20: frame 20 is outside
    forced[6, :3] = [-1, 9, 9]                                        # -1 ends the prefix at once
    forced[1, :2] = [3, 4]                                            # a poisoned row places nothing
    got = run_design(dev, s, e, vlen, tlen, aps, 6, forced=forced)
    np.testing.assert_array_equal(got['frames'][0, :3], [4, 12, 4])
    assert got['info'][0, 2] == got['info'][0, 1] > got['info'][0, 0] > 0 and got['n_design'][0] == 6
    assert 4 not in got['frames'][0, 3:].tolist() and 12 not in got['frames'][0, 3:].tolist()
    np.testing.assert_array_equal(got['frames'][4, :3], [5, 20, 25])
    assert got['info'][4, 0] == 0.0 and got['info'][4, 1] == 0.0 and got['info'][4, 2] > 0
    assert got['frames'][5, 0] == 3 and (got['frames'][5, :got['n_design'][5]] < 20).all()
    assert_same_design(got, free, rows=[1, 2, 3, 6])
    row = D.Row(Q.case(33)['ps'][0], Q.case(33)['pe'][0], 33, [])
    assert abs(row.info([4, 12, 4]) - float(got['info'][0, 2])) <= INFO_BAR
    for k in range(6):
        assert abs(row.info([int(f) for f in got['frames'][0, :k + 1]]) - float(got['info'][0, k])) <= INFO_BAR
    row4 = D.Row(Q.case(33)['ps'][3], Q.case(33)['pe'][3], int(vlen[4]), aps[4])
    for k in range(int(got['n_design'][4])):
        assert abs(row4.info([int(f) for f in got['frames'][4, :k + 1]]) - float(got['info'][4, k])) <= INFO_BAR


def test_a_row_longer_than_256_frames_is_poisoned_and_argument_errors(dev):
    """tlen is device memory, so the C entry point cannot refuse it (lib.al_design does, on the host): the raw call"""
    from hual_amd import lib
    c = Q.case(33)
    N, ld, M = 2, 300, 4
    s = pad_logits(dev, c['s'][:2], ld, 5)
    e = pad_logits(dev, c['e'][:2], ld, 6)
    aset, keep = make_set(dev, [300, 33], [300, 33], [[], []], ld)
    with pytest.raises(lib.HualError, match='256'):
        lib.al_design(aset, s, e, np.array([300, 33]), M)
    bufs = [_sentinel(shape, dt, dev, FILL[k]) for k, (shape, dt) in zip(NAMES, _specs(N, M))]
    L = lib.load()

    def raw(mmax=M, min_gain=0.0, stop_entropy=-1.0, drop=None):
        o = [None if i == drop else lib.ptr(b[0]) for i, b in enumerate(bufs)]
        return L.hual_al_design(ctypes.byref(aset), lib.ptr(s), lib.ptr(e), None, N, mmax, None, min_gain, stop_entropy, *o, lib.stream_ptr())
    assert raw() == 0
    torch.cuda.synchronize()
    r = {k: b[0].cpu().numpy() for k, b in zip(NAMES, bufs)}
    assert all(_pads_intact(b[1], b[2], FILL[k]) for k, b in zip(NAMES, bufs))
    assert r['stop_reason'][0] == D.POISONED and r['n_design'][0] == 0 and (r['frames'][0] == -1).all() and (r['info'][0] == -1).all()
    assert r['stop_reason'][1] == D.BUDGET and r['n_design'][1] == M
    for bad in (dict(mmax=0), dict(mmax=17), dict(min_gain=-1.0), dict(min_gain=float('nan')), dict(stop_entropy=float('nan')),
                dict(drop=0), dict(drop=4)):
        assert raw(**bad) < 0, bad
    aset2, keep2 = make_set(dev, [33, 33], [33, 33], [[], []], ld)
    for kw in (dict(mmax=0), dict(mmax=17), dict(min_gain=-0.1), dict(forced=torch.zeros(2, 3, dtype=torch.int32, device=dev)),
               dict(sel=torch.zeros(0, dtype=torch.int32, device=dev))):
        args = dict(mmax=4)
        args.update(kw)
        with pytest.raises(lib.HualError):
            lib.al_design(aset2, s, e, np.array([33, 33]), args.pop('mmax'), **args)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- 6. the updater, the label update
def _updater(RS):
    from hual_amd import al
    return al.LabelUpdater(RS['prop'], [[] for _ in range(RS['N'])])


@pytest.mark.parametrize('noise', [None, 0.1])
def test_label_updater_design(dev, noise):
    from hual_amd import lib
    RS = _round_set()
    N = RS['N']
    up = _updater(RS)
    lists = [[(3, False)] if i % 3 == 0 else [] for i in range(N)]
    up.set_active_points(lists)
    sel = np.arange(0, N, 2)
    if noise is not None:
        up.tilt(noise)                                                # (made once: the design launch is then the only launch)
    (frames, nd), launches = _prof(lambda: up.design(3, noise=noise, sel=sel))
    assert sum(launches.values()) == 1 and 'al_design' in list(launches)[0], launches
    assert up.aps is lists and (noise is None or up.tilt_eps == float(np.float32(noise)))      # nothing is installed, the tilt stands
    assert (frames[1::2] == -1).all() and (up.design_stop.cpu().numpy()[1::2] == -1).all() and (nd[sel] >= 1).any()
    up.query(noise=noise)
    qp, h = up.query_point.cpu().numpy(), up.post_entropy.cpu().numpy()
    asks = nd > 0
    np.testing.assert_array_equal(frames[asks, 0], qp[asks])
    np.testing.assert_array_equal(up.design_entropy.cpu().numpy()[sel].view(np.int32), h[sel].view(np.int32))
    if noise is None:                                                 # (under noise query_gain is the noisy answer's: another number)
        np.testing.assert_array_equal(up.design_info.cpu().numpy()[asks, 0].view(np.int32), up.query_gain.cpu().numpy()[asks].view(np.int32))
    # a hand-made grid, scored: the forced frames come back with their information
    grid = np.tile(np.array([[2, 6, 10]], dtype=np.int64), (N, 1))
    g_frames, g_nd = up.design(3, noise=noise, forced=grid)
    live = (g_nd == 3) & (up.vlen_h > 10)                             # (a clip of at most 10 frames ignores the grid's last)
    assert live.any() and (g_frames[live] == grid[live]).all()
    grid_info = up.design_info.cpu().numpy()
    _, free_nd = up.design(3, noise=noise)
    free_info = up.design_info.cpu().numpy()
    both = live & (free_nd == 3)
    assert both.any() and (free_info[both, 0] >= grid_info[both, 0]).all()      # the greedy's first frame is the best single frame
    for bad in (dict(max_points=0), dict(max_points=17), dict(max_points=3, min_gain=-1.0), dict(max_points=3, stop_entropy=-1.0),
                dict(max_points=3, sel=np.array([N])), dict(max_points=3, forced=np.zeros((N, 4)))):
        with pytest.raises(ValueError):
            up.design(**bad)
    z = torch.zeros(2, N, up.ld, device=up.dev)
    up.set_ensemble(z, z.clone())
    with pytest.raises(lib.HualError, match='no ensemble form'):
        up.design(3)


@pytest.mark.parametrize('noise,flip', [(None, None), (0.1, 0.3), (None, 0.3)])
def test_update_labels_with_three_questions_at_once(dev, noise, flip):
    from hual_amd import al
    RS = _round_set()
    N, prop, coff, M = RS['N'], RS['prop'], al.get_coff('charades', 1), 3
    kw = dict(observe_by='info_gain', answer_noise=noise)

    def flipper():
        return None if flip is None else (flip, np.random.default_rng(21))
    (new, d), launches = _prof(lambda: al.update_labels(copy.deepcopy(RS['data_old']), RS['data_gt'], prop, coff, return_debug=True,
                                                        annotator_flip=flipper(), questions_at_once=M, **kw))
    assert sum(v for k, v in launches.items() if 'al_design' in k) == 1 and not any('al_session' in k for k in launches), launches
    base, d1 = al.update_labels(copy.deepcopy(RS['data_old']), RS['data_gt'], prop, coff, return_debug=True, **kw)
    for key in ('order', 'uncert_video', 'observe', 'gt_idx', 'old_idx', 'query_point', 'observe_used'):
        np.testing.assert_array_equal(d[key], d1[key])
    sel, gt, observe = d1['order'][:(N + 1) // 2], d1['gt_idx'], d1['observe']
    flips = np.zeros((N, M), dtype=bool)
    if flip is not None:
        rng = np.random.default_rng(21)
        for i in sel:
            for k in range(M):
                flips[i, k] = rng.random() < flip
    # the restatement: one design of the selected samples that have a gain, on the answers of the earlier rounds (none)
    ref = _updater(RS)
    ref.query(noise=noise)
    has_gain = ref.query_gain.cpu().numpy() > 0
    designed = np.array([i for i in sel if has_gain[i]])
    frames, nd = ref.design(M, noise=noise, sel=designed)
    lists = [[] for _ in range(N)]
    for i in sel:
        if has_gain[i]:
            lists[i] = [(int(t), bool(gt[i, 0] <= t <= gt[i, 1]) != bool(flips[i, k])) for k, t in enumerate(frames[i, :nd[i]])]
        else:
            lists[i] = [(int(observe[i]), bool(gt[i, 0] <= observe[i] <= gt[i, 1]) != bool(flips[i, 0]))]
    ans = _answers(new, RS['data_old'])
    for i in range(N):
        pos, neg = [f for f, p in lists[i] if p], [f for f, p in lists[i] if not p]
        assert ans[i] == [(f, True) for f in pos] + [(f, False) for f in neg], i
    assert d['updater'].aps == lists
    np.testing.assert_array_equal(d['design'][designed], frames[designed])
    np.testing.assert_array_equal(d['n_design'][designed], nd[designed])
    np.testing.assert_array_equal(d['design_info'][designed].view(np.int32), ref.design_info.cpu().numpy()[designed].view(np.int32))
    rest = np.setdiff1d(np.arange(N), designed)
    assert (d['design'][rest] == -1).all() and (d['n_design'][rest] == 0).all() and (d['design_stop'][rest] == -1).all()
    assert d['design'].shape == (N, M) and (d['n_design'][designed] >= 1).all() and (d['n_design'] > 1).any()
    np.testing.assert_array_equal(d['design'][designed, 0], d1['query_point'][designed])
    if flip is not None:
        np.testing.assert_array_equal(d['flipped'], np.array([flips[i, :len(lists[i])].any() for i in range(N)]))
    ref.set_active_points(lists)
    ref.score(coff[6])
    want_idx = ref.renew(sel, d1['old_idx'], coff)
    np.testing.assert_array_equal(d['new_idx'][sel], want_idx[sel])


def test_one_question_at_once_is_the_call_without_the_argument(dev):
    from hual_amd import al
    RS = _round_set()
    prop, coff = RS['prop'], al.get_coff('charades', 1)
    for kw in (dict(), dict(observe_by='info_gain'), dict(observe_by='info_gain', answer_noise=0.1), dict(observe_by='info_gain', questions_per_clip=2)):
        def run(**more):
            return _prof(lambda: al.update_labels(copy.deepcopy(RS['data_old']), RS['data_gt'], prop, coff, return_debug=True,
                                                  annotator_flip=(0.3, np.random.default_rng(5)), **kw, **more))
        (a, da), ka = run()
        (b, db), kb = run(questions_at_once=1)
        assert a == b and ka == kb and not any('al_design' in k for k in kb)
        assert sorted(da) == sorted(db)
        for k in da:
            if k != 'updater':
                np.testing.assert_array_equal(da[k], db[k], err_msg=k)


def test_refusals_leave_data_old_untouched(dev):
    from hual_amd import al
    RS = _round_set()
    old = copy.deepcopy(RS['data_old'])
    for kw in (dict(questions_at_once=3), dict(questions_at_once=17, observe_by='info_gain'),
               dict(questions_at_once=3, observe_by='info_gain', questions_per_clip=2), dict(questions_at_once=3, acquire_by='label_gain')):
        with pytest.raises(ValueError):
            al.update_labels(old, RS['data_gt'], RS['prop'], al.get_coff('charades', 1), **kw)
        assert old == RS['data_old']


def test_run_round_with_two_questions_at_once(dev):
    from hual_amd import al
    RS = _round_set()
    model, ds, N = RS['model'], RS['ds'], RS['N']
    new, prop, m = al.run_round(model, ds, copy.deepcopy(RS['data_old']), RS['data_gt'], RS['prop'], 'charades', 1, epochs=1, batch_size=16,
                                lr=1e-3, drop_rate=0.2, observe_by='info_gain', questions_at_once=2)
    t = m['designs']
    assert sorted(t) == ['design', 'design_info', 'design_stop', 'n_design'] and 'sessions' not in m
    assert t['design'].shape == (N, 2) and t['design_info'].shape == (N, 2)
    ans = _answers(new, RS['data_old'])
    designed = t['design_stop'] >= 0
    assert [len(a) for a in ans if a] and (np.array([len(a) for a in ans])[designed] == t['n_design'][designed]).all()
    assert sum(1 for a in ans if a) == (N + 1) // 2 and t['n_design'].max() == 2 and len(prop) == N
    with pytest.raises(ValueError):
        al.run_round(model, ds, copy.deepcopy(RS['data_old']), RS['data_gt'], RS['prop'], 'charades', 1, epochs=1, batch_size=16, lr=1e-3,
                     drop_rate=0.2, questions_at_once=2)
