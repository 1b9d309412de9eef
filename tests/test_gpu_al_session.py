"""GPU: hual_al_session (annotation sessions: several adaptive questions per clip in one launch) against the launches it replaces -
a host loop over hual_al_query, behind hual_al_noisy_tilt under noise, bit for bit -, against the float64 reference of its contract
(tests/al_session_ref.py) teacher-forced on the device's own lists, its edge rows and the memory it must not touch, graph capture,
and the three places it lands: LabelUpdater.session, al.update_labels(questions_per_clip=) and al.run_round(questions_per_clip=).

The bars of the float64 comparison are those of tests/test_gpu_al_query.py, whose arithmetic every step of a session is: the asked
frame's reference gain within 1e-4 bits of the reference's maximum, the entropy and the gain within 5e-5 bits, q within 1e-6.  The
stop decision is compared wherever the reference's entropy and best gain lie more than al_session_ref.NEAR from their thresholds
(tests/test_al_session.py bounds the share of the other steps)."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import al_query_ref as Q
import al_session_ref as S
from test_gpu_al_query import _answers, _pads_intact, _prof, _round_set, _sentinel, make_set, pad_logits

pytestmark = pytest.mark.gpu

INCL_BAR, GAIN_BAR, ENT_BAR = 1e-6, 5e-5, 5e-5
FILL = {'asked': -7, 'answer': 77, 'q_asked': 777.0, 'gain': 777.0, 'entropy': 777.0, 'n_asked': -7, 'stop_reason': -7}      # no transcript holds these
NAMES = ('asked', 'answer', 'q_asked', 'gain', 'entropy', 'n_asked', 'stop_reason')


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def _i32(dev, x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).to(dev)


def _u32(dev, x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.uint32).view(np.int32))).to(dev)


def _specs(N, qmax):
    i32, f32 = torch.int32, torch.float32
    return [((N, qmax), i32), ((N, qmax), torch.int8), ((N, qmax), f32), ((N, qmax), f32), ((N, qmax + 1), f32), ((N,), i32), ((N,), i32)]


def run_session(dev, s, e, vlen, tlen, aps, gt, qmax, sel=None, budget=None, stop_entropy=-1.0, min_gain=0.0, eps=0.0, flip=None,
                selected=None):
    """one launch into sentinel-filled outputs -> dict of numpy arrays, after checking the memory around them, that the rows outside
    `selected` (default: all) keep their fill and that every slot of a selected row was written"""
    from hual_amd import lib
    N, ld = s.shape
    aset, keep = make_set(dev, vlen, tlen, aps, ld)
    bufs = [_sentinel(shape, dt, dev, FILL[k]) for k, (shape, dt) in zip(NAMES, _specs(N, qmax))]
    out = tuple(b[0] for b in bufs)
    got = lib.al_session(aset, s, e, np.asarray(tlen), _i32(dev, gt), qmax, sel=_i32(dev, sel), budget=_i32(dev, budget),
                         stop_entropy=stop_entropy, min_gain=min_gain, eps=eps, flip=_u32(dev, flip), out=out)
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
    return r


def host_loop(dev, s, e, vlen, tlen, aps, gt, qmax, budget=None, stop_entropy=-1.0, min_gain=0.0, eps=0.0, flip=None):
    """the launches a session replaces: per question one hual_al_query on the lists so far (under noise: hual_al_noisy_tilt, then
    hual_al_query on the tilted rows and a set without answers), a read-back and a host append -> the transcript as run_session's"""
    from hual_amd import lib
    N, ld = s.shape
    lists = [list(a) for a in aps]
    cap = np.full(N, qmax) if budget is None else np.clip(np.asarray(budget), 0, qmax)
    flip = np.zeros(N, dtype=np.uint32) if flip is None else np.asarray(flip, dtype=np.uint32)
    r = dict(asked=np.full((N, qmax), -1, np.int32), answer=np.full((N, qmax), -1, np.int8), q_asked=np.full((N, qmax), -1, np.float32),
             gain=np.full((N, qmax), -1, np.float32), entropy=np.full((N, qmax + 1), -1, np.float32), n_asked=np.zeros(N, np.int32),
             stop_reason=np.full(N, -1, np.int32))
    over = np.array([len(lists[n]) + cap[n] > S.MAX_POINTS for n in range(N)])
    r['stop_reason'][over] = S.OVERFLOW
    free, keep_free = make_set(dev, vlen, tlen, [[] for _ in range(N)], ld)
    for k in range(qmax + 1):
        live = np.flatnonzero(r['stop_reason'] < 0)
        if not len(live):
            break
        aset, keep = make_set(dev, vlen, tlen, lists, ld)
        if eps > 0:
            s_t, e_t, _ = lib.al_noisy_tilt(aset, s, e, np.asarray(tlen), eps)
            out = lib.al_query(free, s_t, e_t, np.asarray(tlen))
        else:
            out = lib.al_query(aset, s, e, np.asarray(tlen))
        incl, _, qp, qg, ent, agree = [o.cpu().numpy() for o in out]
        for n in live:
            r['entropy'][n, k] = ent[n]
            if qp[n] < 0:
                why = S.CONTRADICTORY if agree[n] == 0 else S.POISONED
            elif stop_entropy >= 0 and ent[n] <= np.float32(stop_entropy):
                why = S.ENTROPY
            elif not qg[n] > np.float32(min_gain):
                why = S.GAIN
            elif k >= cap[n]:
                why = S.BUDGET
            else:
                t = int(qp[n])
                ans = bool(gt[n][0] <= t <= gt[n][1]) != bool((int(flip[n]) >> k) & 1)
                r['asked'][n, k], r['answer'][n, k], r['q_asked'][n, k], r['gain'][n, k] = t, ans, incl[n, t], qg[n]
                r['n_asked'][n] = k + 1
                lists[n].append((t, ans))
                continue
            r['stop_reason'][n] = why
    assert (r['stop_reason'] >= 0).all()
    return r, lists


def assert_same_transcript(got, want, rows=None):
    for k in NAMES:
        a, b = got[k], want[k]
        if rows is not None:
            a, b = a[rows], b[rows]
        if a.dtype == np.float32:
            a, b = a.view(np.int32), b.view(np.int32)                 # bit for bit
        np.testing.assert_array_equal(a, b, err_msg=k)


_LOGITS = {}


def case_logits(dev, T, extra):
    if (T, extra) not in _LOGITS:
        c = Q.case(T)
        _LOGITS[(T, extra)] = (pad_logits(dev, c['s'], T + extra, 1), pad_logits(dev, c['e'], T + extra, 2))
    return _LOGITS[(T, extra)]


# ---------------------------------------------------------------------------------------------------------------- 1. the launches it replaces
@pytest.mark.parametrize('extra', [0, 7])
@pytest.mark.parametrize('T', Q.TS)
def test_equals_the_launches_it_replaces(dev, T, extra):
    c = Q.case(T)
    s, e = case_logits(dev, T, extra)
    vlen, tlen, gt = c['vlen'].numpy(), [T] * Q.N_ROWS, c['gt']
    reasons, asked = set(), 0
    for qmax in (1, 6, 16):
        for start in S.STARTS:
            for eps in S.EPS:
                for flipped in (False, True):
                    for stop_entropy, min_gain in ((-1.0, 0.0), (S.STOP_ENTROPY, S.MIN_GAIN)) if qmax == 6 else ((-1.0, 0.0),):
                        kw = dict(stop_entropy=stop_entropy, min_gain=min_gain, eps=eps, flip=S.flip_masks(T) if flipped else None)
                        lists = S.start_list(T, start)
                        got = run_session(dev, s, e, vlen, tlen, lists, gt, qmax, **kw)
                        want, _ = host_loop(dev, s, e, vlen, tlen, lists, gt, qmax, **kw)
                        assert_same_transcript(got, want)
                        reasons |= set(int(x) for x in got['stop_reason'])
                        asked += int(got['n_asked'].sum())
    assert asked > 0 and S.GAIN in reasons and (T == 2 or {S.BUDGET, S.ENTROPY} <= reasons)
    assert T == 2 or S.CONTRADICTORY in reasons                       # (a flipped answer of an earlier round)


# ---------------------------------------------------------------------------------------------------------------- 2. the float64 reference
@pytest.mark.parametrize('extra', [0, 7])
@pytest.mark.parametrize('T', Q.TS)
def test_against_the_float64_reference_teacher_forced(dev, T, extra):
    c = Q.case(T)
    s, e = case_logits(dev, T, extra)
    vlen, tlen, gt, qmax = c['vlen'].numpy(), [T] * Q.N_ROWS, c['gt'], 6
    d = dict(q=0.0, gain=0.0, ent=0.0, lost=0.0)
    compared = skipped = 0
    for start, eps, flipped in S.TEACHER_GRID:
        fm = S.flip_masks(T) if flipped else np.zeros(Q.N_ROWS, dtype=np.uint32)
        lists = S.start_list(T, start)
        got = run_session(dev, s, e, vlen, tlen, lists, gt, qmax, stop_entropy=S.STOP_ENTROPY, min_gain=S.MIN_GAIN, eps=eps, flip=fm)
        for n in range(Q.N_ROWS):
            na = int(got['n_asked'][n])
            cur = list(lists[n])
            for k in range(na + 1):
                post = S.case_step(T, n, tuple(cur), eps)             # the reference on the device's own list up to this step
                if post['status'] == Q.LIVE:
                    d['ent'] = max(d['ent'], abs(float(got['entropy'][n, k]) - post['post_entropy']))
                else:
                    assert got['entropy'][n, k] == -1.0
                dev_why = int(got['stop_reason'][n]) if k == na else None
                if S.near_threshold(post, S.STOP_ENTROPY, S.MIN_GAIN):
                    skipped += 1
                else:
                    assert S.decide(post, k, qmax, S.STOP_ENTROPY, S.MIN_GAIN) == dev_why, (start, eps, flipped, n, k)
                    compared += 1
                if k == na:
                    break
                assert post['status'] == Q.LIVE
                t, ans = int(got['asked'][n, k]), bool(got['answer'][n, k])
                assert 0 <= t < int(c['v'][n])
                d['lost'] = max(d['lost'], float(post['gain'].max() - post['gain'][t]))
                d['q'] = max(d['q'], abs(float(got['q_asked'][n, k]) - float(post['incl'][t])))
                d['gain'] = max(d['gain'], abs(float(got['gain'][n, k]) - float(post['gain'][t])))
                assert ans == (Q.answer(gt[n], t) != bool((int(fm[n]) >> k) & 1))      # the answer is exact
                cur.append((t, ans))
            assert (got['asked'][n, na:] == -1).all() and (got['answer'][n, na:] == -1).all() and (got['entropy'][n, na + 1:] == -1).all()
            assert (got['q_asked'][n, na:] == -1).all() and (got['gain'][n, na:] == -1).all()
    print('T=%d ld=%d: max |q_asked - ref| = %.3e (bar %.0e), |gain - ref| = %.3e bits (bar %.0e), |entropy - ref| = %.3e bits (bar %.0e), '
          'reference gain lost at the asked frame = %.3e bits (bar %.0e); %d decisions compared, %d near a threshold skipped'
          % (T, T + extra, d['q'], INCL_BAR, d['gain'], GAIN_BAR, d['ent'], ENT_BAR, d['lost'], 2 * GAIN_BAR, compared, skipped))
    assert d['q'] <= INCL_BAR
    assert d['gain'] <= GAIN_BAR
    assert d['ent'] <= ENT_BAR
    assert d['lost'] <= 2 * GAIN_BAR
    assert skipped <= 0.05 * (compared + skipped)


# ---------------------------------------------------------------------------------------------------------------- 3. edges
def _edge_set(dev):
    """six rows of case(33), ld = 40: 0 plain | 1 a NaN logit | 2 v = 1 | 3 a list of 60 points | 4 budget 0 | 5 budget above qmax"""
    c = Q.case(33)
    pick = [0, 1, 8, 2, 3, 4]
    s, e = c['s'][pick].clone(), c['e'][pick].clone()
    s[1, 2] = float('nan')
    vlen = c['vlen'].numpy()[pick]
    assert vlen[2] == 1
    aps = [[], [], [], [(0, False)] * 60, [], []]
    budget = np.array([6, 6, 6, 6, 0, 99], dtype=np.int32)
    return pad_logits(dev, s, 40, 3), pad_logits(dev, e, 40, 4), vlen, [33] * 6, aps, c['gt'][pick], budget


def test_edge_rows(dev):
    s, e, vlen, tlen, aps, gt, budget = _edge_set(dev)
    got = run_session(dev, s, e, vlen, tlen, aps, gt, 6, budget=budget)
    want, _ = host_loop(dev, s, e, vlen, tlen, aps, gt, 6, budget=budget)
    assert_same_transcript(got, want)
    np.testing.assert_array_equal(got['stop_reason'][1:5], [S.POISONED, S.GAIN, S.OVERFLOW, S.BUDGET])
    np.testing.assert_array_equal(got['n_asked'][1:5], [0, 0, 0, 0])
    assert got['entropy'][1, 0] == -1.0 and abs(got['entropy'][2, 0]) <= ENT_BAR and got['entropy'][3, 0] == -1.0 and got['entropy'][4, 0] > 0
    assert got['n_asked'][0] > 1
    plain = run_session(dev, s, e, vlen, tlen, aps, gt, 6)
    assert_same_transcript(plain, got, rows=[0, 1, 2, 5])             # (a budget of 99 reads as qmax)
    # the same list with a budget that fits is not an overflow
    fits = run_session(dev, s, e, vlen, tlen, aps, gt, 6, budget=np.array([6, 6, 6, 4, 0, 99], dtype=np.int32))
    assert fits['stop_reason'][3] != S.OVERFLOW
    # under noise: the same flags
    noisy = run_session(dev, s, e, vlen, tlen, aps, gt, 6, budget=budget, eps=0.2)
    want_n, _ = host_loop(dev, s, e, vlen, tlen, aps, gt, 6, budget=budget, eps=0.2)
    assert_same_transcript(noisy, want_n)
    np.testing.assert_array_equal(noisy['stop_reason'][1:5], [S.POISONED, S.GAIN, S.OVERFLOW, S.BUDGET])


def test_eps_one_half_copies_the_logits(dev):
    """eps = 0.5: lam == 0, the tilt copies the logits, an answer carries nothing - the posterior never moves, so every question of a
    session is the same frame and only the budget ends it"""
    T = 33
    c = Q.case(T)
    s, e = case_logits(dev, T, 7)
    vlen, tlen, lists, fm = c['vlen'].numpy(), [T] * Q.N_ROWS, S.start_list(T, 3), S.flip_masks(T)
    got = run_session(dev, s, e, vlen, tlen, lists, c['gt'], 6, eps=0.5, flip=fm)
    want, _ = host_loop(dev, s, e, vlen, tlen, lists, c['gt'], 6, eps=0.5, flip=fm)
    assert_same_transcript(got, want)
    free = run_session(dev, s, e, vlen, tlen, [[] for _ in range(Q.N_ROWS)], c['gt'], 6, flip=fm)      # the hard rule with no answer yet
    asking = got['n_asked'] > 0
    assert asking.sum() >= Q.N_ROWS - 2
    for n in np.flatnonzero(asking):
        assert got['n_asked'][n] == 6 and got['stop_reason'][n] == S.BUDGET
        assert (got['asked'][n] == free['asked'][n, 0]).all()
        assert (got['entropy'][n].view(np.int32) == free['entropy'][n, 0].view(np.int32)).all()
        assert (got['gain'][n].view(np.int32) == free['gain'][n, 0].view(np.int32)).all()


def test_sel_with_a_repeated_and_an_outside_id(dev):
    s, e, vlen, tlen, aps, gt, budget = _edge_set(dev)
    for eps in (0.0, 0.2):
        full = run_session(dev, s, e, vlen, tlen, aps, gt, 6, budget=budget, eps=eps)
        part = run_session(dev, s, e, vlen, tlen, aps, gt, 6, budget=budget, eps=eps, sel=[5, 0, 77, 0, -3, 2], selected=[0, 2, 5])
        assert_same_transcript(part, full, rows=[0, 2, 5])


def test_a_row_longer_than_256_frames_is_poisoned(dev):
    """tlen is device memory, so the C entry point cannot refuse it (lib.al_session does, on the host): the raw call"""
    from hual_amd import lib
    c = Q.case(33)
    N, ld, qmax = 2, 300, 4
    s = pad_logits(dev, c['s'][:2], ld, 5)
    e = pad_logits(dev, c['e'][:2], ld, 6)
    aset, keep = make_set(dev, [300, 33], [300, 33], [[], []], ld)
    with pytest.raises(lib.HualError):
        lib.al_session(aset, s, e, np.array([300, 33]), _i32(dev, c['gt'][:2]), qmax)
    bufs = [_sentinel(shape, dt, dev, FILL[k]) for k, (shape, dt) in zip(NAMES, _specs(N, qmax))]
    gt = _i32(dev, c['gt'][:2])
    lib.check(lib.load().hual_al_session(ctypes.byref(aset), lib.ptr(s), lib.ptr(e), lib.ptr(gt), None, N, qmax, None, -1.0, 0.0, 0.0, None,
                                         *[lib.ptr(b[0]) for b in bufs], lib.stream_ptr()))
    torch.cuda.synchronize()
    r = {k: b[0].cpu().numpy() for k, b in zip(NAMES, bufs)}
    assert all(_pads_intact(b[1], b[2], FILL[k]) for k, b in zip(NAMES, bufs))
    assert r['stop_reason'][0] == S.POISONED and r['n_asked'][0] == 0 and (r['asked'][0] == -1).all() and (r['entropy'][0] == -1).all()
    assert r['stop_reason'][1] == S.BUDGET and r['n_asked'][1] == qmax


def test_argument_errors(dev):
    from hual_amd import lib
    s, e, vlen, tlen, aps, gt, budget = _edge_set(dev)
    aset, keep = make_set(dev, vlen, tlen, aps, 40)
    g = _i32(dev, gt)
    for kw in (dict(qmax=0), dict(qmax=17), dict(min_gain=-0.1), dict(min_gain=float('nan')), dict(eps=0.6), dict(eps=-0.1),
               dict(eps=float('nan')), dict(gt=None), dict(sel=torch.zeros(0, dtype=torch.int32, device=dev))):
        args = dict(qmax=6, gt=g)
        args.update(kw)
        with pytest.raises(lib.HualError):
            lib.al_session(aset, s, e, np.asarray(tlen), args.pop('gt'), args.pop('qmax'), **args)
    # the C entry point itself: negative codes and hual_last_error, before any HIP call
    outs = [torch.zeros(shape, dtype=dt, device=dev) for shape, dt in _specs(6, 6)]
    L = lib.load()

    def raw(qmax=6, min_gain=0.0, eps=0.0, gt=g, drop=None):
        o = [None if i == drop else lib.ptr(x) for i, x in enumerate(outs)]
        return L.hual_al_session(ctypes.byref(aset), lib.ptr(s), lib.ptr(e), lib.ptr(gt), None, 6, qmax, None, -1.0, min_gain, eps, None,
                                 *o, lib.stream_ptr())
    assert raw() == 0
    for bad in (dict(qmax=0), dict(qmax=17), dict(min_gain=-1.0), dict(eps=0.51), dict(gt=None), dict(drop=0), dict(drop=6)):
        assert raw(**bad) < 0, bad
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- 4. graph capture
def test_graph_capture_and_replay(dev):
    from hual_amd import lib
    T = 70
    c = Q.case(T)
    s, e = case_logits(dev, T, 7)
    vlen, tlen, lists = c['vlen'].numpy(), [T] * Q.N_ROWS, S.start_list(T, 3)
    fm = S.flip_masks(T)
    for eps in (0.0, 0.2):
        want = run_session(dev, s, e, vlen, tlen, lists, c['gt'], 6, eps=eps, flip=fm)
        aset, keep = make_set(dev, vlen, tlen, lists, T + 7)
        gt, flip = _i32(dev, c['gt']), _u32(dev, fm)
        out = tuple(torch.zeros(shape, dtype=dt, device=dev) for shape, dt in _specs(Q.N_ROWS, 6))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            lib.al_session(aset, s, e, np.asarray(tlen), gt, 6, eps=eps, flip=flip, out=out)      # (warm-up: the module is loaded)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            lib.al_session(aset, s, e, np.asarray(tlen), gt, 6, eps=eps, flip=flip, out=out)
        for _ in range(2):
            for o in out:
                o.fill_(5)
            graph.replay()
            torch.cuda.synchronize()
            assert_same_transcript({k: o.cpu().numpy() for k, o in zip(NAMES, out)}, want)


# ---------------------------------------------------------------------------------------------------------------- 5. the updater, the label update
def _updater(S_):
    from hual_amd import al
    aps = [[] for _ in range(S_['N'])]
    return al.LabelUpdater(S_['prop'], aps)


def _gt_idx(S_, up):
    from hual_amd import al
    return np.array([[al._round_half_even_index(t, S_['data_gt'][i][1], int(up.vlen_h[i])) for t in S_['data_gt'][i][2]]
                     for i in range(S_['N'])])


@pytest.mark.parametrize('noise', [None, 0.1])
def test_label_updater_session(dev, noise):
    RS = _round_set()
    N = RS['N']
    up, ref = _updater(RS), _updater(RS)
    gt = _gt_idx(RS, up)
    flips = np.random.default_rng(11).integers(0, 8, N).astype(np.uint32)
    sel = np.arange(0, N, 2)
    (asked, answers, n_asked), launches = _prof(lambda: up.session(gt, 3, noise=noise, flips=flips, sel=sel))
    assert sum(launches.values()) == 1 and 'al_session' in list(launches)[0], launches
    assert up.tilt_eps is None                                        # the new lists invalidate a tilt
    # the equivalent single questions
    lists = [[] for _ in range(N)]
    going = np.zeros(N, dtype=bool)
    going[sel] = True
    for k in range(3):
        ref.query(noise=noise)
        qp, qg = ref.query_point.cpu().numpy(), ref.query_gain.cpu().numpy()
        going &= qg > 0
        for i in np.flatnonzero(going):
            t = int(qp[i])
            lists[i].append((t, bool(gt[i, 0] <= t <= gt[i, 1]) != bool((int(flips[i]) >> k) & 1)))
        ref.set_active_points(lists)
    assert up.aps == lists and sum(len(a) for a in lists) > len(sel)
    for i in range(N):
        assert [(int(asked[i, k]), bool(answers[i, k])) for k in range(int(n_asked[i]))] == lists[i]
    assert (up.asked.cpu().numpy()[1::2] == -1).all() and (up.stop_reason.cpu().numpy()[1::2] == -1).all()
    # what reads the lists reads the same
    old = np.zeros((N, 2), dtype=np.int32)
    for a, b in ((up, ref),):
        a.query(noise=noise)
        b.query(noise=noise)
        for k in ('incl', 'gain', 'query_point', 'query_gain', 'post_entropy'):
            assert torch.equal(getattr(a, k), getattr(b, k)), k
        for x, y in zip(a.mbr_label(np.arange(N), old, noise=noise), b.mbr_label(np.arange(N), old, noise=noise)):
            np.testing.assert_array_equal(x, y)
        a.span_marginals(noise=noise)
        b.span_marginals(noise=noise)
        assert torch.equal(a.y_start, b.y_start) and torch.equal(a.y_end, b.y_end) and torch.equal(a.marg_status, b.marg_status)
    # the host knows the lists: a row the kernel would report as an overflow is refused before the launch
    up.set_active_points([[(0, False)] * 62] + [[] for _ in range(N - 1)])
    with pytest.raises(ValueError, match='exceeds'):
        up.session(gt, 3)
    up.session(gt, 3, sel=np.arange(1, N))                            # (the long row is not selected)


@pytest.mark.parametrize('noise,flip', [(None, None), (0.1, 0.3), (None, 0.3)])
def test_update_labels_with_three_questions(dev, noise, flip):
    from hual_amd import al
    RS = _round_set()
    N, prop, coff, Qn = RS['N'], RS['prop'], al.get_coff('charades', 1), 3
    kw = dict(observe_by='info_gain', answer_noise=noise)

    def flipper():
        return None if flip is None else (flip, np.random.default_rng(21))
    (new, d), launches = _prof(lambda: al.update_labels(copy.deepcopy(RS['data_old']), RS['data_gt'], prop, coff, return_debug=True,
                                                        annotator_flip=flipper(), questions_per_clip=Qn, **kw))
    assert sum(v for k, v in launches.items() if 'al_session' in k) == 1, launches
    # the restatement: the same selection, three iterated LabelUpdater.query calls on the selected samples, the same renew
    base, d1 = al.update_labels(copy.deepcopy(RS['data_old']), RS['data_gt'], prop, coff, return_debug=True, **kw)
    for key in ('order', 'uncert_video', 'observe', 'gt_idx', 'old_idx', 'query_point', 'observe_used'):
        np.testing.assert_array_equal(d[key], d1[key])
    sel, gt, observe = d1['order'][:(N + 1) // 2], d1['gt_idx'], d1['observe']
    flips = np.zeros((N, Qn), dtype=bool)
    if flip is not None:
        rng = np.random.default_rng(21)
        for i in sel:
            for k in range(Qn):
                flips[i, k] = rng.random() < flip
    ref = _updater(RS)
    lists = [[] for _ in range(N)]
    going = np.zeros(N, dtype=bool)
    going[sel] = True
    for k in range(Qn):
        ref.query(noise=noise)
        qp, qg = ref.query_point.cpu().numpy(), ref.query_gain.cpu().numpy()
        for i in sel:
            if not going[i]:
                continue
            if qg[i] > 0:
                t = int(qp[i])
            elif k == 0:
                t, going[i] = int(observe[i]), False                  # the reference's frame, one question
            else:
                going[i] = False
                continue
            lists[i].append((t, bool(gt[i, 0] <= t <= gt[i, 1]) != bool(flips[i, k])))
        ref.set_active_points(lists)
    ans = _answers(new, RS['data_old'])
    for i in range(N):
        pos, neg = [f for f, p in lists[i] if p], [f for f, p in lists[i] if not p]
        assert ans[i] == [(f, True) for f in pos] + [(f, False) for f in neg], i
        assert [(int(d['asked'][i, k]), bool(d['answers'][i, k])) for k in range(int(d['n_asked'][i]))] == lists[i]
        assert (d['asked'][i, int(d['n_asked'][i]):] == -1).all()
    assert d['updater'].aps == lists
    assert (d['n_asked'][sel] >= 1).all() and (d['n_asked'][sel] > 1).any() and d['n_asked'].sum() == sum(len(a) for a in lists)
    assert d['entropy_path'].shape == (N, Qn + 1) and d['stop_reason'].shape == (N,)
    if flip is not None:
        np.testing.assert_array_equal(d['flipped'], np.array([flips[i, :int(d['n_asked'][i])].any() for i in range(N)]))
    ref.score(coff[6])
    want_idx = ref.renew(sel, d1['old_idx'], coff)
    np.testing.assert_array_equal(d['new_idx'][sel], want_idx[sel])
    for i in range(N):
        if i in set(int(x) for x in sel):
            dur, vl = RS['data_old'][i][1], int(ref.vlen_h[i])
            assert new[i][2] == [round(int(t) / (vl - 1) * dur, 2) for t in want_idx[i]]
        else:
            assert new[i][2] == RS['data_old'][i][2]


def test_one_question_per_clip_is_the_call_without_the_argument(dev):
    from hual_amd import al
    RS = _round_set()
    prop, coff = RS['prop'], al.get_coff('charades', 1)
    for kw in (dict(), dict(observe_by='info_gain'), dict(observe_by='info_gain', answer_noise=0.1)):
        def run(**more):
            return _prof(lambda: al.update_labels(copy.deepcopy(RS['data_old']), RS['data_gt'], prop, coff, return_debug=True,
                                                  annotator_flip=(0.3, np.random.default_rng(5)), **kw, **more))
        (a, da), ka = run()
        (b, db), kb = run(questions_per_clip=1)
        assert a == b and ka == kb and not any('al_session' in k for k in kb)
        assert sorted(da) == sorted(db)
        for k in da:
            if k != 'updater':
                np.testing.assert_array_equal(da[k], db[k], err_msg=k)


# ---------------------------------------------------------------------------------------------------------------- 6. a whole round
def test_run_round_with_two_questions(dev):
    from hual_amd import al
    RS = _round_set()
    model, ds, N = RS['model'], RS['ds'], RS['N']
    new, prop, m = al.run_round(model, ds, copy.deepcopy(RS['data_old']), RS['data_gt'], RS['prop'], 'charades', 1, epochs=1, batch_size=16,
                                lr=1e-3, drop_rate=0.2, observe_by='info_gain', questions_per_clip=2)
    t = m['sessions']
    assert sorted(t) == ['answers', 'asked', 'entropy_path', 'n_asked', 'stop_reason']
    assert t['asked'].shape == (N, 2) and t['entropy_path'].shape == (N, 3)
    ans = _answers(new, RS['data_old'])
    assert [len(a) for a in ans] == list(t['n_asked'])
    assert (t['n_asked'] > 0).sum() == (N + 1) // 2 and t['n_asked'].max() == 2 and len(prop) == N
    with pytest.raises(ValueError):
        al.run_round(model, ds, copy.deepcopy(RS['data_old']), RS['data_gt'], RS['prop'], 'charades', 1, epochs=1, batch_size=16, lr=1e-3,
                     drop_rate=0.2, questions_per_clip=2)
