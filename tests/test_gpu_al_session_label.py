"""GPU: hual_al_session_label (annotation sessions that stop once the pseudo-label is reliable) against the launches it replaces - a
host loop over hual_al_query, hual_al_mbr_label and hual_al_hit_label per pass, behind hual_al_noisy_tilt under noise, every stored
value bit for bit -, against the float64 reference of its contract (tests/al_session_label_ref.py) teacher-forced on the device's own
lists, its edge rows and the memory it must not touch, graph capture, and the two places it lands: LabelUpdater.session_label and
al.update_labels(stop_hit=).

The bars of the float64 comparison: label_conf and label_hit within 1e-6, the project's bar for float64-accumulated probabilities
stored as float32 (tests/test_gpu_al_label.py, tests/test_gpu_al_hit_label.py); the label equals the reference's wherever the
reference's runner-up lies 1e-5 or more below it, and elsewhere its reference R is within 2e-6 of the best; a stop decision is compared
wherever the reference's hit probability, entropy and gain lie outside al_session_label_ref.near_threshold (tests/
test_al_session_label.py bounds the share of the other passes on the reference alone), and at most 5 % of the passes may be skipped."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import al_label_ref as L
import al_hit_ref as HL
import al_query_ref as Q
import al_session_label_ref as SL
import al_session_ref as S
from test_gpu_al_query import _pads_intact, _prof, _round_set, _sentinel, make_set, pad_logits
from test_gpu_al_session import FILL as SESSION_FILL, NAMES as SESSION_NAMES, _i32, _specs as _session_specs, _u32, case_logits
from test_gpu_al_session import run_session

pytestmark = pytest.mark.gpu

PROB_BAR, TIE_BAR = 1e-6, 2e-6
NAMES = SESSION_NAMES + ('label', 'label_conf', 'label_hit')
FILL = dict(SESSION_FILL, label=-7, label_conf=777.0, label_hit=777.0)      # no trail holds these
THR = SL.THR
RULE = (0.9, 2)                                                             # stop_hit 0.9 at 7/10


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def _specs(N, qmax, M=len(THR)):
    return _session_specs(N, qmax) + [((N, qmax + 1, 2), torch.int32), ((N, qmax + 1), torch.float32), ((N, qmax + 1, M), torch.float32)]


def run_label_session(dev, s, e, vlen, tlen, aps, gt, qmax, thr=THR, stop_hit=-1.0, stop_m=0, sel=None, budget=None, stop_entropy=-1.0,
                      min_gain=0.0, eps=0.0, flip=None, selected=None):
    """one launch into sentinel-filled outputs -> dict of numpy arrays, after checking the memory around them, that the rows outside
    `selected` (default: all) keep their fill and that every slot of a selected row was written"""
    from hual_amd import lib
    N, ld = s.shape
    aset, keep = make_set(dev, vlen, tlen, aps, ld)
    bufs = [_sentinel(shape, dt, dev, FILL[k]) for k, (shape, dt) in zip(NAMES, _specs(N, qmax, len(thr)))]
    out = tuple(b[0] for b in bufs)
    got = lib.al_session_label(aset, s, e, np.asarray(tlen), _i32(dev, gt), qmax, thresholds=thr, stop_m=stop_m, stop_hit=stop_hit,
                               sel=_i32(dev, sel), budget=_i32(dev, budget), stop_entropy=stop_entropy, min_gain=min_gain, eps=eps,
                               flip=_u32(dev, flip), out=out)
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


def host_loop(dev, s, e, vlen, tlen, aps, gt, qmax, thr=THR, stop_hit=-1.0, stop_m=0, budget=None, stop_entropy=-1.0, min_gain=0.0, eps=0.0,
              flip=None):
    """the launches a session with a label trail replaces: per pass hual_al_query, hual_al_mbr_label and hual_al_hit_label (the label
    as the one candidate, no search) on the lists so far - under noise behind hual_al_noisy_tilt, on the tilted rows and a set without
    answers -, a read-back, the decision from the stored float32 values and a host append -> the outputs as run_label_session's"""
    from hual_amd import lib
    N, ld = s.shape
    M = len(thr)
    lists = [list(a) for a in aps]
    cap = np.full(N, qmax) if budget is None else np.clip(np.asarray(budget), 0, qmax)
    flip = np.zeros(N, dtype=np.uint32) if flip is None else np.asarray(flip, dtype=np.uint32)
    r = dict(asked=np.full((N, qmax), -1, np.int32), answer=np.full((N, qmax), -1, np.int8), q_asked=np.full((N, qmax), -1, np.float32),
             gain=np.full((N, qmax), -1, np.float32), entropy=np.full((N, qmax + 1), -1, np.float32), n_asked=np.zeros(N, np.int32),
             stop_reason=np.full(N, -1, np.int32), label=np.full((N, qmax + 1, 2), -1, np.int32),
             label_conf=np.full((N, qmax + 1), -1, np.float32), label_hit=np.full((N, qmax + 1, M), -1, np.float32))
    over = np.array([len(lists[n]) + cap[n] > S.MAX_POINTS for n in range(N)])
    r['stop_reason'][over] = S.OVERFLOW
    free, keep_free = make_set(dev, vlen, tlen, [[] for _ in range(N)], ld)
    tl = np.asarray(tlen)
    for k in range(qmax + 1):
        live = np.flatnonzero(r['stop_reason'] < 0)
        if not len(live):
            break
        aset, keep = make_set(dev, vlen, tlen, lists, ld)
        rs, rows_s, rows_e = aset, s, e
        if eps > 0:
            rows_s, rows_e, _ = lib.al_noisy_tilt(aset, s, e, tl, eps)
            rs = free
        incl, _, qp, qg, ent, agree = [o.cpu().numpy() for o in lib.al_query(rs, rows_s, rows_e, tl)]
        new_idx, conf, _ = lib.al_mbr_label(rs, rows_s, rows_e, tl)
        hit, _ = lib.al_hit_label(rs, rows_s, rows_e, tl, thresholds=thr, cand=new_idx[:, None, :].contiguous(), best=False)
        new_idx, conf, hit = new_idx.cpu().numpy(), conf.cpu().numpy(), hit.cpu().numpy()[:, 0, :]
        for n in live:
            r['entropy'][n, k] = ent[n]
            if qp[n] < 0:
                why = S.CONTRADICTORY if agree[n] == 0 else S.POISONED
            else:
                r['label'][n, k], r['label_conf'][n, k], r['label_hit'][n, k] = new_idx[n], conf[n], hit[n]
                if stop_hit >= 0 and hit[n, stop_m] >= np.float32(stop_hit):
                    why = SL.RELIABLE
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


def assert_same(got, want, rows=None, names=NAMES):
    for k in names:
        a, b = got[k], want[k]
        if rows is not None:
            a, b = a[rows], b[rows]
        if a.dtype == np.float32:
            a, b = a.view(np.int32), b.view(np.int32)                 # bit for bit
        np.testing.assert_array_equal(a, b, err_msg=k)


# ---------------------------------------------------------------------------------------------------------------- 1. the launches it replaces
@pytest.mark.parametrize('extra', [0, 7])
@pytest.mark.parametrize('T', Q.TS)
def test_equals_the_launches_it_replaces(dev, T, extra):
    c = Q.case(T)
    s, e = case_logits(dev, T, extra)
    vlen, tlen, gt = c['vlen'].numpy(), [T] * Q.N_ROWS, c['gt']
    reasons, asked = set(), 0
    for qmax in (1, 6, 16) if T == 33 else (1, 6):
        for start in S.STARTS:
            lists = S.start_list(T, start)
            for eps in (0.0, 0.05):
                for flipped in (False, True):
                    kw = dict(eps=eps, flip=S.flip_masks(T) if flipped else None)
                    for stop_hit, stop_m in ((-1.0, 0), RULE):
                        got = run_label_session(dev, s, e, vlen, tlen, lists, gt, qmax, stop_hit=stop_hit, stop_m=stop_m, **kw)
                        want, _ = host_loop(dev, s, e, vlen, tlen, lists, gt, qmax, stop_hit=stop_hit, stop_m=stop_m, **kw)
                        assert_same(got, want)
                        if stop_hit < 0:                                  # the rule off: hual_al_session's seven outputs
                            assert_same(got, run_session(dev, s, e, vlen, tlen, lists, gt, qmax, **kw), names=SESSION_NAMES)
                            assert SL.RELIABLE not in got['stop_reason']
                        else:
                            reasons |= set(int(x) for x in got['stop_reason'])
                        asked += int(got['n_asked'].sum())
                        na = got['n_asked']
                        for n in range(Q.N_ROWS):                         # the trail ends where the session does
                            assert (got['label'][n, na[n] + 1:] == -1).all() and (got['label_hit'][n, na[n] + 1:] == -1).all()
    assert asked > 0 and SL.RELIABLE in reasons
    assert T < 33 or S.BUDGET in reasons


# ---------------------------------------------------------------------------------------------------------------- 2. the float64 reference
@pytest.mark.parametrize('T', [2, 33, 70])
def test_against_the_float64_reference_teacher_forced(dev, T):
    c = Q.case(T)
    s, e = case_logits(dev, T, 7)
    vlen, tlen, gt, qmax = c['vlen'].numpy(), [T] * Q.N_ROWS, c['gt'], 6
    stop_hit, stop_m = RULE
    d = dict(conf=0.0, hit=0.0, tie=0.0)
    compared = skipped = close_labels = 0
    for start, eps, flipped in SL.SETTINGS:
        fm = S.flip_masks(T) if flipped else np.zeros(Q.N_ROWS, dtype=np.uint32)
        lists = S.start_list(T, start)
        got = run_label_session(dev, s, e, vlen, tlen, lists, gt, qmax, stop_hit=stop_hit, stop_m=stop_m, eps=eps, flip=fm)
        for n in range(Q.N_ROWS):
            na = int(got['n_asked'][n])
            cur = list(lists[n])
            for k in range(na + 1):
                p = SL.case_pass(T, n, tuple(cur), eps)               # the reference on the device's own list up to this pass
                if p['post']['status'] != Q.LIVE:
                    assert (got['label'][n, k] == -1).all() and got['label_conf'][n, k] == -1.0 and (got['label_hit'][n, k] == -1.0).all()
                else:
                    lab, ref = tuple(int(x) for x in got['label'][n, k]), p['label']
                    if ref['margin'] >= SL.MARGIN:
                        assert lab == ref['label'], (start, eps, flipped, n, k, lab, ref['label'])
                        hit_ref = p['hit']
                    else:                                             # a near tie: the device's span is as good as the reference's
                        close_labels += 1
                        assert L.is_member(ref['st'], *lab)
                        d['tie'] = max(d['tie'], ref['conf'] - L.span_R(ref['st'], *lab))
                        hit_ref = HL.cand_prob(p['hit_state'], [lab], list(THR))[0]
                    if lab == ref['label']:
                        d['conf'] = max(d['conf'], abs(float(got['label_conf'][n, k]) - ref['conf']))
                    d['hit'] = max(d['hit'], float(np.abs(got['label_hit'][n, k].astype(np.float64) - hit_ref).max()))
                dev_why = int(got['stop_reason'][n]) if k == na else None
                if SL.near_threshold(p, stop_hit, stop_m) or (p['label'] is not None and p['label']['margin'] < SL.MARGIN):
                    skipped += 1
                else:
                    assert SL.decide(p, k, qmax, stop_hit, stop_m) == dev_why, (start, eps, flipped, n, k)
                    compared += 1
                if k == na:
                    break
                cur.append((int(got['asked'][n, k]), bool(got['answer'][n, k])))
            assert (got['label'][n, na + 1:] == -1).all() and (got['label_conf'][n, na + 1:] == -1).all()
            assert (got['label_hit'][n, na + 1:] == -1).all()
    print('T=%d: max |label_conf - ref| = %.3e, |label_hit - ref| = %.3e (bar %.0e); %d labels within %.0e of their runner-up, reference R '
          'lost there = %.3e (bar %.0e); %d decisions compared, %d near a threshold skipped'
          % (T, d['conf'], d['hit'], PROB_BAR, close_labels, SL.MARGIN, d['tie'], TIE_BAR, compared, skipped))
    assert d['conf'] <= PROB_BAR
    assert d['hit'] <= PROB_BAR
    assert d['tie'] <= TIE_BAR
    assert skipped <= 0.05 * (compared + skipped)


# ---------------------------------------------------------------------------------------------------------------- 3. edges and memory
def _edge_set(dev):
    """seven rows of case(33), ld = 40: 0 plain | 1 a NaN logit | 2 v = 1 | 3 a list of 60 points | 4 budget 0 | 5 budget above qmax |
    6 contradictory at the start | 7 empty (vlen 0)"""
    c = Q.case(33)
    pick = [0, 1, 8, 2, 3, 4, 5, 6]
    s, e = c['s'][pick].clone(), c['e'][pick].clone()
    s[1, 2] = float('nan')
    vlen = c['vlen'].numpy()[pick].copy()
    assert vlen[2] == 1 and vlen[6] >= 3
    vlen[7] = 0
    aps = [[], [], [], [(0, False)] * 60, [], [], [(0, True), (2, True), (1, False)], []]
    budget = np.array([6, 6, 6, 6, 0, 99, 6, 6], dtype=np.int32)
    return pad_logits(dev, s, 40, 3), pad_logits(dev, e, 40, 4), vlen, [33] * 8, aps, c['gt'][pick], budget


def test_edge_rows(dev):
    s, e, vlen, tlen, aps, gt, budget = _edge_set(dev)
    for eps in (0.0, 0.2):
        for stop_hit, stop_m in ((-1.0, 0), RULE):
            kw = dict(budget=budget, eps=eps, stop_hit=stop_hit, stop_m=stop_m)
            got = run_label_session(dev, s, e, vlen, tlen, aps, gt, 6, **kw)
            want, _ = host_loop(dev, s, e, vlen, tlen, aps, gt, 6, **kw)
            assert_same(got, want)
            np.testing.assert_array_equal(got['stop_reason'][[1, 3, 7]], [S.POISONED, S.OVERFLOW, S.POISONED])
            np.testing.assert_array_equal(got['n_asked'][[1, 2, 3, 4, 7]], [0, 0, 0, 0, 0])
            for n in (1, 3, 7):                                       # no pass was live: no label
                assert (got['label'][n] == -1).all() and (got['label_conf'][n] == -1).all() and (got['label_hit'][n] == -1).all()
            # one frame: the label is that frame, certainly
            np.testing.assert_array_equal(got['label'][2, 0], [0, 0])
            assert got['label_conf'][2, 0] == 1.0 and (got['label_hit'][2, 0] == 1.0).all()
            assert got['stop_reason'][2] == (SL.RELIABLE if stop_hit > 0 else S.GAIN)
            assert got['stop_reason'][4] in (S.BUDGET, SL.RELIABLE) and got['label'][4, 0, 0] >= 0      # budget 0: one pass, one label
            if eps == 0.0:
                assert got['stop_reason'][6] == S.CONTRADICTORY and (got['label'][6] == -1).all()
            else:
                assert got['label'][6, 0, 0] >= 0                     # under noise no list is contradictory


def test_sel_with_a_repeated_and_an_outside_id(dev):
    s, e, vlen, tlen, aps, gt, budget = _edge_set(dev)
    for eps in (0.0, 0.2):
        kw = dict(budget=budget, eps=eps, stop_hit=RULE[0], stop_m=RULE[1])
        full = run_label_session(dev, s, e, vlen, tlen, aps, gt, 6, **kw)
        part = run_label_session(dev, s, e, vlen, tlen, aps, gt, 6, sel=[5, 0, 77, 0, -3, 2], selected=[0, 2, 5], **kw)
        assert_same(part, full, rows=[0, 2, 5])


def _raw(lib, aset, s, e, gt, nsel, qmax, thr, M, stop_m, stop_hit, outs, eps=0.0, min_gain=0.0):
    return lib.load().hual_al_session_label(ctypes.byref(aset), lib.ptr(s), lib.ptr(e), lib.ptr(gt), None, nsel, qmax, None, -1.0, min_gain, eps,
                                            None, thr, M, stop_m, stop_hit, *outs, lib.stream_ptr())


def test_a_row_longer_than_256_frames_is_poisoned(dev):
    """tlen is device memory, so the C entry point cannot refuse it (lib.al_session_label does, on the host): the raw call"""
    from hual_amd import lib
    c = Q.case(33)
    N, ld, qmax = 2, 300, 4
    s = pad_logits(dev, c['s'][:2], ld, 5)
    e = pad_logits(dev, c['e'][:2], ld, 6)
    aset, keep = make_set(dev, [300, 33], [300, 33], [[], []], ld)
    with pytest.raises(lib.HualError):
        lib.al_session_label(aset, s, e, np.array([300, 33]), _i32(dev, c['gt'][:2]), qmax)
    bufs = [_sentinel(shape, dt, dev, FILL[k]) for k, (shape, dt) in zip(NAMES, _specs(N, qmax))]
    gt = _i32(dev, c['gt'][:2])
    thr = (ctypes.c_int32 * 6)(*[x for nd in THR for x in nd])
    lib.check(_raw(lib, aset, s, e, gt, N, qmax, thr, 3, 2, -1.0, [lib.ptr(b[0]) for b in bufs]))
    torch.cuda.synchronize()
    r = {k: b[0].cpu().numpy() for k, b in zip(NAMES, bufs)}
    assert all(_pads_intact(b[1], b[2], FILL[k]) for k, b in zip(NAMES, bufs))
    assert r['stop_reason'][0] == S.POISONED and r['n_asked'][0] == 0 and (r['label'][0] == -1).all() and (r['label_hit'][0] == -1).all()
    assert r['stop_reason'][1] == S.BUDGET and r['n_asked'][1] == qmax and (r['label'][1] >= 0).all()


def test_the_entry_point_accepts_what_the_checks_leave(dev):
    """the argument errors are tests/test_al_session_label.py's (no GPU); here the same raw call with valid arguments succeeds"""
    from hual_amd import lib
    s, e, vlen, tlen, aps, gt, budget = _edge_set(dev)
    aset, keep = make_set(dev, vlen, tlen, aps, 40)
    outs = [torch.zeros(shape, dtype=dt, device=dev) for shape, dt in _specs(8, 6)]
    thr = (ctypes.c_int32 * 6)(*[x for nd in THR for x in nd])
    assert _raw(lib, aset, s, e, _i32(dev, gt), 8, 6, thr, 3, 2, 0.9, [lib.ptr(o) for o in outs]) == 0
    assert _raw(lib, aset, s, e, _i32(dev, gt), 8, 6, thr, 3, 3, 0.9, [lib.ptr(o) for o in outs]) < 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- 4. graph capture
def test_second_launch_and_graph_replay(dev):
    from hual_amd import lib
    T = 70
    c = Q.case(T)
    s, e = case_logits(dev, T, 7)
    vlen, tlen, lists = c['vlen'].numpy(), [T] * Q.N_ROWS, S.start_list(T, 3)
    fm = S.flip_masks(T)
    for eps in (0.0, 0.05):
        kw = dict(stop_hit=RULE[0], stop_m=RULE[1], eps=eps)
        want = run_label_session(dev, s, e, vlen, tlen, lists, c['gt'], 6, flip=fm, **kw)
        assert_same(run_label_session(dev, s, e, vlen, tlen, lists, c['gt'], 6, flip=fm, **kw), want)
        aset, keep = make_set(dev, vlen, tlen, lists, T + 7)
        gt, flip = _i32(dev, c['gt']), _u32(dev, fm)
        out = tuple(torch.zeros(shape, dtype=dt, device=dev) for shape, dt in _specs(Q.N_ROWS, 6))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            lib.al_session_label(aset, s, e, np.asarray(tlen), gt, 6, thresholds=THR, flip=flip, out=out, **kw)      # (warm-up: the module is loaded)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            lib.al_session_label(aset, s, e, np.asarray(tlen), gt, 6, thresholds=THR, flip=flip, out=out, **kw)
        for _ in range(2):
            for o in out:
                o.fill_(5)
            graph.replay()
            torch.cuda.synchronize()
            assert_same({k: o.cpu().numpy() for k, o in zip(NAMES, out)}, want)


# ---------------------------------------------------------------------------------------------------------------- 5. the updater, the label update
def _updater(RS):
    from hual_amd import al
    return al.LabelUpdater(RS['prop'], [[] for _ in range(RS['N'])])


def _gt_idx(RS, up):
    from hual_amd import al
    return np.array([[al._round_half_even_index(t, RS['data_gt'][i][1], int(up.vlen_h[i])) for t in RS['data_gt'][i][2]]
                     for i in range(RS['N'])])


@pytest.mark.parametrize('noise', [None, 0.1])
def test_label_updater_session_label(dev, noise):
    from hual_amd import lib
    RS = _round_set()
    N = RS['N']
    up, plain, ref = _updater(RS), _updater(RS), _updater(RS)
    gt = _gt_idx(RS, up)
    flips = np.random.default_rng(11).integers(0, 8, N).astype(np.uint32)
    sel = np.arange(0, N, 2)
    (asked, answers, n_asked), launches = _prof(lambda: up.session_label(gt, 3, stop_hit=0.9, noise=noise, flips=flips, sel=sel))
    assert sum(launches.values()) == 1 and 'al_session_label' in list(launches)[0], launches
    assert up.tilt_eps is None                                        # the new lists invalidate a tilt
    reason, na = up.stop_reason.cpu().numpy(), up.n_asked.cpu().numpy()
    assert (reason[1::2] == -1).all() and (up.label_path.cpu().numpy()[1::2] == -1).all()
    assert up.label_path.shape == (N, 4, 2) and up.label_conf_path.shape == (N, 4) and up.label_hit_path.shape == (N, 4, 3)
    for i in range(N):
        assert up.aps[i] == [(int(asked[i, k]), bool(answers[i, k])) for k in range(int(n_asked[i]))]
    # the final label is the label of the installed lists, the final reliability its hit probability
    final = np.clip(na, 0, None)
    lab = up.label_path.cpu().numpy()[np.arange(N), final]
    new_idx, conf, _ = up.mbr_label(sel, np.zeros((N, 2), dtype=np.int32), noise=noise)
    np.testing.assert_array_equal(lab[sel], new_idx[sel])
    np.testing.assert_array_equal(up.label_conf_path.cpu().numpy()[np.arange(N), final][sel].view(np.int32), conf[sel].view(np.int32))
    up.hit_label(sel=sel, cand=new_idx[:, None, :], best=False, noise=noise)
    np.testing.assert_array_equal(up.label_hit_path.cpu().numpy()[np.arange(N), final][sel].view(np.int32),
                                  up.cand_hit.cpu().numpy()[sel, 0].view(np.int32))
    rel = reason == lib.AL_STOP_REASONS.index('reliable')
    assert (up.label_hit_path.cpu().numpy()[np.arange(N), final, 2][rel] >= np.float32(0.9)).all()
    # the rule only ever ends a session earlier: the same session without it is a continuation
    plain.session(gt, 3, noise=noise, flips=flips, sel=sel)
    pa, pn = plain.asked.cpu().numpy(), plain.n_asked.cpu().numpy()
    assert (na[sel] <= pn[sel]).all()
    for i in sel:
        np.testing.assert_array_equal(asked[i, :na[i]], pa[i, :na[i]])
    # stop_hit=None: session()'s tensors bit for bit
    ref.session_label(gt, 3, noise=noise, flips=flips, sel=sel)
    for k in ('asked', 'answers', 'q_asked', 'session_gain', 'entropy_path', 'n_asked', 'stop_reason'):
        assert torch.equal(getattr(ref, k), getattr(plain, k)), k
    assert ref.aps == plain.aps
    with pytest.raises(ValueError, match='stop_at'):
        up.session_label(gt, 3, stop_hit=0.9, stop_at=0.6)
    with pytest.raises(ValueError, match='stop_hit'):
        up.session_label(gt, 3, stop_hit=0.0)


@pytest.mark.parametrize('noise', [None, 0.1])
def test_update_labels_with_stop_hit(dev, noise):
    from hual_amd import al, lib
    RS = _round_set()
    N, prop, coff = RS['N'], RS['prop'], al.get_coff('charades', 1)
    kw = dict(observe_by='info_gain', renew_by='posterior', answer_noise=noise, questions_per_clip=3, return_debug=True)

    def run(**more):
        return _prof(lambda: al.update_labels(copy.deepcopy(RS['data_old']), RS['data_gt'], prop, coff, **kw, **more))
    (new, d), launches = run(stop_hit=0.9)
    assert sum(v for k, v in launches.items() if 'al_session_label' in k) == 1, launches
    assert sum(v for k, v in launches.items() if 'al_session' in k) == 1, launches          # in place of the session's launch
    (base, d0), launches0 = run()
    assert not any('al_session_label' in k for k in launches0)
    reliable = lib.AL_STOP_REASONS.index('reliable')
    in_session = np.flatnonzero(d['stop_reason'] >= 0)
    assert len(in_session) and (d['stop_reason'][in_session] == reliable).any()
    np.testing.assert_array_equal(in_session, np.flatnonzero(d0['stop_reason'] >= 0))
    # the session's final label is the renew's
    final = d['n_asked'][in_session]
    live = d['label_path'][in_session, final, 0] >= 0
    assert live.any()
    np.testing.assert_array_equal(d['label_path'][in_session, final][live], d['new_idx'][in_session][live])
    np.testing.assert_array_equal(d['label_conf_path'][in_session, final][live].view(np.int32), d['label_conf'][in_session][live].view(np.int32))
    assert d['label_hit_path'].shape == (N, 4, 3)
    rel = in_session[d['stop_reason'][in_session] == reliable]
    assert (d['label_hit_path'][rel, d['n_asked'][rel], 2] >= np.float32(0.9)).all()
    # a row that stopped as reliable asked no more than in the same round without the rule
    assert (d['n_asked'][rel] <= d0['n_asked'][rel]).all()
    out = np.setdiff1d(np.arange(N), in_session)
    assert (d['label_path'][out] == -1).all() and (d['label_hit_path'][out] == -1).all()
    # stop_hit=None is the call without the argument
    (same, d1), launches1 = run(stop_hit=None)
    assert same == base and launches1 == launches0 and sorted(d1) == sorted(d0)
    for k in d0:
        if k != 'updater':
            np.testing.assert_array_equal(d1[k], d0[k], err_msg=k)
