"""GPU: hual_al_evidence_grid - the evidence of a set's answers on a grid of temperatures and error rates and its sum over the set -
against the float64 enumeration of its contract (tests/al_calib_ref.py) and against hual_al_noisy_tilt on rows scaled by torch; the
fold's totals, counts and best cell; edge rows, subsets, the memory it must not touch, graph capture; and the places it lands:
LabelUpdater.calibrate / set_temperature and al.update_labels(calibrate=, temperature=).

The bars (from the contract's arithmetic, include/hual_seqpan.h; not tuned):
  table                  1e-9 * max(1, |ref|): both sides float64 on bit-equal float32 probabilities; the slack is for libm differences.
  (float)table           1e-6 relative to hual_al_noisy_tilt's log_evidence of the torch-scaled row: that output's bar in
                         tests/test_gpu_al_noisy.py.
  total                  1e-9 * the sum of |cell| over the summed rows; two launches give the same bits.
  status, counts         exact; the best cell exact on the cases whose reference margin tests/test_al_calib.py holds above ten bars."""
import copy

import numpy as np
import pytest
import torch

import al_calib_ref as CR
import al_noisy_ref as NR
import al_query_ref as Q
from test_al_calib import ARGMAX_CASES, MARGIN, argmax_case
from test_gpu_al_noisy import _records
from test_gpu_al_query import _pads_intact, _prof, _sentinel, make_set, pad_logits

pytestmark = pytest.mark.gpu

BAR, TILT_BAR = 1e-9, 1e-6
FILL, IFILL = 777.0, 777
NAMES = ('table', 'status', 'total', 'counts')


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def run_grid(dev, s, e, vlen, tlen, aps, inv_tau, eps, sel=None):
    """one call into sentinel-filled outputs -> dict of numpy arrays, after checking the memory around them and the rows of table /
    status that must keep their fill.  sel: sample ids (any order; ids outside [0, N) must write nothing) or None = all"""
    from hual_amd import lib
    N, ld = s.shape
    AB = len(inv_tau) * len(eps)
    aset, keep = make_set(dev, vlen, tlen, aps, ld)
    bufs = [_sentinel((N, AB), torch.float64, dev, FILL), _sentinel((N,), torch.int32, dev, IFILL), _sentinel((AB,), torch.float64, dev, FILL),
            _sentinel((4,), torch.int32, dev, IFILL)]
    out = tuple(b[0] for b in bufs)
    sel_d = torch.from_numpy(np.asarray(sel, dtype=np.int32)).to(dev) if sel is not None else None
    got = lib.al_evidence_grid(aset, s, e, np.asarray(tlen), inv_tau, eps, sel=sel_d, out=out)
    assert all(a is b for a, b in zip(got, out))
    torch.cuda.synchronize()
    for b, fill in zip(bufs, (FILL, IFILL, FILL, IFILL)):
        assert _pads_intact(b[1], b[2], fill)
    r = {k: o.cpu().numpy() for k, o in zip(NAMES, out)}
    written = np.zeros(N, dtype=bool)
    written[np.arange(N) if sel is None else [i for i in sel if 0 <= i < N]] = True
    assert (r['table'][~written] == FILL).all() and not (r['table'][written] == FILL).any()      # only the selected rows, and all of them
    assert (r['status'][~written] == IFILL).all() and np.isin(r['status'][written], (0, 1)).all()
    assert not (r['total'] == FILL).any() and not (r['counts'] == IFILL).any()
    return r


def check_table(got, want, status, want_status, where):
    """every cell within BAR * max(1, |ref|), NaN exactly where the reference is -> the worst ratio to the bar"""
    assert (np.isnan(got) == np.isnan(want)).all(), where
    assert (status == want_status).all(), where
    ok = ~np.isnan(want)
    d = np.abs(got[ok] - want[ok]) / np.maximum(1.0, np.abs(want[ok]))
    return float(d.max()) if d.size else 0.0


def check_fold(r, table, status, answers, sel, where, by_index):
    """total within BAR * the sum of |cell|, counts exact (the best cell where by_index) -> the worst |total - ref| / scale"""
    total, counts, scale = CR.fold(table, status, answers, sel)
    assert list(r['counts'][:3]) == list(counts[:3]), (where, r['counts'], counts)
    assert 0 <= r['counts'][3] < len(total) if counts[0] else r['counts'][3] == -1, where
    if counts[0]:
        assert r['total'][r['counts'][3]] == r['total'].max() and r['counts'][3] == int(np.argmax(r['total'])), where      # the first maximal one
    if by_index:
        assert r['counts'][3] == counts[3], (where, r['counts'], counts)
    d = np.abs(r['total'] - total)
    assert (d <= BAR * np.maximum(scale, 1e-300)).all() or (scale == 0).all() and (r['total'] == 0).all(), (where, d.max())
    return float((d / np.maximum(scale, 1e-300)).max()) if scale.max() > 0 else 0.0


# ------------------------------------------------------------------------------------------------------------- 1. the cells
@pytest.mark.parametrize('name', sorted(CR.GRIDS))
@pytest.mark.parametrize('T', CR.TS)
def test_cells_against_the_float64_reference(dev, T, name):
    c = CR.case(T)
    it, ep = CR.grid(name)
    vl, tl = c['vlen'].numpy(), [T] * Q.N_ROWS
    worst, worst_t, bits = 0.0, 0.0, None
    for extra in (0, 3):
        s, e = pad_logits(dev, c['s'], T + extra, 1), pad_logits(dev, c['e'], T + extra, 2)
        for h in CR.HISTORIES:
            want, st, ans = CR.case_table(T, h, name)
            r = run_grid(dev, s, e, vl, tl, c['naps'][h], it, ep)
            worst = max(worst, check_table(r['table'], want, r['status'], st, (T, name, extra, h)))
            worst_t = max(worst_t, check_fold(r, want, st, ans, None, (T, name, extra, h), (T, h, name, Q.N_ROWS) in ARGMAX_CASES))
            if h == 0:
                assert (r['table'] == 0).all() and (r['total'] == 0).all() and r['counts'][1] == 0      # no answer: ln 1, exactly
            else:
                assert (r['table'][np.isfinite(r['table'])] <= 1e-12).all()                             # a probability
            if extra == 0 and h == 6:
                bits = r['table'].copy()
            elif h == 6:
                assert (r['table'].view(np.int64) == bits.view(np.int64)).all()                         # ld changes no bit
    print('T=%d grid %s: max |cell - ref| / max(1, |ref|) = %.2e, max |total - ref| / sum |cell| = %.2e (bars %.0e)' % (T, name, worst, worst_t, BAR))
    assert worst <= BAR


@pytest.mark.parametrize('T', CR.TS)
def test_cells_against_the_tilt_launch_on_scaled_rows(dev, T):
    """(float)table against hual_al_noisy_tilt's log_evidence of the rows torch scaled: the product is torch's, the probabilities the
    family's, the sum another order"""
    from hual_amd import lib
    c = CR.case(T)
    it, ep = CR.grid('3x2')
    ld = T + 3
    s, e = pad_logits(dev, c['s'], ld, 1), pad_logits(dev, c['e'], ld, 2)
    vl, tl = c['vlen'].numpy(), np.full(Q.N_ROWS, T)
    worst = 0.0
    for h in NR.HISTORIES:
        r = run_grid(dev, s, e, vl, tl, c['naps'][h], it, ep)
        aset, keep = make_set(dev, vl, tl, c['naps'][h], ld)
        for a, k in enumerate(it):
            sk, ek = (s * float(k)).contiguous(), (e * float(k)).contiguous()
            for b, eps in enumerate(ep):
                ev = lib.al_noisy_tilt(aset, sk, ek, tl, float(eps))[2].cpu().numpy()
                got = r['table'][:, a * len(ep) + b].astype(np.float32)
                assert np.isfinite(ev).all() and np.isfinite(got).all()
                nz = ev != 0
                assert (got[~nz] == 0).all()
                worst = max(worst, float((np.abs(got[nz].astype(np.float64) - ev[nz]) / np.abs(ev[nz])).max()) if nz.any() else 0.0)
    print('T=%d: max relative |(float)cell - log_evidence of the tilt launch| = %.2e (bar %.0e)' % (T, worst, TILT_BAR))
    assert worst <= TILT_BAR


@pytest.mark.parametrize('v', (33, 256))
def test_many_answers_stay_finite(dev, v):
    """64 answers at eps = 1e-6: r^64 is far beyond float64, the sums carry it as an exponent"""
    from hual_amd import lib
    c = CR.case(v)
    s, e = c['s'][:1].contiguous().to(dev), c['e'][:1].contiguous().to(dev)
    assert int(c['v'][0]) == v
    aps = [NR.many_answers(v, 64)]
    it, ep = np.array([1.0, CR.inv32(2.0), CR.inv32(0.5)], dtype=np.float32), np.array([1e-6, 0.1], dtype=np.float32)
    r = run_grid(dev, s, e, [v], [v], aps, it, ep)
    want, st, ans = CR.set_table(s.cpu().numpy(), e.cpu().numpy(), [v], [v], aps, it, ep)
    assert np.isfinite(r['table']).all() and r['status'][0] == 1 and r['table'][0, 0] < -100.0 and list(r['counts']) == [1, 64, 0, int(np.argmax(want[0]))]
    worst = check_table(r['table'], want, r['status'], st, v)
    aset, keep = make_set(dev, [v], [v], aps, v)
    ev = lib.al_noisy_tilt(aset, s, e, [v], 1e-6)[2].cpu().numpy()
    print('v=%d: 64 answers at eps = 1e-6: cell %.6f, reference %.6f, the tilt launch %.6f' % (v, r['table'][0, 0], want[0, 0], ev[0]))
    assert worst <= BAR and abs(float(np.float32(r['table'][0, 0])) - float(ev[0])) <= TILT_BAR * abs(float(ev[0]))


# ------------------------------------------------------------------------------------------------------------- 2. the fold
@pytest.mark.parametrize('T,h,name,N', ARGMAX_CASES)
def test_totals_counts_and_best_cell(dev, T, h, name, N):
    c = CR.case(T)
    it, ep = CR.grid(name)
    rows, total, counts, scale = argmax_case(T, h, name, N)
    assert CR.margin(total) > MARGIN * scale.max()                    # (tests/test_al_calib.py: the index is a condition, not luck)
    s, e = c['s'][rows].contiguous().to(dev), c['e'][rows].contiguous().to(dev)
    vl, aps = c['vlen'].numpy()[rows], [c['naps'][h][n] for n in rows]
    r = run_grid(dev, s, e, vl, [T] * N, aps, it, ep)
    again = run_grid(dev, s, e, vl, [T] * N, aps, it, ep)
    assert (r['total'].view(np.int64) == again['total'].view(np.int64)).all() and (r['counts'] == again['counts']).all()
    assert list(r['counts']) == list(counts), (r['counts'], counts)
    d = np.abs(r['total'] - total)
    print('T=%d answers=%d grid %s N=%d: counts %s, max |total - ref| / sum |cell| = %.2e (bar %.0e)' % (T, h, name, N, list(r['counts']),
                                                                                                  float((d / scale).max()), BAR))
    assert (d <= BAR * scale).all()


# ------------------------------------------------------------------------------------------------------------- 3. edges, subsets
def test_edge_rows(dev):
    T, ld = 33, 40
    c = Q.case(T)
    N = 8
    s, e = c['s'][:N].clone(), c['e'][:N].clone()
    vlen, tlen = np.full(N, T, dtype=np.int32), np.full(N, T, dtype=np.int32)
    aps = [[(3, True), (9, False)] for _ in range(N)]
    s[1, 3] = float('nan')                                            # a NaN logit below v: poisoned at every cell
    vlen[2] = 0                                                       # an empty clip
    tlen[3] = 300                                                     # T > 256 (the binding refuses it; the kernel must as well)
    vlen[4] = 20
    e[4, 30] = float('nan')                                           # a NaN logit at t >= v: not read
    aps[4] = [(4, True), (25, False), (20, True), (-3, False)]        # two of the four lie outside [0, v)
    aps[5] = []                                                       # no answer: every cell 0
    aps[6] = [(40, True), (-1, False)]                                # none inside the clip: the same
    s[7, :2], e[7, :2], vlen[7], tlen[7] = torch.tensor([0.0, 30.0]), torch.tensor([30.0, 0.0]), 2, 2
    aps[7] = [(0, True)]                                              # live at inv_tau = 1, one-hot with the start behind the end at 8
    sd, ed = pad_logits(dev, s, ld, 3), pad_logits(dev, e, ld, 4)
    it, ep = np.array([1.0, 8.0], dtype=np.float32), np.array([0.1, 0.3], dtype=np.float32)
    from hual_amd import lib
    aset, keep = make_set(dev, vlen, tlen, aps, ld)
    with pytest.raises(lib.HualError, match='at most 256'):
        lib.al_evidence_grid(aset, sd, ed, tlen, it, ep)
    host_tlen = np.minimum(tlen, 256)                                 # (past the binding's gate: the device's tlen still says 300)
    out = [_sentinel((N, 4), torch.float64, dev, FILL), _sentinel((N,), torch.int32, dev, IFILL), _sentinel((4,), torch.float64, dev, FILL),
           _sentinel((4,), torch.int32, dev, IFILL)]
    lib.al_evidence_grid(aset, sd, ed, host_tlen, it, ep, out=tuple(o[0] for o in out))
    torch.cuda.synchronize()
    assert all(_pads_intact(o[1], o[2], f) for o, f in zip(out, (FILL, IFILL, FILL, IFILL)))
    table, status, total, counts = (o[0].cpu().numpy() for o in out)
    want, st, ans = CR.set_table(sd.cpu().numpy(), ed.cpu().numpy(), vlen, tlen, aps, it, ep)
    assert check_table(table, want, status, st, 'edges') <= BAR
    for n in (1, 2, 3):
        assert np.isnan(table[n]).all() and status[n] == 0, n
    assert np.isfinite(table[4]).all() and status[4] == 1 and (table[4] < 0).all()
    for n in (5, 6):
        assert (table[n] == 0).all() and status[n] == 1, n
    assert np.isfinite(table[7, :2]).all() and np.isnan(table[7, 2:]).all() and status[7] == 0      # poisoned at one temperature only
    assert list(counts[:3]) == [4, 2 + 1 + 0 + 0, 4]                  # rows 0, 4, 5, 6; row 7 is absent from EVERY total
    ref_total, ref_counts, scale = CR.fold(want, st, ans)
    assert (np.abs(total - ref_total) <= BAR * scale).all() and list(ref_counts[:3]) == list(counts[:3])
    assert (np.abs(total[:2] - (table[0, :2] + table[4, :2])) <= 1e-12).all()


def test_subsets_in_any_order_and_foreign_ids(dev):
    T, h, name = 33, 3, '3x2'
    c = CR.case(T)
    it, ep = CR.grid(name)
    want, st, ans = CR.case_table(T, h, name)
    s, e = pad_logits(dev, c['s'], T + 3, 1), pad_logits(dev, c['e'], T + 3, 2)
    vl, tl = c['vlen'].numpy(), [T] * Q.N_ROWS
    full = run_grid(dev, s, e, vl, tl, c['naps'][h], it, ep)
    for sel in ([13, Q.N_ROWS + 3, 2, 7, -2, 0, 12], [5], [15, 14, 1], [-1, Q.N_ROWS]):
        r = run_grid(dev, s, e, vl, tl, c['naps'][h], it, ep, sel=sel)      # (checks the fill of every row not listed)
        ok = [i for i in sel if 0 <= i < Q.N_ROWS]
        assert (r['table'][ok].view(np.int64) == full['table'][ok].view(np.int64)).all() and (r['status'][ok] == full['status'][ok]).all()
        check_fold(r, want, st, ans, sel, sel, False)
        if not ok:
            assert list(r['counts']) == [0, 0, 0, -1] and (r['total'] == 0).all()
    twice = run_grid(dev, s, e, vl, tl, c['naps'][h], it, ep, sel=[4, 9, 4])      # a repeated id is summed twice
    assert twice['counts'][0] == 3 and (np.abs(twice['total'] - (2 * want[4] + want[9])) <= BAR * np.abs(2 * want[4] + want[9]).max()).all()


# ------------------------------------------------------------------------------------------------------------- 4. capture
def test_grid_in_a_captured_graph(dev):
    from hual_amd import lib
    T, h = 33, 6
    c = CR.case(T)
    it, ep = CR.grid('3x2')
    ld = T + 3
    s, e = pad_logits(dev, c['s'], ld, 1), pad_logits(dev, c['e'], ld, 2)
    vl, tl = c['vlen'].numpy(), np.full(Q.N_ROWS, T)
    aset, keep = make_set(dev, vl, tl, c['naps'][h], ld)

    def outs():
        return (torch.full((Q.N_ROWS, 6), FILL, dtype=torch.float64, device=dev), torch.full((Q.N_ROWS,), IFILL, dtype=torch.int32, device=dev),
                torch.full((6,), FILL, dtype=torch.float64, device=dev), torch.full((4,), IFILL, dtype=torch.int32, device=dev))
    eager = outs()
    lib.al_evidence_grid(aset, s, e, tl, it, ep, out=eager)
    torch.cuda.synchronize()
    want = [x.cpu().numpy() for x in eager]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        lib.al_evidence_grid(aset, s, e, tl, it, ep, out=outs())     # (warm-up)
    torch.cuda.current_stream().wait_stream(side)
    out = outs()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        lib.al_evidence_grid(aset, s, e, tl, it, ep, out=out)
    for _ in range(2):
        for o in out:
            o.fill_(5)
        graph.replay()
        torch.cuda.synchronize()
        for o, w in zip(out, want):
            assert o.cpu().numpy().tobytes() == w.tobytes()
    assert np.isfinite(want[0]).all() and (want[0] < 0).any() and want[3][0] == Q.N_ROWS


# ------------------------------------------------------------------------------------------------------------- 5. the updater
def test_calibrate_finds_the_planted_pair(dev):
    from hual_amd import al
    tau, eps, scale = CR.PLANTED[0]
    p = CR.planted(tau, eps, scale, 0)
    up = al.LabelUpdater(CR.planted_records(p), p['aps'], device=dev)
    fit, launches = _prof(lambda: up.calibrate(at_eps=0.2))
    assert sum(v for k, v in launches.items() if 'al_evidence_grid_kernel' in k) == 3 and sum(launches.values()) == 9, launches
    assert len(fit['grids']) == 3 and fit['rows'] == CR.PLANT_N and fit['answers'] == CR.PLANT_N * CR.PLANT_ANSWERS and fit['excluded'] == 0
    taus, epss, totals = fit['grids'][-1]
    want, counts, sc = CR.set_totals(p, taus, epss)
    ia, ib = divmod(int(np.argmax(want)), len(epss))
    print('planted tau* = %g eps* = %g: fitted tau = %.4f eps = %.4f, per answer %.4f against %.4f at (1, 0.2); reference margin %.3e (bar %.3e)'
          % (tau, eps, fit['tau'], fit['eps'], fit['per_answer'], np.exp(fit['at_default'] / fit['answers']), CR.margin(want), MARGIN * sc.max()))
    assert (np.abs(totals - want) <= BAR * sc.reshape(want.shape)).all()
    assert CR.margin(want) > MARGIN * sc.max()
    assert fit['tau'] == taus[ia] and fit['eps'] == epss[ib] and fit['log_evidence'] == totals[ia, ib]
    assert abs(np.log2(fit['tau'] / tau)) <= 0.5 and abs(fit['eps'] - eps) <= 0.05      # near the planted pair (the coarse cell is test_al_calib's)
    t0, e0, tot0 = fit['grids'][0]
    assert len(t0) == 17 and len(e0) == 10 and fit['at_default'] == tot0[list(t0).index(1.0), list(e0).index(NR.eps64(0.2))]
    assert fit['per_answer'] > np.exp(fit['at_default'] / fit['answers']) and 0.0 < fit['per_answer'] < 1.0
    assert fit['log_evidence'] >= max(g[2].max() for g in fit['grids'][:-1])          # a zoom never loses the best cell
    # below min_answers: no fit, and no launch
    few, launches = _prof(lambda: up.calibrate(min_answers=CR.PLANT_N * CR.PLANT_ANSWERS + 1))
    assert few is None and not launches, launches
    c = CR.case(33)
    small = al.LabelUpdater(_records(c), c['naps'][1], device=dev)
    none, launches = _prof(small.calibrate)
    assert none is None and not launches and sum(len(a) for a in c['naps'][1]) < 32


def _snapshot(up, gt):
    """what the posterior's readers leave on an updater: every output, as bytes"""
    out = []
    up.query()
    out += [up.incl, up.gain, up.query_point, up.query_gain, up.post_entropy, up.agree]
    up.tilt(0.1)
    out += [up.s_t, up.e_t, up.log_evidence]
    up.span_marginals()
    out += [up.y_start, up.y_end, up.marg_status]
    up.span_marginals(noise=0.1)
    out += [up.y_start, up.y_end]
    out += list(up.mbr_label(np.arange(up.N), np.zeros((up.N, 2), dtype=np.int64)))
    out += list(up.mbr_label(np.arange(up.N), np.zeros((up.N, 2), dtype=np.int64), noise=0.1))
    out += list(up.session(gt, 3, noise=0.1))
    out += [up.q_asked, up.session_gain, up.entropy_path, up.stop_reason]
    return [(x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)).tobytes() for x in out]


def test_set_temperature(dev):
    from hual_amd import al
    c = CR.case(33)
    rec, aps, gt = _records(c), c['naps'][3], c['gt']
    fresh = _snapshot(al.LabelUpdater(rec, aps, device=dev), gt)
    for tau in (None, 1.0):
        up = al.LabelUpdater(rec, aps, device=dev)
        up.set_temperature(tau)
        assert up._logits()[0] is up._s0 and up._logits()[1] is up._e0 and up.temperature is None      # the very same tensors
        assert _snapshot(up, gt) == fresh, tau
    half = [dict(r, prop_logits=(r['prop_logits'][0] * np.float32(0.5), r['prop_logits'][1] * np.float32(0.5))) for r in rec]
    want = _snapshot(al.LabelUpdater(half, aps, device=dev), gt)
    up = al.LabelUpdater(rec, aps, device=dev)
    up.set_temperature(2.0)
    got = _snapshot(up, gt)
    assert got == want and got != fresh
    up = al.LabelUpdater(rec, aps, device=dev)                       # (the session above left its answers on the other one)
    up.set_temperature(2.0)
    up.score(0.5)                                                     # score() keeps the unscaled logits
    plain = al.LabelUpdater(rec, aps, device=dev)
    plain.score(0.5)
    assert up.uncert_frame.cpu().numpy().tobytes() == plain.uncert_frame.cpu().numpy().tobytes()
    for bad in (0.0, -1.0, float('nan'), float('inf'), 'hot', True):
        with pytest.raises(ValueError):
            up.set_temperature(bad)
    # the cell of evidence_grid at tau is the evidence tilt() reports under set_temperature(tau)
    up = al.LabelUpdater(rec, aps, device=dev)
    table = up.evidence_grid([2.0], [0.1])[0].cpu().numpy()[:, 0]
    up.set_temperature(2.0)
    up.tilt(0.1)
    ev = up.log_evidence.cpu().numpy()
    assert (np.abs(table.astype(np.float32).astype(np.float64) - ev) <= TILT_BAR * np.abs(ev)).all()


# ------------------------------------------------------------------------------------------------------------- 6. the label update
def _equal(a, b):
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and a.tobytes() == b.tobytes()
    return a == b


def test_update_labels_calibrated_by_evidence(dev):
    from hual_amd import al
    S = NR.round_set()
    coff = al.get_coff('charades', 1)

    def call(**kw):
        return al.update_labels(copy.deepcopy(S['data_old']), S['data_gt'], S['prop'], coff, return_debug=True, **kw)
    (new0, d0), k0 = _prof(lambda: call(observe_by='info_gain'))
    (new1, d1), k1 = _prof(lambda: call(observe_by='info_gain', calibrate=None, temperature=None))
    assert k0 == k1 and not any('evidence' in k for k in k0) and 'calibration' not in d0 and sorted(d0) == sorted(d1)
    assert new0 == new1 and all(_equal(d0[k], d1[k]) for k in d0 if k != 'updater')      # both off: today's call
    (new2, d2), k2 = _prof(lambda: call(observe_by='info_gain', calibrate='evidence'))
    fit = d2['calibration']
    assert fit is not None and fit['answers'] == 2 * NR.ROUND_N and fit['rows'] == NR.ROUND_N and 0 < fit['eps'] <= 0.5 and fit['tau'] > 0
    assert sum(v for k, v in k2.items() if 'al_evidence_grid_kernel' in k) == 3
    assert d2['updater'].temperature == (None if fit['tau'] == 1.0 else fit['tau']) and d2['updater'].tilt_eps == fit['eps']
    new3, d3 = call(observe_by='info_gain', temperature=fit['tau'], answer_noise=fit['eps'])
    assert 'calibration' not in d3 and sorted(d3) == sorted(k for k in d2 if k != 'calibration')
    assert new2 == new3 and all(_equal(d2[k], d3[k]) for k in d3 if k != 'updater')      # the fit, handed in explicitly
    assert 'log_evidence' in d2 and 'agree' not in d2
    few = [r[:4] + [{'pos_idx': r[4]['pos_idx'][:1] if i < 8 else [], 'neg_idx': []}] for i, r in enumerate(copy.deepcopy(S['data_old']))]
    new4, d4 = al.update_labels(few, S['data_gt'], S['prop'], coff, return_debug=True, observe_by='info_gain', calibrate='evidence',
                                answer_noise=0.1)
    assert d4['calibration'] is None and d4['updater'].temperature is None and d4['updater'].tilt_eps == NR.eps64(0.1)      # 8 answers: no fit
