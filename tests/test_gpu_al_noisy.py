"""GPU: the span posterior under an annotator who errs - hual_al_noisy_tilt (the answers folded into the logits, and their evidence),
the launches of the family on the tilted rows through LabelUpdater(noise=), hual_al_label_gain_noisy against the float64 enumeration of
its contract (tests/al_noisy_ref.py), candidate lists, subsets, edge rows, the memory they must not touch, graph capture, and the
place they land: al.update_labels(answer_noise=, annotator_flip=).

The bars (from the contract's arithmetic, include/hual_seqpan.h; not tuned):
  s_t, e_t               every bit of the numpy float32 restatement (one product, one addition, each rounded on its own).
  log_evidence           1e-6 relative: float64 sums, one rounding to float32 (6e-8).
  incl, marginals, conf  1e-6 absolute, post_entropy 5e-5 bits, the label itself: the family's own bars, against the float64 enumeration of
                         the posterior the tilted rows define (tests/test_al_noisy.py holds that posterior within 1e-5 of the direct one).
  channel gain           1e-6 of h2(eps + (1 - 2 eps) q) - h2(eps) in float64 at the launch's own q: one rounding to float32 of a value <= 1.
  gain, ask_gain, value  1e-6 absolute, as hual_al_label_gain: float32 probabilities shared bit for bit with the reference, float64 sums
                         of non-negative terms, a difference of three values <= 1, one final rounding to float32.
  ask_point              exact on every state whose reference margin between the best and the second-best frame exceeds 1e-5
                         (tests/test_al_noisy.py counts them); on the others the kernel's frame has a reference gain within 2e-6 of the best."""
import copy

import numpy as np
import pytest
import torch

import al_label_ref as L
import al_noisy_ref as NR
import al_query_ref as Q
from test_al_noisy import BY_INDEX, CASES
from test_gpu_al_label import run_label
from test_gpu_al_query import _pads_intact, _prof, _sentinel, make_set, pad_logits

pytestmark = pytest.mark.gpu

BAR = 1e-6
FILL, IFILL = 777.0, 777
NAMES = ('gain', 'ask_point', 'ask_gain', 'value')
TILT_TS = (2, 33, 70, 256)


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


def run_tilt(dev, s, e, vlen, tlen, aps, eps):
    """one launch into sentinel-filled outputs -> (s_t, e_t, log_evidence) numpy, after checking the memory around and beyond them"""
    from hual_amd import lib
    N, ld = s.shape
    aset, keep = make_set(dev, vlen, tlen, aps, ld)
    bufs = [_sentinel((N, ld), torch.float32, dev, FILL), _sentinel((N, ld), torch.float32, dev, FILL), _sentinel((N,), torch.float32, dev, FILL)]
    out = tuple(b[0] for b in bufs)
    got = lib.al_noisy_tilt(aset, s, e, np.asarray(tlen), eps, out=out)
    assert all(a is b for a, b in zip(got, out))
    torch.cuda.synchronize()
    for b in bufs:
        assert _pads_intact(b[1], b[2], FILL)
    s_t, e_t, ev = (o.cpu().numpy() for o in out)
    assert not (ev == FILL).any()
    beyond = np.arange(ld)[None, :] >= np.minimum(np.asarray(tlen), ld)[:, None]
    for y in (s_t, e_t):
        assert (y[beyond] == FILL).all()                              # columns [tlen, ld) keep their fill
    return s_t, e_t, ev, out


def run_noisy_gain(dev, s_t, e_t, vlen, tlen, eps, sel=None, cand=None, frames=True, aps=None):
    """one launch on tilted device rows into sentinel-filled outputs -> dict of numpy arrays, after checking the memory around and
    beyond them.  sel: sample ids (any order; ids outside [0, N) must write nothing) or None = all; aps: the set's active points, which
    the launch must not read (None: none)"""
    from hual_amd import lib
    N, ld = s_t.shape
    aset, keep = make_set(dev, vlen, tlen, aps if aps is not None else [[] for _ in range(N)], ld)
    bufs = [_sentinel((N, ld), torch.float32, dev, FILL) if frames else None, _sentinel((N,), torch.int32, dev, IFILL),
            _sentinel((N,), torch.float32, dev, FILL), _sentinel((N,), torch.float32, dev, FILL)]
    out = tuple(b[0] if b is not None else None for b in bufs)
    sel_d = torch.from_numpy(np.asarray(sel, dtype=np.int32)).to(dev) if sel is not None else None
    cand_d = torch.from_numpy(np.ascontiguousarray(cand, dtype=np.int32)).to(dev) if cand is not None else None
    got = lib.al_label_gain_noisy(aset, s_t, e_t, np.asarray(tlen), eps, sel=sel_d, cand=cand_d, frames=frames, out=out)
    assert all(a is b for a, b in zip(got, out))
    torch.cuda.synchronize()
    for b, fill in zip(bufs, (FILL, IFILL, FILL, FILL)):
        if b is not None:
            assert _pads_intact(b[1], b[2], fill)
    r = {k: (o.cpu().numpy() if o is not None else None) for k, o in zip(NAMES, out)}
    written = np.zeros(N, dtype=bool)
    written[np.arange(N) if sel is None else [i for i in sel if 0 <= i < N]] = True
    for k, fill in zip(NAMES[1:], (IFILL, FILL, FILL)):               # only the selected rows are written, and all of them
        assert (r[k][~written] == fill).all() and not (r[k][written] == fill).any(), k
    if frames:                                                        # of a selected row the columns [0, tlen), nothing else
        inside = written[:, None] & (np.arange(ld)[None, :] < np.minimum(np.asarray(tlen), ld)[:, None])
        assert (r['gain'][~inside] == FILL).all() and not (r['gain'][inside] == FILL).any()
    return r


def tilted_on_device(dev, T, eps, h, extra=0):
    """the rows of al_noisy_ref.case(T) after history h, tilted by eps ON THE DEVICE -> (s_t, e_t device [16, T + extra], the case)"""
    c = NR.case(T)
    ld = T + extra
    s, e = pad_logits(dev, c['s'], ld, 1), pad_logits(dev, c['e'], ld, 2)
    _, _, _, out = run_tilt(dev, s, e, c['vlen'].numpy(), [T] * Q.N_ROWS, c['naps'][h], eps)
    return out[0], out[1], c


def check_row(r, n, ref, T_n):
    """row n of a launch over the frames ref['frames'] against its reference -> (|gain - ref|, |ask_gain - ref|, |value - ref|, was the
    frame compared by index)"""
    if ref['status'] != NR.LIVE:
        assert r['ask_point'][n] == -1 and r['ask_gain'][n] == -1.0 and r['value'][n] == -1.0 and (r['gain'][n, :T_n] == 0).all(), n
        return 0.0, 0.0, 0.0, False
    v = len(ref['gain'])
    g = r['gain'][n, :v]
    assert (r['gain'][n, v:T_n] == 0).all() and g.min() >= 0.0 and g.max() <= 1.0
    assert (g[[t for t in range(v) if t not in ref['frames']]] == 0).all()
    d = (float(np.abs(g.astype(np.float64) - ref['gain']).max()), abs(float(r['ask_gain'][n]) - ref['ask_gain']),
         abs(float(r['value'][n]) - ref['value']))
    ap = int(r['ask_point'][n])
    if not ref['frames']:
        assert ap == -1 and r['ask_gain'][n] == 0.0
        return d + (False,)
    assert ap in ref['frames'] and r['ask_gain'][n] == g[ap] == g.max(), (n, ap)
    if NR.by_index(ref):
        assert ap == ref['ask_point'], (n, ap, ref['ask_point'], ref['margin'])
    elif ref['ask_gain'] > 1e-9:                                      # a runner-up within ten bars: any frame within the bar on either side
        assert ref['ask_gain'] - ref['gain'][ap] <= 2 * BAR, (n, ap, ref['ask_point'])
    else:
        assert r['ask_gain'][n] <= BAR, n
    return d + (NR.by_index(ref),)


# ---------------------------------------------------------------------------------------------------------------- 1. the tilt
@pytest.mark.parametrize('eps', NR.EPS + (0.5,))
@pytest.mark.parametrize('T', TILT_TS)
def test_tilt_is_the_numpy_restatement_bit_for_bit(dev, T, eps):
    c = NR.case(T)
    ld = T + 7
    s, e = pad_logits(dev, c['s'], ld, 1), pad_logits(dev, c['e'], ld, 2)
    sn, en = s.cpu().numpy(), e.cpu().numpy()
    vl, tl = c['vlen'].numpy(), [T] * Q.N_ROWS
    worst = 0.0
    for h in NR.HISTORIES:
        s_t, e_t, ev, _ = run_tilt(dev, s, e, vl, tl, c['naps'][h], eps)
        ws, we = NR.tilt_set(sn, en, vl, tl, c['naps'][h], eps)
        assert (bits(s_t[:, :T]) == bits(ws[:, :T])).all() and (bits(e_t[:, :T]) == bits(we[:, :T])).all(), (T, eps, h)
        for n in range(Q.N_ROWS):
            v = int(c['v'][n])
            assert (bits(s_t[n, v:T]) == bits(sn[n, v:T])).all() and (bits(e_t[n, v:T]) == bits(en[n, v:T])).all()      # raw copies
            if eps == 0.5:
                assert (bits(s_t[n, :T]) == bits(sn[n, :T])).all() and (bits(e_t[n, :T]) == bits(en[n, :T])).all()      # the input bits
            want = NR.direct(c['ps'][n], c['pe'][n], v, c['naps'][h][n], eps)['log_evidence']
            if c['naps'][h][n]:
                assert want < 0
                worst = max(worst, abs(float(ev[n]) - want) / abs(want))
            else:
                assert ev[n] == 0.0                                   # (a clip of one frame is never asked about) no answer: ln 1
        assert eps == 0.5 or (bits(s_t[:, :T]) != bits(sn[:, :T])).any()
    print('T=%d eps=%g: tilted rows bit-equal; max relative |log_evidence - ref| = %.2e (bar %.0e)' % (T, eps, worst, BAR))
    assert worst <= BAR


def test_evidence_of_many_answers_and_poisoned_rows(dev):
    T, ld, eps = 33, 40, 1e-6
    c = Q.case(T)
    N = 8
    s, e = c['s'][:N].clone(), c['e'][:N].clone()
    vlen = np.full(N, T, dtype=np.int32)
    tlen = np.full(N, T, dtype=np.int32)
    aps = [[] for _ in range(N)]
    aps[0] = NR.many_answers(T)                                       # 64 clicks, 30 % of them wrong, at eps = 1e-6
    aps[1] = [(5, True)]
    s[1, 3] = float('nan')                                            # a NaN logit below v: poisoned
    vlen[2] = 0                                                       # an empty clip: poisoned
    aps[2] = [(1, False)]
    s[3, 5] = float('inf')                                            # an Inf logit: Z is not finite: poisoned
    aps[3] = [(2, True), (9, False)]
    vlen[4] = 20
    e[4, 30] = float('nan')                                           # a NaN logit at t >= v: not read, copied
    aps[4] = [(4, True), (25, False), (20, True), (-3, False)]        # active points outside [0, v): ignored
    vlen[5], tlen[5] = 20, 25                                         # v < T < ld
    aps[5] = [(5, True), (9, True), (7, False)]                       # a negative inside the positive hull: no contradiction any more
    aps[6] = [(11, False), (11, False), (11, True)]                   # duplicates count once each
    sd, ed = pad_logits(dev, s, ld, 3), pad_logits(dev, e, ld, 4)
    sn, en = sd.cpu().numpy(), ed.cpu().numpy()
    s_t, e_t, ev, _ = run_tilt(dev, sd, ed, vlen, tlen, aps, eps)
    ws, we = NR.tilt_set(sn, en, vlen, tlen, aps, eps, poisoned=(1, 2, 3))
    for n in range(N):
        Tn = int(tlen[n])
        assert (bits(s_t[n, :Tn]) == bits(ws[n, :Tn])).all() and (bits(e_t[n, :Tn]) == bits(we[n, :Tn])).all(), n
    for n in (1, 2, 3):                                               # poisoned: raw columns, NaN evidence
        assert np.isnan(ev[n]) and (bits(s_t[n, :T]) == bits(sn[n, :T])).all() and (bits(e_t[n, :T]) == bits(en[n, :T])).all(), n
    assert ev[7] == 0.0                                               # no answer: ln 1
    for n in (0, 4, 5, 6):
        v = min(int(vlen[n]), int(tlen[n]))
        sr, er = s[n, :tlen[n]].numpy().copy(), e[n, :tlen[n]].numpy().copy()
        sr[v:], er[v:] = 0.0, 0.0                                     # (the columns beyond v are not the posterior's)
        ps, pe = NR.probabilities(sr, er, v)
        want = NR.direct(ps, pe, v, aps[n], eps)['log_evidence']
        assert np.isfinite(ev[n]) and abs(float(ev[n]) - want) <= BAR * abs(want), (n, ev[n], want)
    assert ev[0] < -100.0


# ---------------------------------------------------------------------------------------------------------------- 2. the family
def _records(c):
    return [{'vid': 'v%d' % n, 'v_len': int(c['vlen'][n]), 'prop_logits': (c['s'][n].numpy(), c['e'][n].numpy()),
             'prop_logits1': (c['s'][n].numpy(), c['e'][n].numpy()), 'prop_logits2': (c['s'][n].numpy(), c['e'][n].numpy())}
            for n in range(Q.N_ROWS)]


@pytest.mark.parametrize('T,eps', CASES)
def test_family_on_tilted_rows_through_the_updater(dev, T, eps):
    from hual_amd import al
    c = NR.gain_case(T, eps)
    rec = _records(c)
    d = dict(incl=0.0, entropy=0.0, marg=0.0, conf=0.0, channel=0.0)
    revived = 0
    e64 = NR.eps64(eps)
    for h in NR.HISTORIES:
        up = al.LabelUpdater(rec, c['naps'][h], device=dev)

        def all_three():
            up.query(noise=eps)
            up.span_marginals(noise=eps)
            return up.mbr_label(np.arange(Q.N_ROWS), np.zeros((Q.N_ROWS, 2), dtype=np.int64), noise=eps)
        (new_idx, conf, _), launches = _prof(all_three)
        assert sum(v for k, v in launches.items() if 'al_noisy_tilt' in k) == 1 and sum(launches.values()) == 4, launches      # one tilt
        assert up.agree is None and up.tilt_eps == e64
        s_t, e_t = up.s_t.cpu().numpy(), up.e_t.cpu().numpy()
        assert (bits(s_t) == bits(c['s_t'][h])).all() and (bits(e_t) == bits(c['e_t'][h])).all()
        incl, gain, qp, qg = (x.cpu().numpy() for x in (up.incl, up.gain, up.query_point, up.query_gain))
        ent, ys, ye, st = (x.cpu().numpy() for x in (up.post_entropy, up.y_start, up.y_end, up.marg_status))
        lev = up.log_evidence.cpu().numpy()
        for n in range(Q.N_ROWS):
            v, q, m = int(c['v'][n]), c['qref'][h][n], c['mref'][h][n]
            assert q['status'] == Q.LIVE and qp[n] >= 0 and st[n] == 1 and new_idx[n, 0] >= 0, (h, n)      # every state is live
            revived += c['hard'][h][n]['status'] == Q.CONTRADICTORY
            d['incl'] = max(d['incl'], float(np.abs(incl[n, :v] - q['incl']).max()))
            d['entropy'] = max(d['entropy'], abs(float(ent[n]) - q['post_entropy']))
            d['marg'] = max(d['marg'], float(np.abs(ys[n, :v] - m['y_start']).max()), float(np.abs(ye[n, :v] - m['y_end']).max()))
            want = Q.h2_64(e64 + (1.0 - 2.0 * e64) * incl[n, :v].astype(np.float64)) - Q.h2_64(e64)
            d['channel'] = max(d['channel'], float(np.abs(gain[n, :v] - want).max()))
            assert (gain[n, v:T] == 0).all() and qg[n] == gain[n, qp[n]] and abs(float(qg[n]) - float(want.max())) <= BAR
            assert abs(float(lev[n]) - c['dir'][h][n]['log_evidence']) <= BAR * abs(c['dir'][h][n]['log_evidence'])
            lr = c['lref'][h][n]
            if lr is not None:
                d['conf'] = max(d['conf'], abs(float(conf[n]) - lr['conf']))
                if lr['margin'] > 10 * BAR:                           # a runner-up ten bars below: the label itself
                    assert tuple(new_idx[n]) == lr['label'], (h, n, new_idx[n], lr['label'], lr['margin'])
                else:
                    assert lr['conf'] - L.span_R(lr['st'], *new_idx[n]) <= 2 * BAR
    print('T=%d eps=%g: %d states contradictory under the hard rule are live; max |incl - ref| %.2e, |entropy - ref| %.2e bits, '
          '|marginal - ref| %.2e, |conf - ref| %.2e, |channel gain - h2| %.2e' % (T, eps, revived, d['incl'], d['entropy'], d['marg'],
                                                                             d['conf'], d['channel']))
    assert revived > 0 or T == 2
    assert d['incl'] <= BAR and d['marg'] <= BAR and d['conf'] <= BAR and d['channel'] <= BAR and d['entropy'] <= 5e-5


# ---------------------------------------------------------------------------------------------------------------- 3. the noisy gain
@pytest.mark.parametrize('h', NR.HISTORIES)
@pytest.mark.parametrize('T,eps', CASES)
def test_noisy_gain_against_the_float64_reference(dev, T, eps, h):
    c = NR.gain_case(T, eps)
    s_t, e_t, _ = tilted_on_device(dev, T, eps, h, extra=7)
    rows = list(NR.ROWS[T])
    sel = None if len(rows) == Q.N_ROWS else rows
    vl, tl = c['vlen'].numpy(), [T] * Q.N_ROWS
    r = run_noisy_gain(dev, s_t, e_t, vl, tl, eps, sel=sel, aps=c['naps'][h])      # (the set's answers are not read: they change nothing)
    d = np.zeros(3)
    by_index = 0
    for n in rows:
        *dn, exact = check_row(r, n, c['gref'][h][n], T)
        d = np.maximum(d, dn)
        by_index += exact
    print('T=%d eps=%g answers=%d: %d of %d rows equal by index; max |gain - ref| = %.3e, |ask_gain - ref| = %.3e, |value - ref| = %.3e '
          '(bar %.0e)' % (T, eps, h, by_index, len(rows), d[0], d[1], d[2], BAR))
    assert by_index == BY_INDEX[(T, eps)][0][NR.HISTORIES.index(h)]
    assert (d <= BAR).all()
    # value is the conf of hual_al_mbr_label on the same rows and a set without answers
    lab = run_label(dev, s_t, e_t, vl, tl, [[] for _ in range(Q.N_ROWS)], sel=sel)
    assert np.abs(r['value'][rows].astype(np.float64) - lab['conf'][rows]).max() <= BAR
    r0 = run_noisy_gain(dev, s_t, e_t, vl, tl, eps, sel=sel)          # the same bits with no answers in the set
    for k in NAMES:
        assert (bits(r0[k][rows]) == bits(r[k][rows])).all() if k != 'ask_point' else (r0[k][rows] == r[k][rows]).all(), k


def test_candidate_lists_subsets_and_a_poisoned_row(dev):
    T, eps, h = 33, 0.2, 3
    c = NR.gain_case(T, eps)
    s_t, e_t, _ = tilted_on_device(dev, T, eps, h)
    vl, tl = c['vlen'].numpy(), [T] * Q.N_ROWS
    full = run_noisy_gain(dev, s_t, e_t, vl, tl, eps)
    v = c['v']
    cand = np.array([[(3 * n + 1) % int(v[n]), -1, int(v[n]) + n % 3, (7 * n + 5) % int(v[n])] for n in range(Q.N_ROWS)])
    r = run_noisy_gain(dev, s_t, e_t, vl, tl, eps, cand=cand)
    for n in range(Q.N_ROWS):
        listed = [int(cand[n, 0]), int(cand[n, 3])]
        want = np.zeros(T, dtype=np.float32)
        want[listed] = full['gain'][n, listed]
        assert (bits(r['gain'][n]) == bits(want)).all(), n            # the same bits at the listed frames, 0 elsewhere
        first = listed[int(np.argmax(want[listed]))]                  # the first listed frame of maximal gain
        assert r['ask_point'][n] == first and r['ask_gain'][n] == want[first], n
        ref = NR.noisy_gain_ref(c['pst'][h][n], c['pet'][h][n], int(v[n]), eps, frames=cand[n])
        assert max(check_row(r, n, ref, T)[:3]) <= BAR
    assert (bits(r['value']) == bits(full['value'])).all()
    none = run_noisy_gain(dev, s_t, e_t, vl, tl, eps, cand=np.tile(np.array([[-1, T]]), (Q.N_ROWS, 1)))
    assert (none['ask_point'] == -1).all() and (none['ask_gain'] == 0).all() and (none['gain'] == 0).all()
    assert (bits(none['value']) == bits(full['value'])).all()
    # a subset in shuffled order with ids outside [0, N): the listed rows only (run_noisy_gain checks the others' fill), the same bits
    sel = [13, Q.N_ROWS + 3, 2, 7, -2, 0, 12]
    part = run_noisy_gain(dev, s_t, e_t, vl, tl, eps, sel=sel)
    ok = [i for i in sel if 0 <= i < Q.N_ROWS]
    for k in NAMES[1:]:
        assert (bits(part[k][ok]) == bits(full[k][ok])).all() if k != 'ask_point' else (part[k][ok] == full[k][ok]).all(), k
    assert (bits(part['gain'][ok]) == bits(full['gain'][ok])).all()
    nof = run_noisy_gain(dev, s_t, e_t, vl, tl, eps, frames=False)   # gain = NULL writes only the [N] outputs, and the same ones
    assert nof['gain'] is None and (nof['ask_point'] == full['ask_point']).all() and (bits(nof['ask_gain']) == bits(full['ask_gain'])).all()
    # poisoned rows: a NaN logit below v, an empty clip, an Inf logit; a NaN at t >= v is not read
    s2, e2 = s_t.clone(), e_t.clone()
    s2[2, 3] = float('nan')
    s2[4, 5] = float('inf')
    e2[5, T - 1] = float('nan')
    vl2 = vl.copy()
    vl2[3], vl2[5] = 0, 20
    bad = run_noisy_gain(dev, s2, e2, vl2, tl, eps)
    for n in (2, 3, 4):
        assert bad['ask_point'][n] == -1 and bad['ask_gain'][n] == -1.0 and bad['value'][n] == -1.0 and (bad['gain'][n] == 0).all(), n
    assert bad['ask_point'][5] >= 0 and (bad['gain'][5, 20:] == 0).all()
    for n in (0, 1, 6, 7):
        assert bad['ask_point'][n] == full['ask_point'][n] and (bits(bad['gain'][n]) == bits(full['gain'][n])).all(), n


def test_two_candidates_at_256_frames(dev):
    """T = v = 256, one row, two frames: the invariants (the enumeration of 32,896 spans against each other does not fit)"""
    T, eps, h = 256, 0.2, 6
    c = NR.case(T)
    s, e = c['s'][:1].contiguous().to(dev), c['e'][:1].contiguous().to(dev)
    assert int(c['v'][0]) == T
    _, _, ev, out = run_tilt(dev, s, e, [T], [T], [c['naps'][h][0]], eps)
    cand = np.array([[c['ref'][h][0]['query_point'], T // 2]])
    r = run_noisy_gain(dev, out[0], out[1], [T], [T], eps, cand=cand)
    lab = run_label(dev, out[0], out[1], [T], [T], [[]])
    print('T=256: gain at %s = %s, value %.6f, conf %.6f' % (cand[0], r['gain'][0, cand[0]], r['value'][0], lab['conf'][0]))
    assert np.isfinite(r['gain'][0]).all() and r['gain'][0].min() >= 0.0 and r['gain'][0].max() <= 1.0
    assert (np.delete(r['gain'][0], cand[0]) == 0).all() and r['ask_point'][0] in cand[0] and r['ask_gain'][0] == r['gain'][0].max()
    assert 0.0 < r['value'][0] <= 1.0 and abs(float(r['value'][0]) - float(lab['conf'][0])) <= BAR
    assert r['gain'][0].max() <= 1.0 - r['value'][0] + BAR


# ---------------------------------------------------------------------------------------------------------------- 4. capture
def test_tilt_and_noisy_gain_in_a_captured_graph(dev):
    from hual_amd import lib
    T, eps, h = 33, 0.2, 3
    c = NR.case(T)
    ld = T + 7
    s, e = pad_logits(dev, c['s'], ld, 1), pad_logits(dev, c['e'], ld, 2)
    vl, tl = c['vlen'].numpy(), np.full(Q.N_ROWS, T)
    aset, keep = make_set(dev, vl, tl, c['naps'][h], ld)
    free, keep2 = make_set(dev, vl, tl, [[] for _ in range(Q.N_ROWS)], ld)

    def outs():
        return ((torch.full((Q.N_ROWS, ld), FILL, device=dev), torch.full((Q.N_ROWS, ld), FILL, device=dev), torch.full((Q.N_ROWS,), FILL, device=dev)),
                (torch.full((Q.N_ROWS, ld), FILL, device=dev), torch.full((Q.N_ROWS,), IFILL, dtype=torch.int32, device=dev),
                 torch.full((Q.N_ROWS,), FILL, device=dev), torch.full((Q.N_ROWS,), FILL, device=dev)))

    def both(o):
        lib.al_noisy_tilt(aset, s, e, tl, eps, out=o[0])
        lib.al_label_gain_noisy(free, o[0][0], o[0][1], tl, eps, out=o[1])
    eager = outs()
    both(eager)
    torch.cuda.synchronize()
    want = [x.cpu().numpy() for x in eager[0] + eager[1]]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        both(outs())                                                  # (warm-up)
    torch.cuda.current_stream().wait_stream(side)
    out = outs()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        both(out)
    for _ in range(2):
        for o in out[0] + out[1]:
            o.fill_(5)
        for o in (out[0][0], out[0][1], out[1][0]):
            o[:, T:] = FILL
        graph.replay()
        torch.cuda.synchronize()
        for o, w in zip(out[0] + out[1], want):
            assert (o.cpu().numpy().view(np.int32) == w.view(np.int32)).all()
    assert (want[3][:, :T] > 0).any()


# ---------------------------------------------------------------------------------------------------------------- 5. the label update
HARD = dict(rank_by='span_risk', renew_by='posterior')
KEYS0 = ['order', 'uncert_video', 'observe', 'uncert_frame', 'sprob', 'eprob', 'new_idx', 'gt_idx', 'old_idx', 'updater']


def _rounds(al, coff, **kw):
    """ROUNDS label updates on al_noisy_ref.round_set() with the erring annotator of the seed -> per round (data, dbg, soft)"""
    S = NR.round_set()
    rng = np.random.default_rng(NR.ROUND_SEED)
    data, out = copy.deepcopy(S['data_old']), []
    for _ in range(NR.ROUNDS):
        soft = {}
        data, dbg = al.update_labels(data, S['data_gt'], S['prop'], coff, return_debug=True, annotator_flip=(NR.ROUND_FLIP, rng),
                                     soft_out=soft, **HARD, **kw)
        out.append((copy.deepcopy(data), dbg, soft))
    return out


def test_update_labels_under_an_erring_annotator(dev):
    from hual_amd import al
    S = NR.round_set()
    N, sel, coff = NR.ROUND_N, S['sel'], al.get_coff('charades', 1)
    insel = np.zeros(N, dtype=bool)
    insel[sel] = True
    flips = NR.annotator_flips()
    # a call without the two new arguments: the launches, keys and results of a call that names their defaults, and no noisy launch
    def plain(**kw):
        return al.update_labels(copy.deepcopy(S['data_old']), S['data_gt'], S['prop'], coff, return_debug=True, **dict(HARD, **kw))
    (new0, d0), k0 = _prof(plain)
    (new0b, d0b), k0b = _prof(lambda: plain(answer_noise=None, annotator_flip=None))
    assert k0 == k0b and sum(k0.values()) == 2 and not any('noisy' in k for k in k0), k0
    assert sorted(d0) == sorted(d0b) == sorted(KEYS0 + ['span_risk', 'label_conf', 'old_conf', 'renewed_by_posterior'])
    assert new0 == new0b and all(np.array_equal(d0[k], d0b[k]) for k in d0 if k != 'updater')
    assert d0['renewed_by_posterior'][sel].all()                      # truthful answers never contradict
    # the hard rule under the erring annotator: the rows whose answers contradict fall back to the reference's renew
    hard = _rounds(al, coff)
    asked = [d['observe'] for _, d, _ in hard]
    broken = NR.replay_hard_rounds(asked, flips)
    fell = 0
    for k, (data, d, soft) in enumerate(hard):
        np.testing.assert_array_equal(d['order'][:len(sel)], sel)
        np.testing.assert_array_equal(d['flipped'], flips[k])
        back = sorted(int(i) for i in sel if not d['renewed_by_posterior'][i])
        assert back == broken[k], (k, back, broken[k])
        lost = np.zeros(N, dtype=bool)
        lost[np.asarray(broken[k], dtype=np.int64)] = True
        assert not soft['live'][lost].any() and soft['live'][insel & ~lost].all()
        assert 'log_evidence' not in d
        fell += len(back)
    print('hard rule: rows without a posterior label per round %s' % [len(b) for b in broken])
    assert fell >= 1
    # the noisy posterior on the same annotator: every selected row is renewed by the posterior, every row has soft labels
    noisy, k1 = _prof(lambda: _rounds(al, coff, answer_noise=0.1))
    for k, (data, d, soft) in enumerate(noisy):
        np.testing.assert_array_equal(d['flipped'], flips[k])
        np.testing.assert_array_equal(d['observe'], asked[k])         # the same questions: observe_by is the reference's
        assert d['renewed_by_posterior'][sel].all() and not d['renewed_by_posterior'][~insel].any()
        assert soft['live'].all() and soft['answered'].all()
        assert sorted(d) == sorted(KEYS0 + ['span_risk', 'label_conf', 'old_conf', 'renewed_by_posterior', 'flipped', 'log_evidence'])
        lev = d['log_evidence']
        assert lev.dtype == np.float32 and np.isfinite(lev).all() and (lev < 0).all()
        assert (d['label_conf'][sel] > 0).all() and (d['label_conf'][sel] <= 1).all()
        for i in sel:
            assert data[i][2] == [float(t) for t in d['new_idx'][i]], i      # (a frame index is its own time on this set)
    # three rounds: score, one tilt, the marginals and the label, each round
    assert sum(k1.values()) == 4 * NR.ROUNDS and sum(v for k, v in k1.items() if 'al_noisy_tilt' in k) == NR.ROUNDS and \
        not any('al_renew' in k for k in k1), k1
    # the rows the hard rule lost carry answers the model finds less likely than the others'
    up = noisy[-1][1]['updater']
    ref = NR.direct(*NR.probabilities(S['prop'][sel[0]]['prop_logits'][0], S['prop'][sel[0]]['prop_logits'][1], int(S['vlen'][sel[0]])),
                    int(S['vlen'][sel[0]]), [(f, True) for f in noisy[-1][0][sel[0]][4]['pos_idx']] +
                    [(f, False) for f in noisy[-1][0][sel[0]][4]['neg_idx']], 0.1)
    assert abs(float(noisy[-1][1]['log_evidence'][sel[0]]) - ref['log_evidence']) <= BAR * abs(ref['log_evidence'])
    assert up.tilt_eps == NR.eps64(0.1)
    # acquisition by the noisy gain: one more tilt (the answers of the earlier rounds) and the new launch in the old one's place
    (new2, d2), k2 = _prof(lambda: plain(answer_noise=0.1, acquire_by='label_gain', rank_by='uncert_video'))
    assert sum(v for k, v in k2.items() if 'al_label_gain_noisy' in k) == 1 and sum(v for k, v in k2.items() if 'al_noisy_tilt' in k) == 2 \
        and sum(k2.values()) == 5, k2
    assert (d2['ask_gain'] >= 0).all() and (d2['ask_gain'] > 0).any() and (d2['ask_gain'] <= 1 - d2['label_value'] + BAR).all()
    np.testing.assert_array_equal(d2['order'], np.argsort(-d2['ask_gain'], kind='stable'))
    # the question by information under noise: the channel's bits, no agree
    (new3, d3) = plain(answer_noise=0.1, observe_by='info_gain')
    assert 'agree' not in d3 and (d3['query_gain'] > 0).all() and (d3['query_gain'] <= 1.0 - float(Q.h2_64(NR.eps64(0.1))) + BAR).all()
