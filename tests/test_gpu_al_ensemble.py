"""GPU: hual_al_ensemble_query and hual_al_ensemble_label (the span posterior as a Bayesian model average over K stochastic passes)
against the float64 enumeration of their contract (tests/al_ens_ref.py), against the single-pass launches at K = 1, their edge rows, the
memory they must not touch, and the places they land: McBank(passes=), LabelUpdater.set_ensemble, al.update_labels(posterior=).

The bars are the family's (include/hual_seqpan.h; not tuned):
  weight, incl, y_start, y_end, conf, old_conf   1e-6 absolute: float32 probabilities shared bit for bit with the reference, float64 sums,
                                                 one final rounding to float32 of a value <= 1 (6e-8).
  log_evidence                                   1e-6 relative to max(1, |ref|): a float64 logarithm rounded to float32.
  gain, query_gain, the entropies, span_bald     5e-5 bits: the float32 h2 of the family; the entropies are float64 sums rounded once.
  query_point / new_idx                          equal wherever the enumeration's runner-up lies 1e-5 bits / 1e-9 tIoU below its best.  The
                                                 rows excused by that are at most 10 % of a case's live rows ON THE REFERENCE ALONE: the
                                                 cases of al_ens_ref.CASES were chosen so (tests/test_al_ensemble.py checks it without a
                                                 GPU), and the test below asserts it again before it reads a device value.
Under eps the device side is the contract's route - one hual_al_noisy_tilt per plane, a set without answers, the planes' log_evidence as
logw - and the reference the direct product of the per-answer likelihoods."""
import copy
import functools

import numpy as np
import pytest
import torch

import al_ens_ref as E
import al_query_ref as Q
from test_gpu_al_query import _answers, _pads_intact, _prof, _round_set, _sentinel, make_set, pad_logits

pytestmark = pytest.mark.gpu

P_BAR, LE_BAR, BIT_BAR = 1e-6, 1e-6, 5e-5
FILL, IFILL = 777.0, 777
Q_NAMES = ('weight', 'log_evidence', 'incl', 'gain', 'query_point', 'query_gain', 'y_start', 'y_end', 'post_entropy', 'expected_entropy',
           'span_bald', 'status')


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def run_query(dev, ps, pe, vlen, tlen, aps, logw=None, host_tlen=None, frames=True, marginals=True):
    """one hual_al_ensemble_query launch into sentinel-filled outputs -> dict of numpy arrays, after checking the memory around and
    beyond them.  ps / pe: device [K, N, ld]"""
    from hual_amd import lib
    K, N, ld = ps.shape
    aset, keep = make_set(dev, vlen, tlen, aps, ld)
    f32, i32 = torch.float32, torch.int32
    spec = [((N, K), f32), ((N,), f32), ((N, ld), f32), ((N, ld), f32), ((N,), i32), ((N,), f32), ((N, ld), f32), ((N, ld), f32), ((N,), f32),
            ((N,), f32), ((N,), f32), ((N,), i32)]
    off = (() if frames else (2, 3)) + (() if marginals else (6, 7))
    bufs = [None if i in off else _sentinel(shape, dt, dev, IFILL if dt == i32 else FILL) for i, (shape, dt) in enumerate(spec)]
    out = tuple(b[0] if b is not None else None for b in bufs)
    got = lib.al_ensemble_query(aset, ps, pe, np.asarray(tlen if host_tlen is None else host_tlen), logw=logw, out=out)
    assert all(a is b for a, b in zip(got, out))
    torch.cuda.synchronize()
    for b in bufs:
        if b is not None:
            assert _pads_intact(b[1], b[2], IFILL if b[0].dtype == i32 else FILL)
    r = {k: (o.cpu().numpy() if o is not None else None) for k, o in zip(Q_NAMES, out)}
    for k in ('weight', 'log_evidence', 'query_point', 'query_gain', 'post_entropy', 'expected_entropy', 'span_bald', 'status'):
        assert not (r[k] == FILL).any(), k                            # every per-row slot was written
    beyond = np.arange(ld)[None, :] >= np.asarray(tlen)[:, None]
    for k in ('incl', 'gain', 'y_start', 'y_end'):
        if r[k] is not None:
            assert (r[k][beyond] == FILL).all() and not (r[k][~beyond] == FILL).any(), k      # columns [tlen, ld) keep their fill
    return r


def run_label(dev, ps, pe, vlen, tlen, aps, logw=None, old=None, sel=None, host_tlen=None):
    """one hual_al_ensemble_label launch into sentinel-filled outputs -> dict of numpy arrays; only the selected rows are written"""
    from hual_amd import lib
    K, N, ld = ps.shape
    aset, keep = make_set(dev, vlen, tlen, aps, ld)
    bufs = [_sentinel((N, 2), torch.int32, dev, IFILL), _sentinel((N,), torch.float32, dev, FILL),
            _sentinel((N,), torch.float32, dev, FILL) if old is not None else None]
    out = tuple(b[0] if b is not None else None for b in bufs)
    sel_d = torch.from_numpy(np.asarray(sel, dtype=np.int32)).to(dev) if sel is not None else None
    old_d = torch.from_numpy(np.ascontiguousarray(old, dtype=np.int32)).to(dev) if old is not None else None
    lib.al_ensemble_label(aset, ps, pe, np.asarray(tlen if host_tlen is None else host_tlen), logw=logw, sel=sel_d, old_idx=old_d, out=out)
    torch.cuda.synchronize()
    for b, fill in zip(bufs, (IFILL, FILL, FILL)):
        if b is not None:
            assert _pads_intact(b[1], b[2], fill)
    r = {k: (o.cpu().numpy() if o is not None else None) for k, o in zip(('new_idx', 'conf', 'old_conf'), out)}
    written = np.zeros(N, dtype=bool)
    ids = np.arange(N) if sel is None else np.asarray(sel)
    written[ids[(ids >= 0) & (ids < N)]] = True
    for k, fill in (('new_idx', IFILL), ('conf', FILL), ('old_conf', FILL)):
        if r[k] is not None:
            assert (r[k][~written] == fill).all() and not (r[k][written] == fill).any(), k
    return r


def device_rows(dev, c):
    """what the launches read for the shared case c: (planes s, planes e, aps, logw) on the device - under eps every plane tilted by
    hual_al_noisy_tilt, no answers, and the planes' log_evidence (plus the case's prior) as logw"""
    from hual_amd import lib
    K, N, ld = c['K'], E.N_ROWS, c['ld']
    ps = torch.stack([pad_logits(dev, c['pass_s'][k, :, :c['T']], ld, 10 + k) for k in range(K)]).contiguous()
    pe = torch.stack([pad_logits(dev, c['pass_e'][k, :, :c['T']], ld, 40 + k) for k in range(K)]).contiguous()
    logw = None if c['logw'] is None else torch.from_numpy(c['logw']).to(dev)
    if c['eps'] is None:
        return ps, pe, c['aps'], logw
    tlen = [c['T']] * N
    aset, keep = make_set(dev, c['vlen'].numpy(), tlen, c['aps'], ld)
    st, et, lev = torch.zeros_like(ps), torch.zeros_like(pe), torch.empty(K, N, device=dev)
    for k in range(K):
        lib.al_noisy_tilt(aset, ps[k], pe[k], np.asarray(tlen), c['eps'], out=(st[k], et[k], lev[k]))
    torch.cuda.synchronize()
    return st, et, [[] for _ in range(N)], (lev if logw is None else (lev + logw).contiguous())


_GOT = {}


def got(dev, cs):
    if cs not in _GOT:
        c = E.case(*cs)
        ps, pe, aps, logw = device_rows(dev, c)
        vlen, tlen = c['vlen'].numpy(), [c['T']] * E.N_ROWS
        sel = list(range(E.N_ROWS))                                   # every row is labelled: the reference enumerates R on all of them
        _GOT[cs] = (run_query(dev, ps, pe, vlen, tlen, aps, logw=logw),
                    run_label(dev, ps, pe, vlen, tlen, aps, logw=logw, old=c['old'], sel=sel), sel, (ps, pe, aps, logw))
    return _GOT[cs]


# ---------------------------------------------------------------------------------------------------------------- 1. values
@pytest.mark.parametrize('cs', E.CASES, ids=lambda cs: 'T%d-K%d-h%d-%s-%s-pad%d' % (cs[0], cs[1], cs[2], 'eps' if cs[3] else 'hard',
                                                                                     'logw' if cs[4] else 'nologw', cs[5]))
def test_values_against_the_float64_enumeration(dev, cs):
    c = E.case(*cs)
    ref, v = c['ref'], c['v']
    live = [n for n in range(E.N_ROWS) if ref[n]['status'] == E.LIVE]
    ex_q = E.excused(ref, 'query_gain', 'runner_gain', 1e-5)
    ex_l = E.excused(ref, 'conf', 'runner_conf', 1e-9)
    assert len(live) == E.N_ROWS and 10 * len(ex_q) <= len(live) and 10 * len(ex_l) <= len(live)      # on the reference alone
    r, lab, sel, _ = got(dev, cs)
    assert len(sel) == E.N_ROWS and all('members' in x for x in ref)
    d = dict(weight=0.0, incl=0.0, y=0.0, le=0.0, gain=0.0, ent=0.0, conf=0.0, old=0.0)
    for n in live:
        x = ref[n]
        assert r['status'][n] == 1
        d['weight'] = max(d['weight'], np.abs(r['weight'][n] - x['weight']).max())
        d['incl'] = max(d['incl'], np.abs(r['incl'][n, :v[n]] - x['incl']).max())
        d['y'] = max(d['y'], np.abs(r['y_start'][n, :v[n]] - x['y_start']).max(), np.abs(r['y_end'][n, :v[n]] - x['y_end']).max())
        d['le'] = max(d['le'], abs(float(r['log_evidence'][n]) - x['log_evidence']) / max(1.0, abs(x['log_evidence'])))
        d['gain'] = max(d['gain'], np.abs(r['gain'][n, :v[n]] - x['gain']).max(), abs(float(r['query_gain'][n]) - x['query_gain']))
        d['ent'] = max(d['ent'], abs(float(r['post_entropy'][n]) - x['post_entropy']), abs(float(r['expected_entropy'][n]) - x['expected_entropy']),
                       abs(float(r['span_bald'][n]) - x['span_bald']))
        for k in ('incl', 'gain', 'y_start', 'y_end'):
            assert (r[k][n, v[n]:c['T']] == 0).all(), k                # 0 at t >= v
        if n not in ex_q:
            assert int(r['query_point'][n]) == x['query_point'], (n, int(r['query_point'][n]), x['query_point'])
        d['old'] = max(d['old'], abs(float(lab['old_conf'][n]) - x['old_conf'])) if n in sel else d['old']
    for n in sel:
        x = ref[n]
        d['conf'] = max(d['conf'], abs(float(lab['conf'][n]) - x['conf']))
        if n not in ex_l:
            assert tuple(int(t) for t in lab['new_idx'][n]) == x['new_idx'], (n, lab['new_idx'][n], x['new_idx'])
    print('%s: %d live rows (%d / %d excused by index), %d labelled; max |weight| %.2e |incl| %.2e |y| %.2e |conf| %.2e |old_conf| %.2e (bar %.0e); '
          'log_evidence rel %.2e (bar %.0e); gains %.2e entropies %.2e bits (bar %.0e)'
          % (cs, len(live), len(ex_q), len(ex_l), len(sel), d['weight'], d['incl'], d['y'], d['conf'], d['old'], P_BAR, d['le'], LE_BAR,
             d['gain'], d['ent'], BIT_BAR))
    assert max(d['weight'], d['incl'], d['y'], d['conf'], d['old']) <= P_BAR
    assert d['le'] <= LE_BAR
    assert max(d['gain'], d['ent']) <= BIT_BAR


# ---------------------------------------------------------------------------------------------------------------- 2. K = 1
@pytest.mark.parametrize('T,extra,h', [(2, 0, 0), (33, 5, 3), (70, 0, 6), (256, 0, 1)])
def test_one_pass_is_the_family_bit_for_bit(dev, T, extra, h):
    from hual_amd import lib
    c = Q.case(T)
    ld = T + extra
    s, e = pad_logits(dev, c['s'], ld, 1), pad_logits(dev, c['e'], ld, 2)
    vlen, tlen, aps = c['vlen'].numpy(), [T] * Q.N_ROWS, c['aps'][h]
    aset, keep = make_set(dev, vlen, tlen, aps, ld)
    old = np.tile(np.array([[0, 1]], dtype=np.int32), (Q.N_ROWS, 1))
    old_d = torch.from_numpy(old).to(dev)
    q1 = [o.cpu().numpy() for o in lib.al_query(aset, s, e, np.asarray(tlen))]
    m1 = [o.cpu().numpy() for o in lib.al_span_marginals(aset, s, e, np.asarray(tlen))]
    l1 = [o.cpu().numpy() for o in lib.al_mbr_label(aset, s, e, np.asarray(tlen), old_idx=old_d)]
    r = run_query(dev, s[None].contiguous(), e[None].contiguous(), vlen, tlen, aps)
    lab = run_label(dev, s[None].contiguous(), e[None].contiguous(), vlen, tlen, aps, old=old)
    bits = lambda a: np.ascontiguousarray(a).view(np.int32)
    for k, want in (('incl', q1[0]), ('gain', q1[1]), ('y_start', m1[0]), ('y_end', m1[1])):
        assert (bits(r[k])[:, :T] == bits(want)[:, :T]).all(), k
    assert (r['query_point'] == q1[2]).all() and (bits(r['query_gain']) == bits(q1[3])).all()
    assert (bits(r['expected_entropy']) == bits(q1[4])).all()
    assert (r['status'] == m1[2]).all() and (r['status'] == 1).all()
    assert (r['weight'] == 1.0).all()
    walk = np.abs(r['post_entropy'] - q1[4]).max()
    print('T=%d ld=%d answers=%d: the walk against the closed form: max |post_entropy - hual_al_query\'s| = %.3e bits (bar %.0e); max span_bald %.3e'
          % (T, ld, h, walk, BIT_BAR, r['span_bald'].max()))
    assert walk <= BIT_BAR and r['span_bald'].max() <= BIT_BAR
    assert (lab['new_idx'] == l1[0]).all()
    assert np.abs(lab['conf'] - l1[1]).max() <= P_BAR and np.abs(lab['old_conf'] - l1[2]).max() <= P_BAR


# ---------------------------------------------------------------------------------------------------------------- 3. edge rows
def test_edge_rows(dev):
    c = E.edge_case()
    ix, ref, N = c['names'], c['ref'], len(E.EDGE_ROWS)
    ps, pe = c['pass_s'].to(dev), c['pass_e'].to(dev)
    host_tlen = np.minimum(c['tlen'], 256)                            # the row of 300 frames is one the host was not told about
    from hual_amd import lib
    aset, keep = make_set(dev, c['vlen'], c['tlen'], c['aps'], c['ld'])
    out = lib.al_ensemble_query(aset, ps, pe, host_tlen)
    torch.cuda.synchronize()
    r = {k: o.cpu().numpy() for k, o in zip(Q_NAMES, out)}
    sel = list(range(N)) + [N + 5, -2, 0, 4]                          # foreign ids write nothing; repeated ids write the same values
    old_d = torch.from_numpy(c['old']).to(dev)
    lab = [o.cpu().numpy() for o in lib.al_ensemble_label(aset, ps, pe, host_tlen, sel=torch.tensor(sel, dtype=torch.int32, device=dev),
                                                          old_idx=old_d)]
    for name, n in ix.items():
        x = ref[n]
        if x['status'] == E.LIVE:
            assert r['status'][n] == 1, name
            v = len(x['incl'])
            assert np.abs(r['weight'][n] - x['weight']).max() <= P_BAR, name
            assert np.abs(r['incl'][n, :v] - x['incl']).max() <= P_BAR and np.abs(r['y_start'][n, :v] - x['y_start']).max() <= P_BAR, name
            assert abs(float(r['log_evidence'][n]) - x['log_evidence']) <= LE_BAR * max(1.0, abs(x['log_evidence'])), name
            assert np.abs(r['y_end'][n, :v] - x['y_end']).max() <= P_BAR and np.abs(r['gain'][n, :v] - x['gain']).max() <= BIT_BAR, name
            for k in ('post_entropy', 'expected_entropy', 'span_bald', 'query_gain'):
                assert abs(float(r[k][n]) - x[k]) <= BIT_BAR, (name, k)
            if x['query_gain'] - x['runner_gain'] >= 1e-5:
                assert int(r['query_point'][n]) == x['query_point'], name
            else:                                                     # (a collapsed posterior, one frame: every gain 0, the first frame)
                assert x['gain'].max() - x['gain'][int(r['query_point'][n])] <= 1e-5, name
            assert tuple(int(t) for t in lab[0][n]) == x['new_idx'] and abs(float(lab[1][n]) - x['conf']) <= P_BAR, name
            assert abs(float(lab[2][n]) - x['old_conf']) <= P_BAR, name
        else:
            assert r['status'][n] == 0 and r['query_point'][n] == -1, name
            for k in ('query_gain', 'post_entropy', 'expected_entropy', 'span_bald'):
                assert r[k][n] == -1.0, (name, k)
            assert (r['weight'][n] == 0).all() and (r['incl'][n] == 0).all() and (r['y_end'][n] == 0).all(), name
            le = float(r['log_evidence'][n])
            assert np.isnan(le) if x['status'] == E.POISONED else le == -np.inf, name
            assert tuple(lab[0][n]) == (-1, -1) and lab[1][n] == -1.0 and lab[2][n] == -1.0, name
    # what the rows are there for
    assert r['weight'][ix['one_pass_underflows'], 2] == 0.0 and r['status'][ix['one_pass_underflows']] == 1
    for n in (ix['collapsed'], ix['one_frame']):
        # (one span: the walk's single term is m log2 m with m = sum_k w_k, 1 up to its float64 rounding; the passes' closed form is
        # hual_al_query's, log2(Z_A) in float64 against the float32 log2f of the factors: 0 within the bar on entropies)
        assert r['query_gain'][n] == 0.0 and 0.0 <= r['post_entropy'][n] <= 1e-12 and 0.0 <= r['expected_entropy'][n] <= BIT_BAR
        assert r['span_bald'][n] <= 1e-12 and lab[1][n] == 1.0
    assert tuple(lab[0][ix['collapsed']]) == (5, 5)


# ---------------------------------------------------------------------------------------------------------------- 4. the launch
def test_second_launch_gives_equal_bits(dev):
    cs = E.CASES[2]
    r, lab, sel, (ps, pe, aps, logw) = got(dev, cs)
    c = E.case(*cs)
    vlen, tlen = c['vlen'].numpy(), [c['T']] * E.N_ROWS
    r2 = run_query(dev, ps, pe, vlen, tlen, aps, logw=logw)
    lab2 = run_label(dev, ps, pe, vlen, tlen, aps, logw=logw, old=c['old'], sel=sel)
    for k in Q_NAMES:
        assert (np.ascontiguousarray(r[k]).view(np.int32) == np.ascontiguousarray(r2[k]).view(np.int32)).all(), k
    for k in ('new_idx', 'conf', 'old_conf'):
        assert (np.ascontiguousarray(lab[k]).view(np.int32) == np.ascontiguousarray(lab2[k]).view(np.int32)).all(), k
    # a proper subset of the rows, in another order, beside a foreign id: the unselected rows keep their sentinel fill (run_label asserts
    # it) and the selected ones are the all-rows launch bit for bit
    part = [14, 0, 6, 2, E.N_ROWS + 3, 10, 4, 12, 8]
    lab3 = run_label(dev, ps, pe, vlen, tlen, aps, logw=logw, old=c['old'], sel=part)
    rows = [n for n in part if n < E.N_ROWS]
    assert len(rows) == E.N_ROWS // 2
    for k in ('new_idx', 'conf', 'old_conf'):
        assert (np.ascontiguousarray(lab[k][rows]).view(np.int32) == np.ascontiguousarray(lab3[k][rows]).view(np.int32)).all(), k
    lab4 = run_label(dev, ps, pe, vlen, tlen, aps, logw=logw, sel=[5])      # one row, the old span not scored
    assert (lab4['new_idx'][5] == lab['new_idx'][5]).all() and lab4['conf'][5] == lab['conf'][5] and lab4['old_conf'] is None
    # without the optional outputs the per-row values are the same
    r3 = run_query(dev, ps, pe, vlen, tlen, aps, logw=logw, frames=False, marginals=False)
    for k in ('weight', 'log_evidence', 'query_point', 'query_gain', 'post_entropy', 'expected_entropy', 'span_bald', 'status'):
        assert (np.ascontiguousarray(r[k]).view(np.int32) == np.ascontiguousarray(r3[k]).view(np.int32)).all(), k


def test_argument_errors_return_before_any_hip_call(dev):
    import ctypes
    from hual_amd import lib
    l = lib.load()
    N, ld, K = 4, 8, 2
    aset, keep = make_set(dev, [8] * N, [8] * N, [[] for _ in range(N)], ld)
    z = torch.zeros(K, N, ld, device=dev)
    o = [torch.full(s, FILL, device=dev) for s in ((N, K), (N,), (N, ld), (N, ld), (N,), (N,), (N, ld), (N, ld), (N,), (N,), (N,), (N,))]
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    torch.cuda.synchronize()

    def query(set_=aset, ps=z, pe=z, k=K, outs=o):
        return l.hual_al_ensemble_query(ctypes.byref(set_) if set_ is not None else None, p(ps), p(pe), k, None, *[p(t) for t in outs], None)

    def without(i):
        return [None if j == i else t for j, t in enumerate(o)]
    bad = [query(set_=None), query(ps=None), query(pe=None), query(k=0), query(k=17), query(outs=without(6)), query(outs=without(7))]
    bad += [query(outs=without(i)) for i in (0, 1, 4, 5, 8, 9, 10, 11)]
    bad += [query(set_=lib.hual_al_set(0, ld, *[lib._addr(t) for t in keep])), query(set_=lib.hual_al_set(N, 1, *[lib._addr(t) for t in keep])),
            query(set_=lib.hual_al_set(N, 1025, *[lib._addr(t) for t in keep]))]
    lo = [torch.full((N, 2), IFILL, dtype=torch.int32, device=dev), torch.full((N,), FILL, device=dev), torch.full((N,), FILL, device=dev)]
    old = torch.zeros(N, 2, dtype=torch.int32, device=dev)

    def label(ps=z, k=K, nsel=N, old_=old, outs=lo):
        return l.hual_al_ensemble_label(ctypes.byref(aset), p(ps), p(z), k, None, None, nsel, p(old_), *[p(t) for t in outs], None)
    bad += [label(ps=None), label(k=0), label(k=17), label(nsel=0), label(old_=None), label(outs=[lo[0], lo[1], None]), label(outs=[None, lo[1], lo[2]]),
            label(outs=[lo[0], None, lo[2]])]
    assert all(rc == -1 for rc in bad), bad                           # HUAL_ERR_INVALID
    torch.cuda.synchronize()
    assert all(bool((t == FILL).all()) for t in o) and bool((lo[0] == IFILL).all()) and bool((lo[1] == FILL).all())      # no stream work
    # the optional ones are optional
    assert query(outs=[None if j in (2, 3, 6, 7) else t for j, t in enumerate(o)]) == 0
    torch.cuda.synchronize()
    # the binding's own gate
    with pytest.raises(lib.HualError):
        lib.al_ensemble_query(aset, torch.zeros(17, N, ld, device=dev), torch.zeros(17, N, ld, device=dev), np.full(N, 8))
    with pytest.raises(lib.HualError):
        lib.al_ensemble_query(aset, z, z, np.full(N, 8), logw=torch.zeros(N, K, device=dev))


# ---------------------------------------------------------------------------------------------------------------- 5. plumbing
@functools.lru_cache(maxsize=None)
def _bank_after_inference(K, passes, info=False):
    """the set of test_gpu_al_query._round_set inferred with K stochastic passes into a McBank(passes=) under a known dropout stream:
    (S, bank, records, batches, (seed, base), rate)"""
    from hual_amd import al
    S = _round_set()
    N, ds, recs, model = S['N'], S['ds'], S['recs'], S['model']
    bank = al.McBank.for_dataset(ds, info=info, passes=passes)
    los = list(range(0, N, 16))

    def batches():
        for lo in los:
            sel = np.arange(lo, min(N, lo + 16))
            f = ds.assemble(sel, labels=False, min_chars=4)
            yield [recs[i] for i in sel], f['video'], f['video_seq_len'], f['word_ids'], f['char_ids']
    rng = (1234, 5000)
    prop, _ = al.infer_trainset(model, batches(), mc_dropout=0.5, mc_samples=K, bank=bank, batch_ids=range(len(los)), rng=rng)
    return S, bank, prop, batches, rng, 0.5


def test_bank_keeps_the_passes(dev):
    from hual_amd import al, lib
    K = 3
    S, bank, prop, batches, (seed, base), rate = _bank_after_inference(K, K)
    model = S['model']
    assert bank.K == K and tuple(bank.pass_s.shape) == (K, S['N'], bank.ld)
    lo = 0
    for i, (raw, video, lens, word_ids, char_ids) in enumerate(batches()):
        for k in range(1, K + 1):
            model.set_rng(seed, base + K * i + (k - 1))              # pass k of batch i (infer_trainset)
            o = model.forward(video, lens, word_ids, char_ids, drop_rate=rate)
            T = o['start_logits'].shape[1]
            assert torch.equal(bank.pass_s[k - 1, lo:lo + len(raw), :T], o['start_logits']), (i, k)
            assert torch.equal(bank.pass_e[k - 1, lo:lo + len(raw), :T], o['end_logits']), (i, k)
            assert bool((bank.pass_s[k - 1, lo:lo + len(raw), T:] == 0).all())
        lo += len(raw)
    # a pass beyond the planes is refused before anything is folded; a bank without planes is what it was
    stats = bank.stats.clone()
    with pytest.raises(lib.HualError):
        bank.fold(np.arange(2), torch.tensor([5, 5]), torch.zeros(2, 6, device=dev), torch.zeros(2, 6, device=dev), K + 1)
    assert torch.equal(stats, bank.stats)
    plain = al.McBank(S['N'], bank.ld)
    assert plain.pass_s is None and plain.pass_e is None and plain.Kmax == 0
    # the rows travel with their planes
    other = al.McBank(S['N'], bank.ld, passes=K)
    ids = np.array([3, 17, 30])
    other.import_rows(bank.export_rows(ids))
    assert torch.equal(other.pass_s[:, ids], bank.pass_s[:, ids]) and torch.equal(other.pass_e[:, ids], bank.pass_e[:, ids])
    assert bool((other.pass_s[:, 0] == 0).all())
    with pytest.raises(lib.HualError):
        plain.import_rows(bank.export_rows(ids))
    with pytest.raises(ValueError):
        al.McBank(4, 8, passes=17)


def test_update_labels_with_the_ensemble_posterior(dev):
    from hual_amd import al, lib
    K = 3
    S, bank, prop, _, _, _ = _bank_after_inference(K, K)
    N, coff = S['N'], al.get_coff('charades', 1)
    base = dict(bank=bank, return_debug=True)
    # the default and 'deterministic' are the parent's round: the same launches, keys and results
    kw = dict(observe_by='info_gain', renew_by='posterior', soft_out={})
    (new0, d0), k0 = _prof(lambda: al.update_labels(copy.deepcopy(S['data_old']), S['data_gt'], prop, coff, **base, **kw))
    soft0 = kw['soft_out']
    kw = dict(observe_by='info_gain', renew_by='posterior', soft_out={})
    (new1, d1), k1 = _prof(lambda: al.update_labels(copy.deepcopy(S['data_old']), S['data_gt'], prop, coff, **base, **kw, posterior='deterministic'))
    assert k0 == k1 and not any('ensemble' in k for k in k0), (k0, k1)
    assert new0 == new1 and sorted(d0) == sorted(d1)
    assert all(np.array_equal(d0[k], d1[k]) for k in d0 if k != 'updater')
    assert torch.equal(soft0['y1'], kw['soft_out']['y1']) and torch.equal(soft0['y2'], kw['soft_out']['y2'])
    # the ensemble round: the two new launches in place of the three, and their values are those of direct calls
    soft = {}
    (new2, d2), k2 = _prof(lambda: al.update_labels(copy.deepcopy(S['data_old']), S['data_gt'], prop, coff, **base, observe_by='info_gain',
                                                    renew_by='posterior', soft_out=soft, posterior='ensemble', rank_by='span_bald'))
    assert sum(v for k, v in k2.items() if 'al_ensemble_query' in k) == 2 and sum(v for k, v in k2.items() if 'al_ensemble_label' in k) == 1, k2
    assert not any(x in k for k in k2 for x in ('al_query_kernel', 'al_span_marginals', 'al_mbr_label')), k2
    up = d2['updater']
    vlen, tlen = up.vlen_h, up.tlen_h
    aps0 = [[] for _ in range(N)]
    aset0, keep0 = make_set(dev, vlen, tlen, aps0, bank.ld)
    q = [o.cpu().numpy() if o is not None else None for o in lib.al_ensemble_query(aset0, bank.pass_s[:K], bank.pass_e[:K], tlen)]
    for k, i in (('weight', 0), ('ens_log_evidence', 1), ('query_point', 4), ('query_gain', 5), ('post_entropy', 8), ('expected_entropy', 9),
                 ('span_bald', 10)):
        assert np.array_equal(d2[k], q[i]), k
    assert np.array_equal(d2['order'], np.argsort(-q[10], kind='stable'))
    sel = d2['order'][:(N + 1) // 2]
    assert np.array_equal(d2['observe_used'], np.where(q[5] > 0, q[4], d2['observe']))
    aps1 = [[(f, True) for f in r[4]['pos_idx']] + [(f, False) for f in r[4]['neg_idx']] for r in new2]
    aset1, keep1 = make_set(dev, vlen, tlen, aps1, bank.ld)
    m = lib.al_ensemble_query(aset1, bank.pass_s[:K], bank.pass_e[:K], tlen, frames=False)
    assert torch.equal(soft['y1'], m[6]) and torch.equal(soft['y2'], m[7]) and np.array_equal(soft['live'], m[11].cpu().numpy() == 1)
    old_d = torch.from_numpy(np.ascontiguousarray(d2['old_idx'], dtype=np.int32)).to(dev)
    lab = lib.al_ensemble_label(aset1, bank.pass_s[:K], bank.pass_e[:K], tlen, sel=torch.from_numpy(sel.astype(np.int32)).to(dev), old_idx=old_d)
    assert np.array_equal(d2['label_conf'], lab[1].cpu().numpy()) and np.array_equal(d2['old_conf'], lab[2].cpu().numpy())
    assert np.array_equal(d2['new_idx'][sel], lab[0].cpu().numpy()[sel]) and d2['renewed_by_posterior'][sel].all()
    assert (q[10] > 0).any() and (q[10] >= 0).all()                   # the passes disagree somewhere: the score is not idle
    # under noise: one tilt per plane, then the same two launches
    (new3, d3), k3 = _prof(lambda: al.update_labels(copy.deepcopy(new2), S['data_gt'], prop, al.get_coff('charades', 2), **base,
                                                    observe_by='info_gain', renew_by='posterior', posterior='ensemble', answer_noise=0.1))
    assert sum(v for k, v in k3.items() if 'al_noisy_tilt' in k) == 2 * K and 'log_evidence' not in d3 and sum(v for k, v in k3.items() if 'al_ensemble' in k) == 2, k3
    st, et, lev = torch.zeros_like(bank.pass_s[:K]), torch.zeros_like(bank.pass_s[:K]), torch.empty(K, N, device=dev)
    for k in range(K):
        lib.al_noisy_tilt(aset1, bank.pass_s[k], bank.pass_e[k], tlen, 0.1, out=(st[k], et[k], lev[k]))
    qn = lib.al_ensemble_query(aset0, st, et, tlen, logw=lev)
    assert np.array_equal(d3['query_point'], qn[4].cpu().numpy()) and np.array_equal(d3['weight'], qn[0].cpu().numpy())
    # what has no ensemble form is refused, with a message, before anything is touched
    data = copy.deepcopy(S['data_old'])
    for bad in (dict(acquire_by='label_gain'), dict(observe_by='info_gain', questions_per_clip=2), dict(observe_by='info_gain', calibrate='evidence'),
                dict(), dict(observe_by='info_gain', bank=al.McBank(N, bank.ld))):
        with pytest.raises(ValueError):
            al.update_labels(data, S['data_gt'], prop, coff, **dict(dict(bank=bank, posterior='ensemble'), **bad))
    with pytest.raises(ValueError):
        al.update_labels(data, S['data_gt'], prop, coff, bank=bank, rank_by='span_bald')
    assert data == S['data_old']


def test_set_ensemble_on_and_off(dev):
    from hual_amd import al, lib
    K = 3
    S, bank, prop, _, _, _ = _bank_after_inference(K, K)
    N = S['N']
    vlen = [p['v_len'] for p in prop]
    aps = [[(2, True)] if n % 2 else [] for n in range(N)]
    names = ('incl', 'gain', 'query_point', 'query_gain', 'post_entropy', 'agree')

    def read(up):
        assert up.query() is None
        up.span_marginals()
        lab = up.mbr_label(np.arange(N), np.zeros((N, 2), dtype=np.int64))
        return [getattr(up, k).clone() for k in names] + [up.y_start.clone(), up.y_end.clone()] + [torch.from_numpy(x) for x in lab]
    plain = al.LabelUpdater.from_bank(bank, vlen, aps)
    (want), k_plain = _prof(lambda: read(plain))
    up = al.LabelUpdater.from_bank(bank, vlen, aps, ensemble=True)
    ens = up.query()
    assert sorted(ens) == ['expected_entropy', 'log_evidence', 'span_bald', 'weight'] and up.agree is None
    for call in (lambda: up.label_gain(), lambda: up.session(np.zeros((N, 2), dtype=np.int64), 2), lambda: up.calibrate(),
                 lambda: up.evidence_grid([1.0], [0.1])):
        with pytest.raises(lib.HualError):
            call()
    # a temperature scales the planes as it scales s0 / e0
    up.set_temperature(2.0)
    up.query()
    inv = float(np.float32(0.5))
    q = lib.al_ensemble_query(up.set, (bank.pass_s[:K] * inv).contiguous(), (bank.pass_e[:K] * inv).contiguous(), up.tlen_h)
    assert torch.equal(up.incl, q[2]) and torch.equal(up.span_bald, q[10])
    up.set_temperature(None)
    up.set_ensemble(None, None)
    got_, k_off = _prof(lambda: read(up))
    assert k_off == k_plain and not any('ensemble' in k for k in k_off), (k_off, k_plain)
    assert all(torch.equal(a, b) for a, b in zip(want, got_))


def test_run_round_with_the_ensemble_posterior(dev):
    """two rounds: the first, under the default posterior, fills a bank that keeps its passes; the second reads them as the ensemble"""
    from hual_amd import al
    K = 3
    S = _round_set()
    model, ds, N = S['model'], S['ds'], S['N']
    kw = dict(epochs=1, batch_size=16, lr=1e-3, drop_rate=0.2, mc_samples=K)
    bank = al.McBank.for_dataset(ds, passes=K)
    data = copy.deepcopy(S['data_old'])
    for b in (None, bank, al.McBank.for_dataset(ds)):               # no bank, a bank nothing was folded into, a bank without planes
        with pytest.raises(ValueError):
            al.run_round(model, ds, data, S['data_gt'], S['prop'], 'charades', 1, bank=b, posterior='ensemble', observe_by='info_gain', **kw)
    with pytest.raises(ValueError):
        al.run_round(model, ds, data, S['data_gt'], S['prop'], 'charades', 1, bank=bank, rank_by='span_bald', **kw)
    assert data == S['data_old'] and bank.K == 0
    new1, prop1, m1 = al.run_round(model, ds, data, S['data_gt'], S['prop'], 'charades', 1, bank=bank, **kw)
    assert m1['mc_bank'] is bank and bank.K == K and bool((bank.pass_s != 0).any())
    # what the second round has to ask and whom: the launch itself on the bank's planes and the first round's answers
    aps = [[(f, True) for f in r[4]['pos_idx']] + [(f, False) for f in r[4]['neg_idx']] for r in new1]
    up = al.LabelUpdater.from_bank(bank, [p['v_len'] for p in prop1], aps, ensemble=True)
    up.query(frames=False)
    bald, qp, qg = up.span_bald.cpu().numpy(), up.query_point.cpu().numpy(), up.query_gain.cpu().numpy()
    planes = bank.pass_s.clone()
    new2, prop2, m2 = al.run_round(model, ds, copy.deepcopy(new1), S['data_gt'], prop1, 'charades', 2, bank=bank, posterior='ensemble',
                                   rank_by='span_bald', observe_by='info_gain', renew_by='posterior', **kw)
    assert len(prop2) == N and m2['train_steps'] == 3 and 0.0 <= m2['miou'] <= 100.0
    sel = set(int(i) for i in np.argsort(-bald, kind='stable')[:(N + 1) // 2])
    ans = _answers(new2, new1)
    assert set(i for i in range(N) if ans[i]) == sel and all(len(ans[i]) == 1 for i in sel)
    asked = [i for i in sel if qg[i] > 0]
    assert len(asked) > N // 4 and all(ans[i][0][0] == int(qp[i]) for i in asked)
    assert bank.K == K and not torch.equal(planes, bank.pass_s)      # refilled by the round's own inference, for the next round
