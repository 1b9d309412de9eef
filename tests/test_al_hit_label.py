"""CPU: hual_al_hit_label (label reliability: the hit probability of pseudo-labels under the answered-point posterior) is declared,
exported and refuses bad arguments before any HIP call, as does its binding; al.frame_hits by hand; al.check_round on the new values
rank_by='label_miss', renew_by='hit_prob' and hit_iou; and the float64 reference the GPU tests compare against (tests/al_hit_ref.py)
has the properties that define the quantity, on the cases the GPU tests use (al_query_ref.case)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import al_hit_ref as HL
import al_query_ref as Q
import span_hit_ref as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THR3 = HL.THR3


# ---------------------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize('T', [2, 33])
def test_reference_without_answers_is_the_bayes_reference(T):
    """no active point: A is the whole triangle, Z_A = Z, and the quantity is hual_span_hit_prob's"""
    c = Q.case(T)
    rows = H.bayes_ref(c['s'], c['e'], c['vlen'], THR3)
    mine = HL.full_best(T, 0)
    for n in range(Q.N_ROWS):
        st, b, r = HL.states(T, 0)[n], mine[n], rows[n]
        assert st['status'] == HL.LIVE and (st['ii'] == r['ii']).all() and (st['jj'] == r['jj']).all()
        assert np.abs(b['prob'] - r['prob']).max() <= 1e-15
        assert (b['best'] == r['best']).all()


@pytest.mark.parametrize('h', Q.HISTORIES)
def test_reference_properties_under_answers(h):
    T, thr = 33, [(1, 1024)] + THR3 + [(1, 1)]
    beats = 0
    for n, st in enumerate(HL.states(T, h)):
        assert st['status'] == HL.LIVE                                # a truthful annotator never contradicts itself
        b = HL.best_ref(st, thr)
        assert (b['prob'] >= 0).all() and (b['prob'] <= 1).all()
        assert (np.diff(b['prob'], axis=1) <= 1e-15).all()            # a hit at a higher threshold is a hit at every lower one
        q = int(np.argmax(st['w']))                                   # at 1 / 1 a span hits itself only: the heaviest member, w / Z_A
        assert b['best'][4] == q and abs(b['top'][4] - st['w'][q] / st['ZA']) <= 1e-15
        assert (np.diff(b['top']) <= 1e-15).all() and (b['gap'] >= 0).all()
        # a span outside A can be a good label: it is scored against the truths in A all the same
        out = HL.random_spans(st, 64, 100 * h + n, inside=False)
        out = out[[not HL.is_member(st, a, z) for a, z in out]]
        if len(out):
            beats += int((HL.cand_prob(st, out, thr)[:, 1] > 0).any())
    if h:
        assert beats > 0


def test_reference_collapsed_posterior_and_dead_rows():
    c = Q.case(33)
    ps, pe = c['ps'][0], c['pe'][0]
    st = HL.state(ps, pe, 33, [(11, False), (12, True), (13, False)])
    assert st['status'] == HL.LIVE and list(zip(st['ii'], st['jj'])) == [(12, 12)]
    b = HL.best_ref(st, THR3)
    assert (b['top'] == 1.0).all() and (b['best'] == 0).all() and np.isinf(b['gap']).all()
    got = HL.cand_prob(st, [(12, 12), (11, 13), (10, 14), (2, 5), (-1, 4), (5, 3), (4, 33)], THR3)
    assert (got[0] == 1.0).all() and list(got[1]) == [1.0, 0.0, 0.0] and (got[2] == 0.0).all() and (got[3] == 0.0).all()      # 1/3, 1/5: outside A, scored
    assert (got[4:] == -1.0).all()
    assert HL.state(ps, pe, 33, [(5, True), (9, True), (7, False)])['status'] == HL.CONTRADICTORY
    assert HL.state(ps, pe, 0, [])['status'] == HL.POISONED and HL.state(ps, pe, 33, [], nan_logit=True)['status'] == HL.POISONED
    assert (HL.cand_prob(HL.state(ps, pe, 0, []), [(0, 0)], THR3) == -1.0).all() and HL.best_ref(HL.state(ps, pe, 0, []), THR3) is None


# ---------------------------------------------------------------------------------------------------------------- frame_hits
def test_frame_hits_by_hand():
    from hual_amd import al
    a = [[0, 9]] * 5 + [[3, 3]] * 3
    b = [[0, 9], [0, 4], [2, 6], [4, 9], [5, 9], [0, 2], [3, 3], [4, 9]]
    # [0, 9] (10 frames) against IoU 1, 0.5, 0.5, 0.6, 0.5; [3, 3] against no overlap, itself, no overlap
    got = al.frame_hits(a, b, [(1, 2), (3, 5), (7, 10), (1, 1024)])
    assert got.dtype == bool and got.shape == (8, 4)
    assert got.tolist() == [[True, True, True, True], [True, False, False, True], [True, False, False, True], [True, True, False, True],
                            [True, False, False, True], [False] * 4, [True] * 4, [False] * 4]
    assert (al.frame_hits(b, a, (0.5, 0.6, 0.7, 1 / 1024)) == got).all()      # symmetric, and floats through lib.hit_thresholds
    assert al.frame_hits([[-1, -1], [5, 3], [2, 4]], [[2, 4], [2, 4], [-1, 4]], (0.5,)).tolist() == [[False], [False], [False]]
    assert al.frame_hits(np.zeros((0, 2)), np.zeros((0, 2)), (0.3, 0.5)).shape == (0, 2)
    with pytest.raises(ValueError, match='same number'):
        al.frame_hits([[0, 1]], [[0, 1], [0, 1]], (0.5,))


# ---------------------------------------------------------------------------------------------------------------- the entry point
def test_symbol_is_declared_and_exported_at_abi_9():
    from hual_amd import build, lib
    build.build()
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'hual_seqpan.h')).read(), flags=re.S)
    assert re.search(r'\bint hual_al_hit_label\s*\(', src)
    assert hasattr(ctypes.CDLL(lib.LIB_PATH), 'hual_al_hit_label'), 'missing export hual_al_hit_label'
    assert lib.load().hual_abi_version() == lib.ABI_VERSION == 9          # a new symbol, the ABI version stays
    assert callable(lib.al_hit_label)


def test_entry_point_refuses_bad_arguments_without_a_gpu():
    """every bad argument returns before any HIP call (the device pointers below are never dereferenced; the thresholds are host memory)"""
    from hual_amd import lib
    l = lib.load()
    buf = ctypes.create_string_buffer(64)
    a = ctypes.addressof(buf)
    p = ctypes.c_void_p(a)
    SET = ('vlen', 'tlen', 'ap_off', 'ap_idx', 'ap_pos')

    def aset(N=4, ld=64, **null):
        f = {k: a for k in SET}
        f.update(null)
        return ctypes.byref(lib.hual_al_set(N, ld, *[f[k] for k in SET]))

    def thr_of(pairs):
        return (ctypes.c_int32 * (2 * len(pairs)))(*[x for nd in pairs for x in nd])

    def call(s=None, s0=p, e0=p, sel=p, nsel=2, thr=thr_of(THR3), M=3, cand=p, k=2, hit=p, best=(p, p), _null_set=False):
        return l.hual_al_hit_label(None if _null_set else (s or aset()), s0, e0, sel, nsel, thr, M, cand, k, hit, *best, None)
    for kw, msg in ((dict(_null_set=True), b'null pointer'), (dict(thr=None), b'null pointer'), (dict(s0=None), b'null input'),
                    (dict(e0=None), b'null input'), (dict(s=aset(vlen=None)), b'null input'), (dict(s=aset(tlen=None)), b'null input'),
                    (dict(s=aset(ap_off=None)), b'null input'), (dict(s=aset(ap_idx=None)), b'null input'),
                    (dict(s=aset(ap_pos=None)), b'null input'), (dict(cand=None), b'null pointer'), (dict(hit=None), b'null pointer'),
                    (dict(best=(p, None)), b'together'), (dict(best=(None, p)), b'together'),
                    (dict(k=0, cand=None, hit=None, best=(None, None)), b'nothing to do'),
                    (dict(nsel=0), b'nsel >= 1'), (dict(nsel=-3), b'nsel >= 1'), (dict(sel=None, nsel=0), b'nsel >= 1'),
                    (dict(s=aset(N=0)), b'N > 0'), (dict(s=aset(ld=1)), b'2 <= ld'), (dict(s=aset(ld=1025)), b'ld <= 1024'),
                    (dict(k=-1), b'k <= 16'), (dict(k=17), b'k <= 16'), (dict(M=0), b'M <= 4'), (dict(M=5), b'M <= 4'),
                    (dict(thr=thr_of([(3, 10), (0, 2), (7, 10)])), b'num <= den'), (dict(thr=thr_of([(3, 10), (3, 2), (7, 10)])), b'num <= den'),
                    (dict(thr=thr_of([(3, 10), (1, 2), (1, 1025)])), b'num <= den'), (dict(thr=thr_of([(-1, 10), (1, 2), (7, 10)])), b'num <= den')):
        rc = call(**kw)
        assert rc == -1 and msg in l.hual_last_error() and b'al_hit_label' in l.hual_last_error(), (kw, msg, rc, l.hual_last_error())
    with pytest.raises(lib.HualError, match='M <= 4'):
        lib.check(call(M=5))


def test_binding_refuses_bad_arguments_without_a_gpu():
    """every argument fault is a HualError before the library is called: the set below holds pointers nothing may follow"""
    from hual_amd import lib
    N, ld = 3, 8
    aset = lib.hual_al_set(N, ld, 8, 8, 8, 8, 8)
    s = torch.zeros(N, ld)
    tl = np.full(N, ld)
    cand = torch.zeros(N, 2, 2, dtype=torch.int32)
    sel = torch.zeros(2, dtype=torch.int32)
    good_out = (torch.zeros(N, 2, 3), (torch.zeros(N, 3, 2, dtype=torch.int32), torch.zeros(N, 3)))
    for args, kw, msg in (((aset, s.double(), s, tl), {}, 's0 / e0 must be'), ((aset, s, s[:, :4], tl), {}, 's0 / e0 must be'),
                          ((aset, s, s, tl[:2]), {}, 'N = 3 row lengths'), ((aset, s, s, np.full(N, 300)), {}, '256'),
                          ((aset, s, s, tl), dict(thresholds=(0.3001234567,)), 'denominator'), ((aset, s, s, tl), dict(thresholds=()), '1 to 4'),
                          ((aset, s, s, tl), dict(thresholds=(0.1, 0.3, 0.5, 0.7, 0.9)), '1 to 4'),
                          ((aset, s, s, tl), dict(sel=sel.long()), 'sel must be'), ((aset, s, s, tl), dict(sel=sel[:0]), 'sel must be'),
                          ((aset, s, s, tl), dict(cand=cand.long()), 'cand must be'), ((aset, s, s, tl), dict(cand=cand[:2]), 'cand must be'),
                          ((aset, s, s, tl), dict(cand=torch.zeros(N, 17, 2, dtype=torch.int32)), 'cand must be'),
                          ((aset, s, s, tl), dict(cand=torch.zeros(N, 0, 2, dtype=torch.int32)), 'cand must be'),
                          ((aset, s, s, tl), dict(cand=torch.zeros(N, 2, 3, dtype=torch.int32)), 'cand must be'),
                          ((aset, s, s, tl), dict(best=False), 'nothing to do'),
                          ((aset, s, s, tl), dict(cand=cand, out=(None, good_out[1])), 'out is'),
                          ((aset, s, s, tl), dict(out=good_out), 'out is'),
                          ((aset, s, s, tl), dict(cand=cand, best=False, out=good_out), 'out is'),
                          ((aset, s, s, tl), dict(cand=cand, out=(good_out[0], good_out[1][:1])), 'out is'),
                          ((aset, s, s, tl), dict(cand=cand, out=(torch.zeros(N, 2, 2), good_out[1])), 'out tensors'),
                          ((aset, s, s, tl), dict(cand=cand, out=(good_out[0], (good_out[1][0].long(), good_out[1][1]))), 'out tensors'),
                          ((aset, s, s, tl), dict(cand=cand, out=(good_out[0], (good_out[1][0], torch.zeros(N, 4)))), 'out tensors')):
        with pytest.raises(lib.HualError, match=msg):
            lib.al_hit_label(*args, **kw)


# ---------------------------------------------------------------------------------------------------------------- the round
class _Bank:
    K = Kmax = 3
    pass_s = object()


def test_check_round_on_the_new_values():
    from hual_amd import al
    base = al.check_round()
    assert base.hit_iou == 0.7 and base[:-1] == ('deterministic', 'uncert_video', 'uncert_frame', 'heuristic', None, 1, None, None, None,
                                                  None, None, False, 1)
    assert al.RoundPolicy._fields[-1] == 'hit_iou' and not base.reads_posterior
    for iou in al.HIT_IOUS:
        assert al.check_round(hit_iou=iou)[:-1] == base[:-1]          # the defaults give the policy they gave
    # both new values read the posterior: noise, temperature and calibrate are accepted with them alone
    for kw in (dict(rank_by='label_miss'), dict(renew_by='hit_prob')):
        for extra in ({}, dict(answer_noise=0.1), dict(temperature=2.0), dict(calibrate='evidence'), dict(hit_iou=0.3)):
            pol = al.check_round(**kw, **extra)
            assert pol.reads_posterior and pol.hit_iou == extra.get('hit_iou', 0.7)
            assert (pol.rank_by, pol.renew_by) == (kw.get('rank_by', 'uncert_video'), kw.get('renew_by', 'heuristic'))
    assert al.check_round(rank_by='label_miss', renew_by='hit_prob', observe_by='info_gain', questions_per_clip=3).Q == 3
    for extra in (dict(answer_noise=0.1), dict(temperature=2.0), dict(calibrate='evidence')):      # as before: idle without a reader
        with pytest.raises(ValueError, match='changes the span posterior'):
            al.check_round(**extra)
    for kw in (dict(rank_by='label_miss'), dict(renew_by='hit_prob'), dict(rank_by='label_miss', renew_by='posterior')):
        with pytest.raises(ValueError, match='no ensemble form'):
            al.check_round(posterior='ensemble', bank=_Bank(), observe_by='info_gain', **kw)
    with pytest.raises(ValueError, match='acquire_by'):
        al.check_round(acquire_by='label_gain', rank_by='label_miss')
    assert al.check_round(acquire_by='label_gain', renew_by='hit_prob').renew_by == 'hit_prob'
    for bad in (0.4, 1.0, 0, None, True, 'high', (0.7,)):
        with pytest.raises(ValueError, match='hit_iou'):
            al.check_round(hit_iou=bad)
    with pytest.raises(ValueError, match='rank_by'):
        al.check_round(rank_by='hit_prob')
    with pytest.raises(ValueError, match='renew_by'):
        al.check_round(renew_by='label_miss')
    assert al.RANK_BY_HIT == ('label_miss',) and al.RENEW_BY_HIT == ('hit_prob',)


def test_update_labels_refuses_before_it_touches_anything():
    import copy
    from hual_amd import al
    data_old = [['v0', 10.0, [1.0, 2.0], 'a b'], ['v1', 12.0, [3.0, 4.0], 'c d']]
    keep = copy.deepcopy(data_old)
    prop, coff = [{'vid': 'v0'}, {'vid': 'v1'}], al.get_coff('charades', 1)
    for kw, msg in ((dict(hit_iou=0.6), 'hit_iou'), (dict(rank_by='label_miss', acquire_by='label_gain'), 'acquire_by'),
                    (dict(renew_by='hit_prob', posterior='ensemble', bank=_Bank()), 'no ensemble form')):
        with pytest.raises(ValueError, match=msg):
            al.update_labels(data_old, copy.deepcopy(data_old), prop, coff, **kw)
        assert data_old == keep
