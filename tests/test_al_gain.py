"""CPU: hual_al_label_gain (per frame, the tIoU the minimum-Bayes-risk pseudo-label is expected to gain from the frame's answer) is
declared, exported and refuses bad arguments before any HIP call; al.update_labels refuses an unknown acquire_by, and acquire_by beside
another ranking or question, before it touches anything; and the float64 reference the GPU tests compare against
(tests/al_gain_ref.py) has the properties that define the quantity - on the very cases the GPU tests use (al_query_ref.case: T in
{2, 33} with 16 rows, T = 70 with rows 0-3, after 0, 1, 3 and 6 truthful answers) - together with the number of states whose best
frame stands far enough above the runner-up for the GPU tests to compare the index itself."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest

import al_gain_ref as G
import al_query_ref as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# states with a best gain above 1e-9 whose margin over the second-best frame exceeds 1e-5 (ten times the GPU tests' 1e-6 bar on a gain: a
# kernel within the bar of every gain cannot prefer another frame), per history (0, 1, 3, 6) - measured with the brute force; the
# smallest margins among the others are 7e-7 (T = 33) and exact ties (T = 2)
BY_INDEX = {2: (6, 4, 0, 0), 33: (15, 14, 13, 13), 70: (4, 4, 4, 3)}


def test_symbol_is_declared_and_exported():
    from hual_amd import build, lib
    build.build()
    src = open(os.path.join(ROOT, 'include', 'hual_seqpan.h')).read()
    assert re.search(r'\bint hual_al_label_gain\s*\(', src)
    assert hasattr(ctypes.CDLL(lib.LIB_PATH), 'hual_al_label_gain'), 'missing export hual_al_label_gain'
    assert lib.load().hual_abi_version() == lib.ABI_VERSION == 9          # a new symbol, the ABI version stays
    assert callable(lib.al_label_gain)


def test_gain_refuses_bad_arguments_without_a_gpu():
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

    def call(s=None, s0=p, e0=p, sel=p, nsel=2, cand=p, M=4, gain=p, point=p, ask=p, value=p, _null_set=False):
        return l.hual_al_label_gain(None if _null_set else (s or aset()), s0, e0, sel, nsel, cand, M, gain, point, ask, value, None)
    for kw, msg in ((dict(_null_set=True), b'null set'), (dict(s0=None), b'null input'), (dict(e0=None), b'null input'),
                    (dict(s=aset(vlen=None)), b'null input'), (dict(s=aset(tlen=None)), b'null input'),
                    (dict(s=aset(ap_off=None)), b'null input'), (dict(s=aset(ap_idx=None)), b'null input'),
                    (dict(s=aset(ap_pos=None)), b'null input'),
                    (dict(point=None), b'null output'), (dict(ask=None), b'null output'), (dict(value=None), b'null output'),
                    (dict(nsel=0), b'nsel >= 1'), (dict(nsel=-3), b'nsel >= 1'), (dict(sel=None, nsel=0), b'nsel >= 1'),
                    (dict(s=aset(N=0)), b'N > 0'), (dict(s=aset(ld=1)), b'2 <= ld'), (dict(s=aset(ld=1025)), b'ld <= 1024'),
                    (dict(M=0), b'1 <= M <= 256'), (dict(M=257), b'1 <= M <= 256'), (dict(M=-1), b'1 <= M <= 256')):
        rc = call(**kw)
        assert rc == -1 and msg in l.hual_last_error(), (kw, msg, rc, l.hual_last_error())      # HUAL_ERR_INVALID
    with pytest.raises(lib.HualError):
        lib.check(rc)


def test_update_labels_refuses_a_bad_acquire_by():
    from hual_amd import al
    data_old = [['v0', 10.0, [1.0, 2.0], 'a b'], ['v1', 12.0, [3.0, 4.0], 'c d']]
    keep = copy.deepcopy(data_old)
    prop, coff = [{'vid': 'v0'}, {'vid': 'v1'}], al.get_coff('charades', 1)
    for kw in (dict(acquire_by='bogus'), dict(acquire_by='label_gain', rank_by='span_risk'),
               dict(acquire_by='label_gain', observe_by='info_gain')):
        with pytest.raises(ValueError, match='acquire_by'):
            al.update_labels(data_old, copy.deepcopy(data_old), prop, coff, **kw)
        assert data_old == keep
    assert al.ACQUIRE_BY == (None, 'label_gain')
    assert al.OBSERVE_BY == ('uncert_frame', 'info_gain') and al.RANK_BY == ('uncert_video', 'span_risk')      # not extended


# ---------------------------------------------------------------------------------------------------------------------
# the reference's own properties
@pytest.mark.parametrize('T', sorted(G.ROWS))
def test_reference_gain_properties(T):
    c = G.case(T)
    raw_min, gained, elsewhere, collapsed = np.inf, 0, 0, 0
    for h in Q.HISTORIES:
        for n in G.ROWS[T]:
            r, q, v = c['gref'][h][n], c['ref'][h][n], int(c['v'][n])
            assert r['status'] == G.LIVE and r['frames'] == list(range(v)), (T, h, n)      # a truthful annotator never contradicts itself
            st = r['st']
            assert abs(r['value'] - c['lref'][h][n]['conf']) <= 1e-14   # V0 is the conf of the minimum-Bayes-risk label
            assert np.abs(r['zp'] + r['zn'] - st['ZA']).max() <= 1e-12 * st['ZA']
            assert np.abs(r['zp'] / st['ZA'] - q['incl']).max() <= 1e-12
            fixed = (q['incl'] == 0) | (q['incl'] == 1)
            assert (r['gain'][fixed] == 0).all() and (r['raw'][fixed] == 0).all()      # a determined answer moves no label
            assert r['gain'].min() >= 0.0 and r['gain'].max() <= 1.0 - r['value'] + 1e-12
            raw_min = min(raw_min, float(r['raw'].min()))
            if len(st['ai']) == 1:                                      # collapsed: nothing to gain, the first frame
                assert (r['gain'] == 0).all() and r['ask_point'] == 0 and r['ask_gain'] == 0.0
                collapsed += 1
            if r['ask_gain'] > 0:
                gained += 1
                elsewhere += r['ask_point'] != q['query_point']
    print('T=%d: smallest gain before the clamp at 0: %.3e; %d states with a gain to be had, the frame of maximal gain is another than the '
          'frame of most information in %d of them; %d collapsed states' % (T, raw_min, gained, elsewhere, collapsed))
    assert raw_min >= -1e-12                                            # no state of these cases needs the clamp
    assert collapsed > 0 or T == 70
    assert elsewhere > 0                                                # another question than hual_al_query's


def test_reference_edge_rules():
    c = Q.case(33)
    ps, pe = c['ps'][0], c['pe'][0]
    for v, aps in ((33, [(5, True), (9, True), (7, False)]), (3, [(0, False), (1, False), (2, False)])):      # a negative in the hull | no gap
        r = G.gain_ref(ps, pe, v, aps)
        assert r['status'] == G.CONTRADICTORY and r['ask_point'] == -1 and r['ask_gain'] == -1.0 and r['value'] == -1.0 and (r['gain'] == 0).all()
    assert G.gain_ref(ps, pe, 0, [])['status'] == G.POISONED and G.gain_ref(ps, pe, 33, [], nan_logit=True)['ask_point'] == -1
    one = G.gain_ref(ps, pe, 20, [(3, False), (4, True), (5, False)])   # one consistent span: collapsed, not an error
    assert one['status'] == G.LIVE and (one['gain'] == 0).all() and one['ask_point'] == 0 and one['ask_gain'] == 0.0 and one['value'] == 1.0
    # a candidate list: the same numbers at the listed frames, 0 elsewhere, the first listed frame of maximal gain
    full = G.gain_ref(ps, pe, 20, [(10, True)])
    part = G.gain_ref(ps, pe, 20, [(10, True)], frames=[14, -1, 3, 25, 12])
    assert part['frames'] == [14, 3, 12] and part['value'] == full['value']
    assert all(part['gain'][t] == full['gain'][t] for t in (14, 3, 12)) and part['gain'].sum() == full['gain'][[14, 3, 12]].sum()
    assert part['ask_point'] == max((14, 3, 12), key=lambda t: full['gain'][t]) and full['ask_gain'] >= part['ask_gain'] > 0
    none = G.gain_ref(ps, pe, 20, [(10, True)], frames=[-1, 20])        # no listed frame inside the clip
    assert none['ask_point'] == -1 and none['ask_gain'] == 0.0 and (none['gain'] == 0).all() and none['value'] == full['value']
    # the chunked walk of a large A is the matrix form
    st = full['st']
    holds = (st['ai'] <= 7) & (7 <= st['aj'])
    for m in (holds, ~holds):
        a, b = G.branch_value(st, m), G.branch_value(st, m, G.pair_iou(st['ai'], st['aj'], st['ai'], st['aj']))
        assert a[0] == b[0] and abs(a[1] - b[1]) <= 1e-15


# ---------------------------------------------------------------------------------------------------------------------
# what the GPU tests' comparison of indices rests on
@pytest.mark.parametrize('T', sorted(G.ROWS))
def test_reference_states_compared_by_index(T):
    c = G.case(T)
    counts = tuple(sum(G.by_index(c['gref'][h][n]) for n in G.ROWS[T]) for h in Q.HISTORIES)
    near = [c['gref'][h][n]['margin'] for h in Q.HISTORIES for n in G.ROWS[T]
            if c['gref'][h][n]['ask_gain'] > 1e-9 and not G.by_index(c['gref'][h][n])]
    print('T=%d: states compared by index per history %s of %d; margins of the states with a gain that are not: %s'
          % (T, counts, len(G.ROWS[T]), ['%.2e' % m for m in near]))
    assert counts == BY_INDEX[T]
