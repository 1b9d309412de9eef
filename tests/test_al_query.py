"""CPU: hual_al_query (the frame of most expected information gain under the span posterior) is declared, exported and refuses bad
arguments before any HIP call; al.update_labels refuses an unknown observe_by before it touches anything; and the float64 reference
the GPU tests compare against (tests/al_query_ref.py) has the properties that define the quantity - on the very cases the GPU tests
use (al_query_ref.case: N(0, 2) logits clipped to |x| <= 8, T in {2, 33, 70, 256}, 16 rows, half of them shorter than T, after 0, 1, 3
and 6 truthful answers at the reference's own query frame)."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest

import al_query_ref as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_declared_and_exported():
    from hual_amd import build, lib
    build.build()
    src = open(os.path.join(ROOT, 'include', 'hual_seqpan.h')).read()
    assert re.search(r'\bint hual_al_query\s*\(', src)
    assert hasattr(ctypes.CDLL(lib.LIB_PATH), 'hual_al_query'), 'missing export hual_al_query'
    assert lib.load().hual_abi_version() == lib.ABI_VERSION == 9          # a new symbol, the ABI version stays


def test_query_refuses_bad_arguments_without_a_gpu():
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

    def call(s=None, s0=p, e0=p, point=p, qgain=p, ent=p, agree=p, _null_set=False):
        return l.hual_al_query(None if _null_set else (s or aset()), s0, e0, None, None, point, qgain, ent, agree, None)
    for kw, msg in ((dict(_null_set=True), b'null set'), (dict(s0=None), b'null input'), (dict(e0=None), b'null input'),
                    (dict(s=aset(vlen=None)), b'null input'), (dict(s=aset(tlen=None)), b'null input'),
                    (dict(s=aset(ap_off=None)), b'null input'), (dict(s=aset(ap_idx=None)), b'null input'),
                    (dict(s=aset(ap_pos=None)), b'null input'),
                    (dict(point=None), b'null output'), (dict(qgain=None), b'null output'), (dict(ent=None), b'null output'),
                    (dict(agree=None), b'null output'),
                    (dict(s=aset(N=0)), b'N > 0'), (dict(s=aset(ld=1)), b'2 <= ld'), (dict(s=aset(ld=1025)), b'ld <= 1024')):
        rc = call(**kw)
        assert rc == -1 and msg in l.hual_last_error(), (kw, msg, rc, l.hual_last_error())      # HUAL_ERR_INVALID
    with pytest.raises(lib.HualError):
        lib.check(rc)


def test_update_labels_refuses_an_unknown_observe_by():
    from hual_amd import al
    data_old = [['v0', 10.0, [1.0, 2.0], 'a b'], ['v1', 12.0, [3.0, 4.0], 'c d']]
    keep = copy.deepcopy(data_old)
    with pytest.raises(ValueError, match='observe_by'):
        al.update_labels(data_old, copy.deepcopy(data_old), [{'vid': 'v0'}, {'vid': 'v1'}], al.get_coff('charades', 1), observe_by='bogus')
    assert data_old == keep
    assert al.OBSERVE_BY == ('uncert_frame', 'info_gain')


# ---------------------------------------------------------------------------------------------------------------------
# the reference's own properties
@pytest.mark.parametrize('T', Q.TS)
def test_reference_inclusion_probabilities(T):
    c = Q.case(T)
    for h in Q.HISTORIES:
        for n in range(Q.N_ROWS):
            r, v, aps = c['ref'][h][n], int(c['v'][n]), c['aps'][h][n]
            assert r['status'] == Q.LIVE, (T, h, n)                     # a truthful annotator never contradicts itself
            q = r['incl']
            assert q.shape == (v,) and q.min() >= 0.0 and q.max() <= 1.0
            pos = [f for f, is_pos in aps if is_pos]
            neg = [f for f, is_pos in aps if not is_pos]
            assert all(q[f] == 0.0 for f in neg)
            if pos:
                assert (np.abs(q[min(pos):max(pos) + 1] - 1.0) <= 1e-12).all()
                assert all((q[:f + 1] == 0.0).all() for f in neg if f < min(pos))          # beyond the bounding negatives
                assert all((q[f:] == 0.0).all() for f in neg if f > max(pos))
            if h == 0:
                assert not aps and r['agree'] == 1.0
                a, b = c['ps'][n, :v].astype(np.float64), c['pe'][n, :v].astype(np.float64)
                want = np.cumsum(a) * np.cumsum(b[::-1])[::-1]
                assert np.abs(q * r['Z'] - want).max() <= 1e-12 * r['Z']


@pytest.mark.parametrize('T', Q.TS)
def test_reference_answers_only_remove_mass(T):
    c = Q.case(T)
    asked = 0
    for n in range(Q.N_ROWS):
        states = c['steps'][n]
        assert all(s['status'] == Q.LIVE for s in states)
        agree = [s['agree'] for s in states]
        # agree never increases with an added answer (1e-15: two float64 sums of the same <= 32,896 non-negative terms, grouped differently)
        assert all(b <= a + 1e-15 for a, b in zip(agree, agree[1:])), (T, n, agree)
        assert agree[0] == 1.0 and agree[-1] > 0.0
        asked += sum(s['query_gain'] > 0 for s in states[:-1])
        for s in states:
            assert 0.0 <= s['query_gain'] <= 1.0 + 1e-12 and s['post_entropy'] >= -1e-12
            if s['query_gain'] == 0:                                    # collapsed: nothing left to ask, the first frame
                assert s['query_point'] == 0
    assert asked > 0 or T == 2
    if T > 2:
        v1 = Q.N_ROWS // 2
        assert int(c['v'][v1]) == 1 and c['steps'][v1][0]['query_gain'] == 0 and abs(c['steps'][v1][0]['post_entropy']) <= 1e-12


@pytest.mark.parametrize('T', Q.TS)
def test_reference_chain_rule(T):
    """the information an answer carries about the span is the entropy of the answer: H_A - E[H after the answer at t] = h2(q(t))"""
    c = Q.case(T)
    worst = 0.0
    for h in Q.HISTORIES:
        for n in range(Q.N_ROWS):
            worst = max(worst, Q.chain_rule_residual(c['ps'][n], c['pe'][n], int(c['v'][n]), c['aps'][h][n]))
    print('T=%d: chain-rule residual %.3e bits (bar 1e-12)' % (T, worst))
    assert worst <= 1e-12


def test_reference_edge_rules():
    c = Q.case(33)
    ps, pe = c['ps'][0], c['pe'][0]
    r = Q.posterior_ref(ps, pe, 33, [(5, True), (9, True), (7, False)])      # a negative inside the positive hull
    assert r['status'] == Q.CONTRADICTORY and r['agree'] == 0.0 and r['query_point'] == -1 and r['query_gain'] == r['post_entropy'] == -1.0
    assert Q.posterior_ref(ps, pe, 3, [(0, False), (1, False), (2, False)])['status'] == Q.CONTRADICTORY      # every gap emptied
    assert Q.posterior_ref(ps, pe, 0, [])['status'] == Q.POISONED and Q.posterior_ref(ps, pe, 33, [], nan_logit=True)['agree'] == -1.0
    a, b = Q.posterior_ref(ps, pe, 20, [(4, True)]), Q.posterior_ref(ps, pe, 20, [(4, True), (20, False), (-1, True), (33, True)])
    assert a['agree'] == b['agree'] and (a['incl'] == b['incl']).all()      # an active point outside [0, v) is ignored
    one = Q.posterior_ref(ps, pe, 20, [(3, False), (4, True), (5, False)])  # one consistent span: collapsed, not an error
    assert one['status'] == Q.LIVE and one['query_gain'] == 0.0 and one['query_point'] == 0 and abs(one['post_entropy']) <= 1e-12
    assert Q.answer((3, 5), 3) and Q.answer((3, 5), 5) and not Q.answer((3, 5), 6) and not Q.answer((3, 5), 2)
