"""CPU: hual_al_mbr_label (the pseudo-label by minimum Bayes risk under the answered-point posterior) is declared, exported and refuses
bad arguments before any HIP call; al.update_labels refuses an unknown renew_by before it touches anything; and the float64
reference the GPU tests compare against (tests/al_label_ref.py) has the properties that define the quantity - on the very cases the
GPU tests use (al_query_ref.case: T in {2, 33, 70, 256}, 16 rows, after 0, 1, 3 and 6 truthful answers) - together with the margin
between its best and second-best span that the GPU tests' exact comparison of indices rests on."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest

import al_label_ref as L
import al_query_ref as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 1e-5        # ten times the GPU tests' 1e-6 bar on R: a kernel within the bar of every R cannot prefer another span


def test_symbol_is_declared_and_exported():
    from hual_amd import build, lib
    build.build()
    src = open(os.path.join(ROOT, 'include', 'hual_seqpan.h')).read()
    assert re.search(r'\bint hual_al_mbr_label\s*\(', src)
    assert hasattr(ctypes.CDLL(lib.LIB_PATH), 'hual_al_mbr_label'), 'missing export hual_al_mbr_label'
    assert lib.load().hual_abi_version() == lib.ABI_VERSION == 9          # a new symbol, the ABI version stays
    assert callable(lib.al_mbr_label)


def test_label_refuses_bad_arguments_without_a_gpu():
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

    def call(s=None, s0=p, e0=p, sel=p, nsel=2, old=p, new=p, conf=p, oconf=p, _null_set=False):
        return l.hual_al_mbr_label(None if _null_set else (s or aset()), s0, e0, sel, nsel, old, new, conf, oconf, None)
    for kw, msg in ((dict(_null_set=True), b'null set'), (dict(s0=None), b'null input'), (dict(e0=None), b'null input'),
                    (dict(s=aset(vlen=None)), b'null input'), (dict(s=aset(tlen=None)), b'null input'),
                    (dict(s=aset(ap_off=None)), b'null input'), (dict(s=aset(ap_idx=None)), b'null input'),
                    (dict(s=aset(ap_pos=None)), b'null input'),
                    (dict(new=None), b'null output'), (dict(conf=None), b'null output'),
                    (dict(old=None), b'both set or both null'), (dict(oconf=None), b'both set or both null'),
                    (dict(nsel=0), b'nsel >= 1'), (dict(nsel=-3), b'nsel >= 1'), (dict(sel=None, nsel=0), b'nsel >= 1'),
                    (dict(s=aset(N=0)), b'N > 0'), (dict(s=aset(ld=1)), b'2 <= ld'), (dict(s=aset(ld=1025)), b'ld <= 1024')):
        rc = call(**kw)
        assert rc == -1 and msg in l.hual_last_error(), (kw, msg, rc, l.hual_last_error())      # HUAL_ERR_INVALID
    with pytest.raises(lib.HualError):
        lib.check(rc)


def test_update_labels_refuses_an_unknown_renew_by():
    from hual_amd import al
    data_old = [['v0', 10.0, [1.0, 2.0], 'a b'], ['v1', 12.0, [3.0, 4.0], 'c d']]
    keep = copy.deepcopy(data_old)
    with pytest.raises(ValueError, match='renew_by'):
        al.update_labels(data_old, copy.deepcopy(data_old), [{'vid': 'v0'}, {'vid': 'v1'}], al.get_coff('charades', 1), renew_by='bogus')
    assert data_old == keep
    assert al.RENEW_BY == ('heuristic', 'posterior')


# ---------------------------------------------------------------------------------------------------------------------
# the reference's own properties
@pytest.mark.parametrize('T', Q.TS)
def test_reference_label_properties(T):
    c = L.case(T)
    full = differs = 0
    for h in Q.HISTORIES:
        for n in range(Q.N_ROWS):
            r, v, aps = c['lref'][h][n], int(c['v'][n]), c['aps'][h][n]
            assert r['status'] == L.LIVE, (T, h, n)                     # a truthful annotator never contradicts itself
            st = r['st']
            old = tuple(int(x) for x in c['old'][h][n])
            assert L.old_valid(old, v) and (n % 2 == 1 or L.is_member(st, *old))
            if not r['full']:
                continue
            full += 1
            a, e = r['label']
            assert L.is_member(st, a, e)
            assert all(a <= f <= e for f, is_pos in aps if is_pos) and not any(a <= f <= e for f, is_pos in aps if not is_pos)
            assert 0.0 <= r['conf'] <= 1.0 + 1e-12
            assert abs(L.span_R(st, a, e) - r['conf']) <= 1e-15
            assert r['conf'] >= L.span_R(st, *r['mode'])
            # >= R of the old span: by definition where the old span is a member of A; on these seeded cases also where it is not (an
            # old span that crosses an answered negative overlaps the mass on either side of it only in part)
            assert r['conf'] >= c['old_conf'][h][n]
            differs += r['label'] != r['mode']
            if r['size'] == 1:                                          # collapsed: its one span, conf 1
                assert r['label'] == (int(st['ai'][0]), int(st['aj'][0])) and abs(r['conf'] - 1.0) <= 1e-15
            if v == 1:
                assert r['label'] == (0, 0) and r['conf'] == 1.0
    assert full == 4 * Q.N_ROWS or T == 256
    assert differs > 0 or T == 2                                        # another label than the posterior's mode


def test_reference_edge_rules():
    c = Q.case(33)
    ps, pe = c['ps'][0], c['pe'][0]
    r = L.label_ref(ps, pe, 33, [(5, True), (9, True), (7, False)])       # a negative inside the positive hull
    assert r['status'] == L.CONTRADICTORY and r['label'] == (-1, -1) and r['conf'] == -1.0
    assert L.label_ref(ps, pe, 3, [(0, False), (1, False), (2, False)])['status'] == L.CONTRADICTORY      # every frame negative
    assert L.label_ref(ps, pe, 0, [])['status'] == L.POISONED and L.label_ref(ps, pe, 33, [], nan_logit=True)['label'] == (-1, -1)
    a, b = L.label_ref(ps, pe, 20, [(4, True)]), L.label_ref(ps, pe, 20, [(4, True), (20, False), (-1, True), (33, True)])
    assert a['label'] == b['label'] and a['conf'] == b['conf'] and a['size'] == b['size']      # an active point outside [0, v) is ignored
    one = L.label_ref(ps, pe, 20, [(3, False), (4, True), (5, False)])    # one consistent span: collapsed, not an error
    assert one['status'] == L.LIVE and one['label'] == (4, 4) and abs(one['conf'] - 1.0) <= 1e-15 and one['margin'] == np.inf
    assert L.label_ref(ps, pe, 1, [])['label'] == (0, 0)
    # R of a span outside A, and of a span that overlaps nothing of A
    st = L.state(ps, pe, 20, [(10, True), (15, False)])
    assert 0.0 < L.span_R(st, 0, 19) < 1.0 and L.span_R(st, 16, 19) == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# what the GPU tests' comparison of indices rests on
@pytest.mark.parametrize('T', Q.TS)
def test_reference_margin_of_the_rows_compared_by_index(T):
    c = L.case(T)
    rows = [(h, n) for h in Q.HISTORIES for n in range(Q.N_ROWS) if c['lref'][h][n]['full']]
    margin = min(c['lref'][h][n]['margin'] for h, n in rows)
    print('T=%d: %d of %d row-states enumerated in full, smallest margin between best and runner-up %.3e (bar %.0e)'
          % (T, len(rows), 4 * Q.N_ROWS, margin, MARGIN))
    assert len(rows) == 4 * Q.N_ROWS if T < 256 else len(rows) >= 30      # the full comparison cannot quietly shrink
    assert all(c['lref'][h][n]['size'] <= L.FULL_MAX for h, n in rows)
    assert margin > MARGIN
