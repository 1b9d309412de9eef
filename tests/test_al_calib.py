"""CPU: hual_al_evidence_grid (the evidence of a set's answers on a grid of temperatures and error rates: the likelihood that calibrates
the span posterior) is declared, exported and refuses bad arguments before any HIP call; al.update_labels refuses a bad temperature /
calibrate before it touches anything; and the float64 reference the GPU tests compare against (tests/al_calib_ref.py) is the definition
- al_noisy_ref.direct on the scaled row -, recovers a planted temperature and error rate, and separates the best cell of every case the
GPU tests compare by index from the runner-up."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest

import al_calib_ref as CR
import al_noisy_ref as NR
import al_query_ref as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the cases whose best cell the GPU tests compare by index: (T, history, grid, N - 1: row 0 alone, 16: the case, 1000: its rows tiled)
ARGMAX_CASES = ((2, 6, '3x2', 16), (33, 3, '3x2', 1), (33, 6, '3x2', 16), (70, 3, '3x2', 16), (256, 6, '3x2', 16), (33, 6, '32x16', 16),
                (33, 1, '32x16', 1000))
MARGIN = 1e-8      # times the sum of |cell| over the summed rows: ten times the GPU tests' bar on a total


def argmax_case(T, h, name, N):
    """the reference of one ARGMAX_CASES entry: (sel = the rows of the case the set holds, total, counts, scale)"""
    table, status, answers = CR.case_table(T, h, name)
    sel = [0] if N == 1 else [n % Q.N_ROWS for n in range(N)]
    return (sel,) + CR.fold(table, status, answers, sel)


def test_symbol_is_declared_and_exported():
    from hual_amd import build, lib
    build.build()
    src = open(os.path.join(ROOT, 'include', 'hual_seqpan.h')).read()
    assert re.search(r'\bint hual_al_evidence_grid\s*\(', src)
    assert hasattr(ctypes.CDLL(lib.LIB_PATH), 'hual_al_evidence_grid'), 'missing export'
    assert lib.load().hual_abi_version() == lib.ABI_VERSION == 9          # one new symbol, the ABI version stays
    assert callable(lib.al_evidence_grid)


def test_refuses_bad_arguments_without_a_gpu():
    from hual_amd import lib
    buf = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p(ctypes.addressof(buf))
    SET = ('vlen', 'tlen', 'ap_off', 'ap_idx', 'ap_pos')
    l = lib.load()

    def aset(N=4, ld=64, **null):
        f = {k: p.value for k in SET}
        f.update(null)
        return ctypes.byref(lib.hual_al_set(N, ld, *[f[k] for k in SET]))

    def floats(x):
        return None if x is None else (ctypes.c_float * max(len(x), 1))(*x)

    def call(s=None, s0=p, e0=p, sel=p, nsel=2, inv_tau=(1.0, 0.5), A=None, eps=(0.1, 0.2, 0.5), B=None, table=p, status=p, total=p, counts=p,
             _null_set=False):
        it, ep = floats(inv_tau), floats(eps)
        return l.hual_al_evidence_grid(None if _null_set else (s or aset()), s0, e0, sel, nsel, it, len(inv_tau) if A is None else A, ep,
                                       len(eps) if B is None else B, table, status, total, counts, None)
    nan, inf = float('nan'), float('inf')
    cases = [(dict(_null_set=True), b'null set'), (dict(s0=None), b'null input'), (dict(e0=None), b'null input'),
             (dict(inv_tau=None, A=1), b'null grid'), (dict(eps=None, B=1), b'null grid'),
             (dict(table=None), b'null output'), (dict(status=None), b'null output'), (dict(total=None), b'null output'),
             (dict(counts=None), b'null output'),
             (dict(nsel=0), b'nsel >= 1'), (dict(nsel=-3), b'nsel >= 1'), (dict(sel=None, nsel=0), b'nsel >= 1'),
             (dict(s=aset(N=0)), b'N > 0'), (dict(s=aset(N=-2)), b'N > 0'), (dict(s=aset(ld=1)), b'2 <= ld'), (dict(s=aset(ld=1025)), b'ld <= 1024'),
             (dict(A=0), b'A in [1, 32]'), (dict(A=33), b'A in [1, 32]'), (dict(A=-1), b'A in [1, 32]'),
             (dict(B=0), b'B in [1, 16]'), (dict(B=17), b'B in [1, 16]'), (dict(B=-1), b'B in [1, 16]')]
    cases += [(dict(s=aset(**{k: None})), b'null input') for k in SET]
    cases += [(dict(inv_tau=(1.0, x)), b'inv_tau finite and > 0') for x in (0.0, -1.0, nan, inf, -inf)]
    cases += [(dict(eps=(0.1, x)), b'eps in (0, 0.5]') for x in (0.0, -0.1, 0.5000001, 1.0, nan, inf)]
    for kw, msg in cases:
        rc = call(**kw)
        assert rc == -1 and msg in l.hual_last_error(), (kw, msg, rc, l.hual_last_error())      # HUAL_ERR_INVALID
    with pytest.raises(lib.HualError):
        lib.check(rc)


def test_update_labels_refuses_bad_calibration_arguments():
    from hual_amd import al
    data_old = [['v0', 10.0, [1.0, 2.0], 'a b'], ['v1', 12.0, [3.0, 4.0], 'c d']]
    keep = copy.deepcopy(data_old)
    prop, coff = [{'vid': 'v0'}, {'vid': 'v1'}], al.get_coff('charades', 1)
    for kw in (dict(calibrate='evidence'),                             # no reader of the posterior is on
               dict(calibrate='gradient', renew_by='posterior'), dict(calibrate=True, soft_out={})):
        with pytest.raises(ValueError, match='calibrate'):
            al.update_labels(data_old, copy.deepcopy(data_old), prop, coff, **kw)
        assert data_old == keep
    for kw in (dict(temperature=2.0),                                  # no reader of the posterior is on
               dict(temperature=0.0, renew_by='posterior'), dict(temperature=-1.0, soft_out={}),
               dict(temperature=float('nan'), observe_by='info_gain'), dict(temperature=float('inf'), observe_by='info_gain'),
               dict(temperature='hot', acquire_by='label_gain'), dict(temperature=True, renew_by='posterior')):
        with pytest.raises(ValueError, match='temperature'):
            al.update_labels(data_old, copy.deepcopy(data_old), prop, coff, **kw)
        assert data_old == keep


def test_run_round_hands_both_arguments_to_the_label_update(monkeypatch):
    import types
    from hual_amd import al
    seen = {}

    class Stop(Exception):
        pass

    def observed(*args, **kw):
        seen.update(kw)
        raise Stop
    monkeypatch.setattr(al, 'update_labels', observed)
    with pytest.raises(Stop):
        al.run_round(types.SimpleNamespace(device='cpu'), None, [], [], [], 'charades', 1, epochs=1, batch_size=16, lr=1e-3, drop_rate=0.2,
                     renew_by='posterior', temperature=1.5, calibrate='evidence')
    assert seen['temperature'] == 1.5 and seen['calibrate'] == 'evidence' and seen['return_debug'] is True
    seen.clear()
    with pytest.raises(Stop):
        al.run_round(types.SimpleNamespace(device='cpu'), None, [], [], [], 'charades', 1, epochs=1, batch_size=16, lr=1e-3, drop_rate=0.2)
    assert seen['temperature'] is None and seen['calibrate'] is None and seen['return_debug'] is False
    with pytest.raises(ValueError, match='calibrate'):
        al.run_round(types.SimpleNamespace(device='cpu'), None, [], [], [], 'charades', 1, epochs=1, batch_size=16, lr=1e-3, drop_rate=0.2,
                     calibrate='evidence')


def test_zoom_grids():
    from hual_amd import al
    x = np.array(al.CALIB_TAUS)
    assert len(x) == 17 and x[8] == 1.0 and abs(x[0] - 0.25) < 1e-15 and abs(x[-1] - 4.0) < 1e-15 and len(al.CALIB_EPS) == 10
    z = al._zoom_axis(x, 8, 17, 0.0, float('inf'))
    assert len(z) == 17 and abs(z[0] - x[7]) < 1e-15 and abs(z[-1] - x[9]) < 1e-15 and abs(z[8] - 1.0) < 1e-12
    z = al._zoom_axis(x, 0, 5, 0.0, float('inf'))                      # the best cell on the edge: one step past it
    assert abs(z[0] - x[0] * x[0] / x[1]) < 1e-15 and abs(z[-1] - x[1]) < 1e-15
    odds = np.array(al.CALIB_EPS) / (1.0 - np.array(al.CALIB_EPS))
    z = al._zoom_axis(odds, 9, 10, 1e-6, 1.0)                          # eps = 0.5 is the last legal value
    assert z[-1] == 1.0 and abs(z[0] - odds[8]) < 1e-15
    assert list(al._zoom_axis(np.array([0.5, 1.0]), 1, 4, 1.0, 1.0)) == [1.0]


# ---------------------------------------------------------------------------------------------------------------------
# the reference's own properties
@pytest.mark.parametrize('T', (2, 33))
def test_reference_cell_at_temperature_one_is_the_noisy_evidence(T):
    """inv_tau = 1 scales nothing: the cell is al_noisy_ref's log-evidence of the same row - and the per-class enumeration the GPU
    tests use is the span-by-span one at any temperature"""
    worst, worst2 = 0.0, 0.0
    for eps in NR.EPS:
        c = NR.tilted_case(T, eps)
        for h in NR.HISTORIES:
            for n in range(Q.N_ROWS):
                v = int(c['v'][n])
                want = c['dir'][h][n]['log_evidence']
                got = CR.cell_direct(c['s'][n].numpy(), c['e'][n].numpy(), v, c['naps'][h][n], np.float32(1.0), eps)
                assert got == want or (not CR.counted(v, c['naps'][h][n]) and got == 0.0 and abs(want) < 1e-12), (T, eps, h, n)
                fast = CR.row_cells(c['ps'][n], c['pe'][n], v, c['naps'][h][n], [eps])[0]
                worst = max(worst, abs(fast - want))
                for tau in (0.5, 3.0):
                    k = CR.inv32(tau)
                    ps, pe = NR.probabilities(CR.scale(c['s'][n].numpy()[:v], k), CR.scale(c['e'][n].numpy()[:v], k), v)
                    d = CR.cell_direct(c['s'][n].numpy(), c['e'][n].numpy(), v, c['naps'][h][n], k, eps)
                    worst2 = max(worst2, abs(CR.row_cells(ps, pe, v, c['naps'][h][n], [eps])[0] - d))
    print('T=%d: max |per-class - span-by-span| = %.2e at tau = 1, %.2e at tau in (0.5, 3)' % (T, worst, worst2))
    assert worst <= 1e-12 and worst2 <= 1e-12


def test_reference_edges():
    s, e = np.array([0.0, 30.0], dtype=np.float32), np.array([30.0, 0.0], dtype=np.float32)
    aps = [(0, True)]
    assert np.isfinite(CR.cell_direct(s, e, 2, aps, np.float32(1.0), 0.1))
    assert np.isnan(CR.cell_direct(s, e, 2, aps, np.float32(8.0), 0.1))       # one-hot with the start behind the end: Z == 0
    assert np.isnan(CR.cell_direct(np.array([np.nan, 0], dtype=np.float32), e, 2, aps, np.float32(1.0), 0.1))
    assert np.isnan(CR.cell_direct(s, e, 0, aps, np.float32(1.0), 0.1))
    assert CR.cell_direct(s, e, 2, [(5, True), (-1, False)], np.float32(1.0), 0.1) == 0.0      # no answer inside the clip
    table, status, answers = CR.set_table(np.stack([s, s]), np.stack([e, e]), [2, 2], [2, 2], [aps, []], [np.float32(1.0), np.float32(8.0)], [0.1, 0.3])
    assert np.isfinite(table[0, :2]).all() and np.isnan(table[:, 2:]).all() and (table[1, :2] == 0).all() and list(status) == [0, 0]
    total, counts, _ = CR.fold(table, status, answers)
    assert list(counts) == [0, 0, 2, -1] and (total == 0).all()
    c = Q.case(33)
    many = NR.many_answers(33)
    x = CR.row_cells(c['ps'][0], c['pe'][0], 33, many, [1e-6])[0]
    assert np.isfinite(x) and abs(x - NR.direct(c['ps'][0], c['pe'][0], 33, many, 1e-6)['log_evidence']) <= 1e-9 * abs(x)


@pytest.mark.parametrize('seed', (0, 1, 2, 3))
@pytest.mark.parametrize('tau,eps,scale', CR.PLANTED)
def test_planted_temperature_and_noise_are_recovered(tau, eps, scale, seed):
    """192 rows whose span is drawn from the posterior at tau* and answered six times by an annotator who errs at eps*: the cell of
    maximal evidence has eps == eps* and tau within one grid step of tau*"""
    p = CR.planted(tau, eps, scale, seed)
    total, counts, _ = CR.set_totals(p, CR.PLANT_TAUS, CR.PLANT_EPS)
    ia, ib = divmod(int(np.argmax(total)), len(CR.PLANT_EPS))
    print('tau* = %g eps* = %g scale %g seed %d: best cell tau = %g eps = %g, %d rows, %d answers'
          % (tau, eps, scale, seed, CR.PLANT_TAUS[ia], CR.PLANT_EPS[ib], counts[0], counts[1]))
    assert counts[0] == CR.PLANT_N and counts[1] == CR.PLANT_N * CR.PLANT_ANSWERS and counts[2] == 0 and counts[3] == ia * len(CR.PLANT_EPS) + ib
    assert CR.PLANT_EPS[ib] == eps
    assert abs(ia - CR.PLANT_TAUS.index(tau)) <= 1


@pytest.mark.parametrize('T,h,name,N', ARGMAX_CASES)
def test_best_cell_of_the_gpu_cases_stands_clear(T, h, name, N):
    """the GPU tests compare counts[3] exactly on these: the reference's best total exceeds the second best by more than MARGIN times the
    sum of |cell| over the summed rows, ten times the bar a GPU total is held to - a launch within its bar cannot prefer another cell"""
    sel, total, counts, scale = argmax_case(T, h, name, N)
    m = CR.margin(total)
    print('T=%d answers=%d grid %s N=%d: best cell %d, margin %.3e, sum |cell| %.3e (needs > %.3e)' % (T, h, name, N, counts[3], m, scale.max(),
                                                                                              MARGIN * scale.max()))
    assert counts[0] >= 1 and m > MARGIN * scale.max()
