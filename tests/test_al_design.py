"""CPU: the float64 enumeration of hual_al_design (tests/al_design_ref.py) against the identities of its contract - step 0 is
hual_al_query's frame and gain, the chain rule the kernel evaluates, the bounds and the symmetry of I(D), the frames a greedy design
may hold -, the export of the symbol, and the rules of al.check_round(questions_at_once=) that come before any device is touched."""
import ctypes
import itertools

import numpy as np
import pytest

import al_design_ref as D
import al_query_ref as Q

TS = (2, 33, 70)
M = 4


def test_symbol_is_exported_and_the_abi_version_stays():
    from hual_amd import lib
    assert hasattr(ctypes.CDLL(lib.LIB_PATH), 'hual_al_design'), 'missing export hual_al_design'
    assert lib.load().hual_abi_version() == lib.ABI_VERSION == 9          # a new symbol, the ABI version stays
    assert lib.AL_DESIGN_MAX_M == D.MAX_M == 16


def _live(T, h):
    return [(n, D.case_row(T, h, n)) for n in range(Q.N_ROWS) if D.case_row(T, h, n).status == Q.LIVE]


@pytest.mark.parametrize('h', Q.HISTORIES)
@pytest.mark.parametrize('T', TS)
def test_step_zero_is_the_query(T, h):
    c = Q.case(T)
    for n, row in _live(T, h):
        ref = c['ref'][h][n]
        cand = row.candidates([])
        assert np.abs(cand - ref['gain']).max() <= 1e-12                 # I({t}) = h2(q(t))
        d = D.case_design(T, h, n, M)
        if ref['query_gain'] > 1e-12:
            assert d['frames'][0] == ref['query_point'] and abs(d['info'][0] - ref['query_gain']) <= 1e-12
        else:
            assert d['n_design'] == 0 and d['stop_reason'] == D.GAIN
        assert d['post_entropy'] == ref['post_entropy']


@pytest.mark.parametrize('h', Q.HISTORIES)
@pytest.mark.parametrize('T', TS)
def test_chain_rule(T, h):
    """I(D + t) - I(D) = sum over the outcomes o of D of P(o) h2(q_o(t)), q_o from posterior_ref on the list extended by o's answers:
    the identity the kernel's marginal gain is built on, at every prefix of the greedy design"""
    c = Q.case(T)
    worst, steps = 0.0, 0
    for n, row in _live(T, h):
        d = D.case_design(T, h, n, M)
        for m in range(d['n_design'] + (1 if d['stop_reason'] == D.GAIN else 0)):
            frames = d['frames'][:m]
            outs = row.outcomes(frames)
            assert abs(sum(p for p, _ in outs) - 1.0) <= 1e-12 and len(outs) <= m * (m + 1) // 2 + 1
            rhs = np.zeros(row.v)
            for p, answers in outs:
                post = Q.posterior_ref(c['ps'][n], c['pe'][n], row.v, row.aps + answers)
                assert post['status'] == Q.LIVE
                rhs += p * post['gain']
            worst = max(worst, float(np.abs((d['cand'][m] - d['base'][m]) - rhs).max()))
            steps += 1
    print('T=%d answers=%d: chain rule residual %.3e bits over %d steps (bar 1e-10)' % (T, h, worst, steps))
    assert worst <= 1e-10 and (steps > 0 or T == 2)


@pytest.mark.parametrize('h', Q.HISTORIES)
@pytest.mark.parametrize('T', TS)
def test_information_bounds_symmetry_and_frames(T, h):
    for n, row in _live(T, h):
        d = D.case_design(T, h, n, M)
        info = d['info']
        assert all(b >= a - 1e-12 for a, b in zip(info, info[1:]))       # non-decreasing
        for m, x in enumerate(info):
            assert x <= min(m + 1, row.H) + 1e-9
        assert len(set(d['frames'])) == len(d['frames']) and not set(d['frames']) & row.answered
        assert d['stop_reason'] in (D.BUDGET, D.GAIN) and (d['stop_reason'] == D.BUDGET) == (d['n_design'] == M)
        if d['n_design'] >= 2:
            base = row.info(d['frames'])
            assert abs(base - info[-1]) <= 1e-12
            for perm in itertools.islice(itertools.permutations(d['frames']), 1, 6):
                assert abs(row.info(list(perm)) - base) <= 1e-12
            assert abs(row.info(d['frames'] + d['frames'][:1]) - base) <= 1e-12      # a repeated frame carries nothing
        for f in row.answered:                                            # neither does an answered one
            assert abs(row.info([f])) <= 1e-12


def test_forced_prefix_stops_and_edges():
    row = D.case_row(33, 0, 0)
    free = D.greedy(row, 6)
    again = D.greedy(row, 6, forced=free['frames'])
    assert again['frames'] == free['frames'] and np.allclose(again['info'], free['info'], atol=1e-12)
    grid = D.greedy(row, 6, forced=[4, 99, 12, 20, -1, 28])               # 99 lies beyond the clip: ignored; -1 ends the prefix
    assert grid['frames'][:3] == [4, 12, 20] and 28 not in grid['frames'][:4] and grid['n_design'] == 6
    assert grid['info'][2] <= free['info'][2] + 1e-12                      # (greedy is not optimal in general; on this row it wins)
    rep = D.greedy(row, 3, forced=[7, 7, 7])
    assert rep['frames'] == [7, 7, 7] and rep['info'][0] == rep['info'][2]
    early = D.greedy(row, 6, stop_entropy=row.H - 1.5)
    assert early['stop_reason'] == D.ENTROPY and 0 < early['n_design'] < 6 and row.H - early['info'][-1] <= row.H - 1.5
    assert D.greedy(row, 6, min_gain=0.5)['stop_reason'] == D.GAIN
    one = D.case_row(33, 0, 8)
    assert one.v == 1 and D.greedy(one, 6)['n_design'] == 0 and D.greedy(one, 6)['stop_reason'] == D.GAIN
    c = Q.case(33)
    assert D.greedy(D.Row(c['ps'][0], c['pe'][0], 33, [], nan_logit=True), 6)['stop_reason'] == D.POISONED
    assert D.greedy(D.Row(c['ps'][0], c['pe'][0], 33, [(5, True), (9, True), (7, False)]), 6)['stop_reason'] == D.CONTRADICTORY


def test_check_round_rules_for_questions_at_once():
    from hual_amd import al
    ok = dict(observe_by='info_gain')
    assert al.check_round().questions_at_once == 1 and al.check_round(questions_at_once=1).questions_at_once == 1
    assert al.check_round(questions_at_once=1)[:-1] == al.check_round()[:-1]
    pol = al.check_round(questions_at_once=6, **ok)
    assert pol.questions_at_once == 6 and pol.Q == 1 and pol.reads_posterior
    assert al.check_round(questions_at_once=16, answer_noise=0.1, temperature=2.0, renew_by='posterior', **ok).questions_at_once == 16
    for bad in (0, 17, 2.5, True, 'x', None):
        with pytest.raises(ValueError, match='questions_at_once: an integer'):
            al.check_round(questions_at_once=bad, **ok)
    with pytest.raises(ValueError, match="questions_at_once > 1 needs observe_by='info_gain'"):
        al.check_round(questions_at_once=3)
    with pytest.raises(ValueError, match='questions_at_once > 1 with questions_per_clip > 1'):
        al.check_round(questions_at_once=3, questions_per_clip=3, **ok)
    with pytest.raises(ValueError, match="questions_at_once > 1 with acquire_by='label_gain'"):
        al.check_round(questions_at_once=3, acquire_by='label_gain')

    class Bank:
        K, Kmax, pass_s = 4, 4, object()
    with pytest.raises(ValueError, match="questions_at_once > 1 with posterior='ensemble'"):
        al.check_round(questions_at_once=3, posterior='ensemble', bank=Bank(), **ok)


def test_update_labels_refuses_before_touching_a_device(monkeypatch):
    from hual_amd import al

    def boom(*a, **k):
        raise AssertionError('a device was touched')
    monkeypatch.setattr(al.LabelUpdater, '__init__', boom)
    monkeypatch.setattr(al.LabelUpdater, 'from_bank', boom)
    old = [['v0', 1.0, [0.0, 1.0], 'a']]
    args = (old, [['v0', 1.0, [0.0, 1.0], 'a']], [{'vid': 'v0'}], al.get_coff('charades', 1))
    for kw in (dict(questions_at_once=0), dict(questions_at_once=17), dict(questions_at_once=3),
               dict(questions_at_once=3, observe_by='info_gain', questions_per_clip=2),
               dict(questions_at_once=3, acquire_by='label_gain')):
        with pytest.raises(ValueError):
            al.update_labels(*args, **kw)
    assert old == [['v0', 1.0, [0.0, 1.0], 'a']]                            # a refusal leaves data_old untouched
    with pytest.raises(AssertionError, match='a device was touched'):      # (the accepted form gets as far as the device)
        al.update_labels(*args, questions_at_once=3, observe_by='info_gain')
