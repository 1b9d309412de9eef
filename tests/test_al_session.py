"""CPU: the float64 reference of hual_al_session (tests/al_session_ref.py) against the six-question sessions al_query_ref.case already
holds, its own rules (no frame twice, the flip mask, every stop reason), the argument checks of al.update_labels(questions_per_clip=)
that come before any device is touched, and the share of decisions too close to a threshold for the GPU test to compare."""
import numpy as np
import pytest

import al_query_ref as Q
import al_session_ref as S


@pytest.mark.parametrize('T', Q.TS)
def test_reference_reproduces_the_six_question_case(T):
    c = Q.case(T)
    got = S.sessions(T, 0, 0.0, False, 6)
    for n in range(Q.N_ROWS):
        r = got[n]
        assert r['aps'] == c['aps'][6][n], n
        assert r['n_asked'] == len(c['aps'][6][n])
        for k in range(7):                                            # (past the collapse the case's states repeat the last one)
            want = c['steps'][n][k]['post_entropy']
            assert r['entropy'][min(k, r['n_asked'])] == want, (n, k)
        assert r['stop_reason'] == (S.BUDGET if r['n_asked'] == 6 and c['steps'][n][6]['query_gain'] > 0 else S.GAIN)
        assert r['answer'] == [Q.answer(c['gt'][n], t) for t in r['asked']]


@pytest.mark.parametrize('T', Q.TS)
def test_no_frame_twice_under_the_hard_rule(T):
    for flipped in (False, True):
        for start in S.STARTS:
            for r in S.sessions(T, start, 0.0, flipped, 6):
                frames = [f for f, _ in r['aps']]
                assert len(set(frames)) == len(frames)


@pytest.mark.parametrize('T', Q.TS)
def test_flip_mask_flips_exactly_the_marked_answers(T):
    c, fm = Q.case(T), S.flip_masks(T)
    assert fm.any()
    for eps in (0.0, 0.2):
        n_flipped = 0
        for n, r in enumerate(S.sessions(T, 0, eps, True, 6)):
            for k, (t, a) in enumerate(zip(r['asked'], r['answer'])):
                marked = bool((int(fm[n]) >> k) & 1)
                assert a == (Q.answer(c['gt'][n], t) != marked)
                n_flipped += marked
        assert n_flipped > 0 or T == 2


def test_every_stop_reason_is_reached():
    seen = set()
    c = Q.case(33)
    r = S.sessions(33, 0, 0.0, False, 6)
    assert int(c['v'][8]) == 1 and r[8]['stop_reason'] == S.GAIN and r[8]['n_asked'] == 0      # v = 1: nothing to gain
    early = [x for x in S.sessions(33, 0, 0.0, False, 6, 1.0, 0.0) if x['stop_reason'] == S.ENTROPY]
    assert early and any(x['n_asked'] < y['n_asked'] for x, y in zip(S.sessions(33, 0, 0.0, False, 6, 1.0, 0.0), r))
    for x in early:
        assert x['entropy'][-1] <= 1.0 and all(h > 1.0 for h in x['entropy'][:-1])
    # a question is only asked where both answers leave a consistent span, so a flip inside a session misleads without contradicting;
    # a flipped answer of an EARLIER round - asked under another list - does: the session stops before its first question
    for T in Q.TS:
        for start in S.STARTS:
            for flipped in (False, True):
                for x in S.sessions(T, start, 0.0, flipped, 6) + S.sessions(T, start, 0.0, flipped, 6, 1.0, 0.0):
                    seen.add(x['stop_reason'])
                    if x['stop_reason'] == S.CONTRADICTORY:
                        assert start == 'flipped3' and x['n_asked'] == 0 and x['entropy'] == [-1.0]
    assert {S.BUDGET, S.ENTROPY, S.GAIN, S.CONTRADICTORY} <= seen
    # under noise no answer contradicts
    assert all(x['stop_reason'] != S.CONTRADICTORY for x in S.sessions(33, 'flipped3', 0.2, True, 6))
    # a NaN logit, and a list that cannot hold the budget
    s, e = c['s'][0].numpy(), c['e'][0].numpy()
    assert S.session(s, e, 33, [], c['gt'][0], 6, nan_logit=True)['stop_reason'] == S.POISONED
    full = [(0, False)] * 60
    assert S.session(s, e, 33, full, c['gt'][0], 6)['stop_reason'] == S.OVERFLOW
    assert S.session(s, e, 33, full, c['gt'][0], 6, budget=4)['stop_reason'] != S.OVERFLOW
    # the budget: 0 asks nothing, one above qmax is qmax
    assert S.session(s, e, 33, [], c['gt'][0], 6, budget=0)['n_asked'] == 0
    assert S.session(s, e, 33, [], c['gt'][0], 3, budget=9)['n_asked'] == 3


def test_update_labels_refuses_before_touching_a_device(monkeypatch):
    from hual_amd import al

    def boom(*a, **k):
        raise AssertionError('a device was touched')
    monkeypatch.setattr(al.LabelUpdater, '__init__', boom)
    monkeypatch.setattr(al.LabelUpdater, 'from_bank', boom)
    args = ([['v0', 1.0, [0.0, 1.0], 'a']], [['v0', 1.0, [0.0, 1.0], 'a']], [{'vid': 'v0'}], al.get_coff('charades', 1))
    for kw in (dict(questions_per_clip=0), dict(questions_per_clip=17), dict(questions_per_clip=2.5), dict(questions_per_clip=3),
               dict(questions_per_clip=3, observe_by='uncert_frame'), dict(questions_per_clip=3, acquire_by='label_gain'),
               dict(questions_per_clip=1, stop_entropy=1.0), dict(questions_per_clip=3, observe_by='info_gain', stop_entropy=-1.0)):
        with pytest.raises(ValueError):
            al.update_labels(*args, **kw)
    with pytest.raises(AssertionError, match='a device was touched'):      # (the accepted form gets as far as the device)
        al.update_labels(*args, questions_per_clip=3, observe_by='info_gain')


def test_few_decisions_lie_near_a_threshold():
    """the (row, step) pairs the teacher-forced GPU comparison skips: at most 5 % of the seeded cases' steps"""
    near = total = 0
    for T in Q.TS:
        for start, eps, flipped in S.TEACHER_GRID:
            for r in S.sessions(T, start, eps, flipped, 6, S.STOP_ENTROPY, S.MIN_GAIN):
                total += len(r['posts'])
                near += sum(S.near_threshold(p, S.STOP_ENTROPY, S.MIN_GAIN) for p in r['posts'])
    print('%d of %d (row, step) pairs lie within %.0e bits of a threshold: %.2f %%' % (near, total, S.NEAR, 100.0 * near / total))
    assert total > 500 and near <= 0.05 * total
