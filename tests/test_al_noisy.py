"""CPU: hual_al_noisy_tilt and hual_al_label_gain_noisy (the span posterior under an annotator who errs with probability eps) are
declared, exported and refuse bad arguments before any HIP call; al.update_labels refuses a bad answer_noise / annotator_flip before it
touches anything; and the float64 reference the GPU tests compare against (tests/al_noisy_ref.py) has the properties that define the
quantities - on the very states the GPU tests use (al_query_ref.case: T in {2, 33} with 16 rows, T = 70 with rows 0-3, after 1, 3 and 6
answers of which a seeded 30 % are flipped; eps in {0.05, 0.2}) - together with the number of states whose best frame stands far
enough above the runner-up for the GPU tests to compare the index itself."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest

import al_noisy_ref as NR
import al_query_ref as Q
import soft_label_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# states with a best gain above 1e-9 whose margin over the second-best frame exceeds 1e-5 (ten times the GPU tests' 1e-6 bar on a gain: a
# kernel within the bar of every gain cannot prefer another frame), per (T, eps) and history (1, 3, 6) - measured with the brute force -
# and beside them the number of states with a gain above 1e-9 at all: at most a quarter of those may be left out
BY_INDEX = {(2, 0.05): ((5, 5, 5), 17), (2, 0.2): ((5, 5, 5), 15), (33, 0.05): ((15, 14, 15), 45), (33, 0.2): ((12, 13, 13), 40),
            (70, 0.05): ((3, 4, 4), 12), (70, 0.2): ((3, 4, 3), 12)}
CASES = sorted(BY_INDEX)


def test_symbols_are_declared_and_exported():
    from hual_amd import build, lib
    build.build()
    src = open(os.path.join(ROOT, 'include', 'hual_seqpan.h')).read()
    for name in ('hual_al_noisy_tilt', 'hual_al_label_gain_noisy'):
        assert re.search(r'\bint %s\s*\(' % name, src)
        assert hasattr(ctypes.CDLL(lib.LIB_PATH), name), 'missing export ' + name
    assert lib.load().hual_abi_version() == lib.ABI_VERSION == 9          # two new symbols, the ABI version stays
    assert callable(lib.al_noisy_tilt) and callable(lib.al_label_gain_noisy)


def _args():
    from hual_amd import lib
    buf = ctypes.create_string_buffer(64)
    a = ctypes.addressof(buf)
    SET = ('vlen', 'tlen', 'ap_off', 'ap_idx', 'ap_pos')

    def aset(N=4, ld=64, **null):
        f = {k: a for k in SET}
        f.update(null)
        return ctypes.byref(lib.hual_al_set(N, ld, *[f[k] for k in SET]))
    return lib.load(), buf, ctypes.c_void_p(a), aset


BAD_EPS = (0.0, -0.1, 0.5000001, 1.0, float('nan'), float('inf'))
BAD_SETS = (('vlen', b'null input'), ('tlen', b'null input'), ('ap_off', b'null input'), ('ap_idx', b'null input'), ('ap_pos', b'null input'))


def test_tilt_refuses_bad_arguments_without_a_gpu():
    from hual_amd import lib
    l, buf, p, aset = _args()

    def call(s=None, s0=p, e0=p, eps=0.1, s_t=p, e_t=p, ev=p, _null_set=False):
        return l.hual_al_noisy_tilt(None if _null_set else (s or aset()), s0, e0, eps, s_t, e_t, ev, None)
    cases = [(dict(_null_set=True), b'null set'), (dict(s0=None), b'null input'), (dict(e0=None), b'null input'),
             (dict(s_t=None), b'null output'), (dict(e_t=None), b'null output'), (dict(ev=None), b'null output'),
             (dict(s=aset(N=0)), b'N > 0'), (dict(s=aset(ld=1)), b'2 <= ld'), (dict(s=aset(ld=1025)), b'ld <= 1024')]
    cases += [(dict(s=aset(**{k: None})), msg) for k, msg in BAD_SETS] + [(dict(eps=e), b'eps in (0, 0.5]') for e in BAD_EPS]
    for kw, msg in cases:
        rc = call(**kw)
        assert rc == -1 and msg in l.hual_last_error(), (kw, msg, rc, l.hual_last_error())      # HUAL_ERR_INVALID
    with pytest.raises(lib.HualError):
        lib.check(rc)


def test_noisy_gain_refuses_bad_arguments_without_a_gpu():
    from hual_amd import lib
    l, buf, p, aset = _args()

    def call(s=None, s0=p, e0=p, eps=0.1, sel=p, nsel=2, cand=p, M=4, gain=p, point=p, ask=p, value=p, _null_set=False):
        return l.hual_al_label_gain_noisy(None if _null_set else (s or aset()), s0, e0, eps, sel, nsel, cand, M, gain, point, ask, value, None)
    cases = [(dict(_null_set=True), b'null set'), (dict(s0=None), b'null input'), (dict(e0=None), b'null input'),
             (dict(point=None), b'null output'), (dict(ask=None), b'null output'), (dict(value=None), b'null output'),
             (dict(nsel=0), b'nsel >= 1'), (dict(nsel=-3), b'nsel >= 1'), (dict(sel=None, nsel=0), b'nsel >= 1'),
             (dict(s=aset(N=0)), b'N > 0'), (dict(s=aset(ld=1)), b'2 <= ld'), (dict(s=aset(ld=1025)), b'ld <= 1024'),
             (dict(M=0), b'1 <= M <= 256'), (dict(M=257), b'1 <= M <= 256'), (dict(M=-1), b'1 <= M <= 256')]
    cases += [(dict(s=aset(**{k: None})), msg) for k, msg in BAD_SETS] + [(dict(eps=e), b'eps in (0, 0.5]') for e in BAD_EPS]
    for kw, msg in cases:
        rc = call(**kw)
        assert rc == -1 and msg in l.hual_last_error(), (kw, msg, rc, l.hual_last_error())      # HUAL_ERR_INVALID
    with pytest.raises(lib.HualError):
        lib.check(rc)


def test_update_labels_refuses_bad_noise_arguments():
    from hual_amd import al
    data_old = [['v0', 10.0, [1.0, 2.0], 'a b'], ['v1', 12.0, [3.0, 4.0], 'c d']]
    keep = copy.deepcopy(data_old)
    prop, coff = [{'vid': 'v0'}, {'vid': 'v1'}], al.get_coff('charades', 1)
    rng = np.random.default_rng(0)
    for kw in (dict(answer_noise=0.1),                                 # no reader of the posterior is on
               dict(answer_noise=0.0, renew_by='posterior'), dict(answer_noise=0.6, renew_by='posterior'),
               dict(answer_noise=-0.1, soft_out={}), dict(answer_noise=float('nan'), observe_by='info_gain'),
               dict(answer_noise='much', acquire_by='label_gain')):
        with pytest.raises(ValueError, match='answer_noise'):
            al.update_labels(data_old, copy.deepcopy(data_old), prop, coff, **kw)
        assert data_old == keep
    for flip in (0.3, (0.3,), (0.3, 7), (1.5, rng), (-0.1, rng), ('x', rng), (0.3, rng, 1)):
        with pytest.raises(ValueError, match='annotator_flip'):
            al.update_labels(data_old, copy.deepcopy(data_old), prop, coff, annotator_flip=flip)
        assert data_old == keep
    for e in (0.0, 0.51, float('nan'), None, True):
        with pytest.raises(ValueError):
            al.check_noise(e)
    assert al.check_noise(0.5) == 0.5 and al.check_noise(0.05) == float(np.float32(0.05))


def test_run_round_hands_both_switches_to_the_label_update(monkeypatch):
    import types
    from hual_amd import al
    seen = {}

    class Stop(Exception):
        pass

    def observed(*args, **kw):
        seen.update(kw)
        raise Stop
    monkeypatch.setattr(al, 'update_labels', observed)
    flip = (0.3, np.random.default_rng(0))
    with pytest.raises(Stop):
        al.run_round(types.SimpleNamespace(device='cpu'), None, [], [], [], 'charades', 1, epochs=1, batch_size=16, lr=1e-3, drop_rate=0.2,
                     renew_by='posterior', answer_noise=0.1, annotator_flip=flip)
    assert seen['answer_noise'] == 0.1 and seen['annotator_flip'] is flip and seen['renew_by'] == 'posterior'
    seen.clear()
    with pytest.raises(Stop):
        al.run_round(types.SimpleNamespace(device='cpu'), None, [], [], [], 'charades', 1, epochs=1, batch_size=16, lr=1e-3, drop_rate=0.2)
    assert seen['answer_noise'] is None and seen['annotator_flip'] is None


# ---------------------------------------------------------------------------------------------------------------------
# the reference's own properties
@pytest.mark.parametrize('T,eps', CASES)
def test_tilted_product_form_is_the_direct_likelihood(T, eps):
    """the identity the feature rests on: the float32-tilted rows' product form against the answer-by-answer, span-by-span product of
    likelihoods.  Bar 1e-5 on every span probability: float32 rounding of two logits of magnitude <= 32 (about 4e-6) and the normaliser"""
    c = NR.tilted_case(T, eps)
    worst, contra = 0.0, 0
    for h in NR.HISTORIES:
        for n in range(Q.N_ROWS):
            v = int(c['v'][n])
            P = NR.tilted(c['pst'][h][n], c['pet'][h][n], v)
            worst = max(worst, float(np.abs(P - c['dir'][h][n]['P']).max()))
            contra += c['hard'][h][n]['status'] == Q.CONTRADICTORY
            assert c['dir'][h][n]['log_evidence'] <= 1e-12               # a probability
    print('T=%d eps=%g: max |tilted - direct| over every span = %.2e; %d of %d states contradictory under the hard rule'
          % (T, eps, worst, contra, len(NR.HISTORIES) * Q.N_ROWS))
    assert worst <= 1e-5
    assert contra > 0 or T == 2


def test_no_noise_to_speak_of_is_the_hard_rule():
    """eps = 1e-6 on the states that are consistent with hard agree >= 0.01: the noisy marginals are within 1e-3 of the hard ones - the
    mass outside A is <= (1 / agree - 1) / r <= 1e-4"""
    T, eps = 33, 1e-6
    c = NR.tilted_case(T, eps)
    worst, used = 0.0, 0
    for h in NR.HISTORIES:
        for n in range(Q.N_ROWS):
            hard = c['hard'][h][n]
            if hard['status'] != Q.LIVE or hard['agree'] < 0.01:
                continue
            v = int(c['v'][n])
            m = S.marginals_ref(c['ps'][n], c['pe'][n], v, c['naps'][h][n])
            ys, ye = NR.marginals_of(NR.tilted(c['pst'][h][n], c['pet'][h][n], v))
            worst = max(worst, float(np.abs(ys - m['y_start']).max()), float(np.abs(ye - m['y_end']).max()))
            used += 1
    print('eps=1e-6: %d consistent states, max |noisy - hard| marginal = %.2e' % (used, worst))
    assert used >= 16 and worst <= 1e-3


@pytest.mark.parametrize('T,eps', CASES)
def test_reference_noisy_gain_properties(T, eps):
    c = NR.gain_case(T, eps)
    raw_min, gained, elsewhere = np.inf, 0, 0
    for h in NR.HISTORIES:
        for n in NR.ROWS[T]:
            r, v = c['gref'][h][n], int(c['v'][n])
            assert r['status'] == NR.LIVE and r['frames'] == list(range(v)), (T, h, n)      # no state is contradictory any more
            assert abs(r['value'] - c['lref'][h][n]['conf']) <= 1e-14   # V0 is the MBR value on the set without answers
            assert r['gain'].min() >= 0.0 and r['gain'].max() <= 1.0 - r['value'] + 1e-12
            raw_min = min(raw_min, float(np.nanmin(r['raw'])))
            half = NR.noisy_gain_ref(c['pst'][h][n], c['pet'][h][n], v, 0.5)
            assert np.abs(half['raw']).max() <= 1e-12 and abs(half['value'] - r['value']) <= 1e-14      # an answer worth a coin flip
            if r['ask_gain'] > 1e-9:
                gained += 1
                elsewhere += r['ask_point'] != c['qref'][h][n]['query_point']
    print('T=%d eps=%g: smallest gain before the clamp at 0: %.3e; %d states with a gain to be had, the frame of maximal gain is another '
          'than the frame of most information in %d of them' % (T, eps, raw_min, gained, elsewhere))
    assert raw_min >= -1e-12                                            # gain >= 0 is a theorem: the candidates are not restricted
    assert elsewhere > 0 or T == 2


@pytest.mark.parametrize('T,eps', CASES)
def test_reference_states_compared_by_index(T, eps):
    c = NR.gain_case(T, eps)
    counts = tuple(sum(NR.by_index(c['gref'][h][n]) for n in NR.ROWS[T]) for h in NR.HISTORIES)
    gained = sum(c['gref'][h][n]['ask_gain'] > 1e-9 for h in NR.HISTORIES for n in NR.ROWS[T])
    print('T=%d eps=%g: states compared by index per history %s, %d of the %d with a gain' % (T, eps, counts, sum(counts), gained))
    assert (counts, gained) == BY_INDEX[(T, eps)]
    assert gained - sum(counts) <= gained / 4                           # at most a quarter of the states with any gain is left out


def test_reference_candidate_list_and_poisoned_row():
    c = NR.tilted_case(33, 0.2)
    ps, pe, v = c['pst'][3][0], c['pet'][3][0], int(c['v'][0])
    full = NR.noisy_gain_ref(ps, pe, v, 0.2)
    part = NR.noisy_gain_ref(ps, pe, v, 0.2, frames=[14, -1, 3, 40, 12])
    assert part['frames'] == [14, 3, 12] and part['value'] == full['value']
    assert all(part['gain'][t] == full['gain'][t] for t in (14, 3, 12)) and part['gain'].sum() == full['gain'][[14, 3, 12]].sum()
    assert part['ask_point'] == max((14, 3, 12), key=lambda t: full['gain'][t])
    none = NR.noisy_gain_ref(ps, pe, v, 0.2, frames=[-1, v])
    assert none['ask_point'] == -1 and none['ask_gain'] == 0.0 and none['value'] == full['value']
    bad = NR.noisy_gain_ref(ps, pe, v, 0.2, nan_logit=True)
    assert bad['status'] == NR.POISONED and bad['ask_point'] == -1 and bad['ask_gain'] == bad['value'] == -1.0


def test_tilt_restatement_edges():
    s = np.array([[0.5, -0.0, 2.0, 7.0, 1.0]], dtype=np.float32)
    e = np.array([[-0.0, 1.5, -3.0, 7.0, 2.0]], dtype=np.float32)
    aps = [[(1, True), (1, True), (2, False), (9, True), (-1, False), (3, True)]]      # a duplicate, two points outside the clip, one at t >= v
    g = NR.counts(3, aps[0])
    assert list(g) == [0, 0, 2, 1]
    lam = NR.lam32(0.2)
    assert lam.dtype == np.float32 and abs(float(lam) - np.log(4.0)) < 1e-6
    s_t, e_t = NR.tilt_set(s, e, [3], [4], aps, 0.2)
    assert (s_t[0, 3:].view(np.int32) == s[0, 3:].view(np.int32)).all() and (e_t[0, 3:].view(np.int32) == e[0, 3:].view(np.int32)).all()
    assert s_t[0, 0] == s[0, 0] and np.signbit(s_t[0, 1]) and s_t[0, 2] == np.float32(2.0) - np.float32(2.0) * lam
    assert np.signbit(e_t[0, 0]) and e_t[0, 1] == np.float32(1.5) + np.float32(2.0) * lam and e_t[0, 2] == np.float32(-3.0) + lam
    for out, src in zip(NR.tilt_set(s, e, [3], [4], aps, 0.5), (s, e)):        # eps = 0.5: the input bits
        assert (out.view(np.int32) == src.view(np.int32)).all()
    # 64 answers at eps = 1e-6: the direct evidence is finite, far below what float64 holds as a plain product
    c = Q.case(33)
    many = NR.many_answers(33)
    d = NR.direct(c['ps'][0], c['pe'][0], 33, many, 1e-6)
    assert np.isfinite(d['log_evidence']) and d['log_evidence'] < -100.0 and len(many) == 64


def test_hard_rule_breaks_on_the_round_set():
    """the synthetic label-update set of the GPU test: whenever the question lands inside the hull of the earlier answers, the erring
    annotator of the seed contradicts them under the hard rule"""
    S_ = NR.round_set()
    flips = NR.annotator_flips()
    mid = np.array([(a + b) // 2 for a, b in S_['gt']])
    broken = NR.replay_hard_rounds([mid] * NR.ROUNDS, flips)
    assert [len(b) for b in broken] == [int(flips[0][S_['sel']].sum()), int((flips[0] | flips[1])[S_['sel']].sum()),
                                        int((flips[0] | flips[1] | flips[2])[S_['sel']].sum())]
    assert len(broken[0]) >= 1 and len(S_['sel']) == 16
    assert NR.replay_hard_rounds([mid] * NR.ROUNDS, [np.zeros(NR.ROUND_N, dtype=bool)] * NR.ROUNDS) == [[], [], []]
