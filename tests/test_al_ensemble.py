"""CPU: the identities of the ensemble span posterior on its float64 enumeration (tests/al_ens_ref.py) - no GPU, no library - and the
host-side plumbing around it (McBank's passes argument, the validation of al.update_labels(posterior=)).

What the enumeration has to satisfy on its own before a kernel is held against it:
  - K identical passes are one pass: the weights are 1 / K and every output is al_query_ref's / the K = 1 value;
  - the weights sum to 1; span_bald (before its clamp) is >= -1e-12 - Jensen, up to the rounding of two float64 sums of <= 32,896
    terms - and exactly 0 for identical passes at every K: the enumeration takes passes whose factor rows are equal bit for bit as
    ONE component with the correctly rounded sum of their weights, which is 1.0 at every K <= 16, so the mixture is the pass itself;
    (this is an identity of the ENUMERATION: the kernels sum the passes one by one and are held to exactness at K = 1 only -
    tests/test_gpu_al_ensemble.py -, their K > 1 cases never hold two equal passes, and span_bald there is within the 5e-5 bar;)
  - under an annotator who errs, "tilt every pass (hual_al_noisy_tilt's float32 arithmetic), weight it by its own log_evidence" is the
    direct product of per-answer likelihoods within 1e-6 on every span probability - the family's figure for the single-pass form;
  - the index conditions of tests/test_gpu_al_ensemble.py hold on the reference alone for the seeded cases: at most 10 % of a case's
    live rows have a runner-up within 1e-5 bits (the question) or 1e-9 tIoU (the label) of the best."""
import numpy as np
import pytest

import al_ens_ref as E
import al_noisy_ref as NZ
import al_query_ref as Q


def _rows(T, h, rows=(0, 3, 9, 12)):
    c = Q.case(T)
    return [(n, c['ps'][n], c['pe'][n], int(c['v'][n]), c['aps'][h][n], c['ref'][h][n]) for n in rows]


@pytest.mark.parametrize('K', [1, 2, 3, 4, 5, 16])
@pytest.mark.parametrize('T,h', [(33, 0), (33, 3), (70, 6)])
def test_identical_passes_are_one_pass(T, h, K):
    worst = 0.0
    for n, ps, pe, v, aps, det in _rows(T, h):
        one = E.ensemble_ref([ps], [pe], v, aps, old=(0, v - 1))
        r = E.ensemble_ref([ps] * K, [pe] * K, v, aps, old=(0, v - 1))
        assert r['status'] == det['status'] == E.LIVE
        assert np.abs(r['weight'] - 1.0 / K).max() <= 1e-15
        assert np.abs(r['incl'] - det['incl']).max() <= 1e-12 and abs(r['post_entropy'] - det['post_entropy']) <= 1e-10
        assert abs(r['expected_entropy'] - det['post_entropy']) <= 1e-10 and abs(r['log_evidence'] - np.log(det['agree'])) <= 1e-12
        assert r['query_point'] == det['query_point'] and r['new_idx'] == one['new_idx']
        assert np.abs(r['y_start'] - one['y_start']).max() <= 1e-14 and abs(r['conf'] - one['conf']) <= 1e-14
        assert abs(r['old_conf'] - one['old_conf']) <= 1e-14
        assert r['bald_raw'] == 0.0 and r['span_bald'] == 0.0
        worst = max(worst, abs(r['bald_raw']))
    print('T=%d answers=%d K=%d: max |span_bald| of identical passes %.2e' % (T, h, K, worst))


@pytest.mark.parametrize('cs', E.CASES)
def test_case_identities_and_index_conditions(cs):
    c = E.case(*cs)
    live = [r for r in c['ref'] if r['status'] == E.LIVE]
    assert len(live) == E.N_ROWS
    for r in live:
        assert abs(r['weight'].sum() - 1.0) <= 1e-14 and (r['weight'] >= 0).all()
        assert r['bald_raw'] >= -1e-12
        assert abs(r['P'].sum() - 1.0) <= 1e-12 and abs(r['y_start'].sum() - 1.0) <= 1e-12 and abs(r['y_end'].sum() - 1.0) <= 1e-12
        assert r['span_bald'] <= np.log2(c['K']) + 1e-12               # the mask holds at most log2 K bits
    ex_q = E.excused(c['ref'], 'query_gain', 'runner_gain', 1e-5)
    ex_l = E.excused(c['ref'], 'conf', 'runner_conf', 1e-9)
    labelled = sum('members' in r for r in live)
    print('%s: %d live rows, %d labelled; excused by index: question %s, label %s; span_bald up to %.3f bits'
          % (cs, len(live), labelled, ex_q, ex_l, max(r['span_bald'] for r in live)))
    assert 10 * len(ex_q) <= len(live) and 10 * len(ex_l) <= len(live) and labelled == E.N_ROWS
    if c['K'] > 1 and c['T'] > 2:
        assert max(r['span_bald'] for r in live) > 1e-3                # the passes differ: the score is not idle


@pytest.mark.parametrize('T,K,h', [(33, 5, 3), (70, 2, 6), (33, 16, 1)])
def test_tilt_each_pass_and_weight_by_its_evidence_is_the_direct_product(T, K, h):
    eps = E.NOISE_EPS
    c = E.case(T, K, h, eps, False, 0)
    worst = worst_w = 0.0
    for n in range(E.N_ROWS):
        v, aps, ref = c['v'][n], c['aps'][n], c['ref'][n]
        lev, Pk = [], []
        for k in range(K):
            s_t, e_t = NZ.tilt_row(c['pass_s'][k, n].numpy(), c['pass_e'][k, n].numpy(), v, aps, eps)
            pst, pet = NZ.probabilities(s_t, e_t, v)
            Pk.append(NZ.tilted(pst, pet, v))
            lev.append(float(np.float32(NZ.direct(c['ps'][k][n], c['pe'][k][n], v, aps, eps)['log_evidence'])))      # as the launch stores it
        u = np.array(lev)
        w = np.exp(u - u.max())
        w /= w.sum()
        P = sum(w[k] * Pk[k] for k in range(K))
        worst = max(worst, np.abs(P - ref['P']).max())
        worst_w = max(worst_w, np.abs(w - ref['weight']).max())
    print('T=%d K=%d answers=%d eps=%.1f: tilted-and-weighted against the direct product: max |P| %.2e, max |weight| %.2e (bar 1e-6)'
          % (T, K, h, eps, worst, worst_w))
    assert worst <= 1e-6 and worst_w <= 1e-6


def test_ensemble_and_deterministic_pass_disagree_somewhere():
    states, dq, dl = E.disagreement()
    print('of %d random row-states (T = 33, K = 8, sigma = %.1f) the ensemble asks about another frame in %d and gives another label in %d'
          % (states, E.PASS_SIGMA, dq, dl))
    assert states > 40 and dq + dl > 0


class _Bank:
    def __init__(self, K, Kmax):
        self.K, self.Kmax = K, Kmax
        self.pass_s = object() if Kmax else None


def test_host_side_plumbing():
    from hual_amd import al, lib
    assert al.check_passes(None) == 0 and al.check_passes(1) == 1 and al.check_passes(16) == 16
    for bad in (0, 17, 2.5, True, 'x'):
        with pytest.raises(ValueError):
            al.check_passes(bad)
    al.check_part_passes({'pass_s': np.zeros((3, 2, 4))}, 3)
    al.check_part_passes({}, 0)
    for part, kmax in (({'pass_s': np.zeros((3, 2, 4))}, 0), ({}, 3), ({'pass_s': np.zeros((2, 2, 4))}, 3)):
        with pytest.raises(lib.HualError):
            al.check_part_passes(part, kmax)
    al.check_bank_planes(_Bank(3, 4))
    al.check_bank_planes(_Bank(3, 4), 2)
    for bank, K in ((_Bank(3, 0), None), (_Bank(0, 4), None), (_Bank(3, 4), 4), (_Bank(3, 4), 0), (None, None)):
        with pytest.raises(ValueError):
            al.check_bank_planes(bank, K)
    ok = dict(posterior='ensemble', bank=_Bank(3, 3), mc_samples=None, rank_by='uncert_video', observe_by='info_gain', renew_by='heuristic',
              acquire_by=None, soft_out=None, questions_per_clip=1, calibrate=None)
    al.check_round(**ok)
    al.check_round(**dict(ok, observe_by='uncert_frame', rank_by='span_bald'))
    al.check_round(**dict(ok, posterior='deterministic', bank=None))
    for bad in (dict(posterior='both'), dict(bank=None), dict(bank=_Bank(3, 0)), dict(acquire_by='label_gain'), dict(questions_per_clip=2),
                dict(calibrate='evidence'), dict(observe_by='uncert_frame'), dict(mc_samples=4),
                dict(posterior='deterministic', rank_by='span_bald')):
        with pytest.raises(ValueError):
            al.check_round(**dict(ok, **bad))
    assert al.RANK_BY_ENSEMBLE == ('span_bald',) and al.POSTERIOR == ('deterministic', 'ensemble')
