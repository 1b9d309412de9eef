"""Reference of hual_al_session_label (include/hual_seqpan.h) for the tests: the contract as a plain Python loop in float64.  It has
no interval, prefix sum or factorisation of its own - per pass it calls
  al_session_ref.step            the posterior on the list so far and the frame to ask,
  al_label_ref.label_ref         the minimum-Bayes-risk label by enumeration,
  al_hit_ref.state / cand_prob   the label's hit probability by enumeration,
the last two on the probabilities the pass reads: the row's own with the list (eps == 0), or those of the rows tilted by the whole
list with no active point (eps > 0).

`decide` is al_session_ref.decide with the new rule in its place, `near_threshold` al_session_ref.near_threshold extended by the hit
probability.  `session` loops; the GPU test calls `pass_ref` one pass at a time on the device's own list (teacher forcing)."""
import functools

import numpy as np

import al_hit_ref as HL
import al_label_ref as L
import al_noisy_ref as NZ
import al_query_ref as Q
import al_session_ref as S

RELIABLE = 6                                  # HUAL_AL_STOP_RELIABLE
THR = tuple(HL.THR3)                          # 3/10, 1/2, 7/10: al.HIT_IOUS as exact rationals
NEAR_HIT = 1e-3                               # a decision whose hit probability lies this close to stop_hit is not compared
MARGIN = 1e-5                                 # a label whose runner-up lies closer than this may differ on the device
# the rules the documents quote and the tests run: (stop_hit, index into THR)
RULES = ((0.9, 2), (0.9, 1), (0.75, 2))
# (start list, eps, flipped) of the settings quoted in the issue: eps 0 without flips, eps 0.05 with the seeded flips
SETTINGS = tuple((st, eps, fl) for st in (0, 3) for eps, fl in ((0.0, False), (0.05, True)))


def read_probs(s0, e0, v, aps, eps=0.0, nan_logit=False):
    """the probabilities a pass reads and the list it reads them with -> (ps, pe, aps_read), or None where al_session_ref.step finds
    the row poisoned before it has probabilities"""
    if v < 1 or nan_logit:
        return None
    ps, pe = NZ.probabilities(s0, e0, v)
    if eps == 0.0:
        return ps, pe, list(aps)
    Z = Q.weights(ps, pe, v)[0].sum()
    if not (Z > 0 and np.isfinite(Z)):
        return ps, pe, []
    s_t, e_t = NZ.tilt_row(s0, e0, v, aps, eps)
    if np.isnan(s_t).any() or np.isnan(e_t).any():
        return None
    pst, pet = NZ.probabilities(s_t, e_t, v)
    return pst, pet, []


def pass_ref(s0, e0, v, aps, eps=0.0, thr=THR, nan_logit=False):
    """one pass: dict(post = al_session_ref.step's posterior, label = al_label_ref.label_ref's dict, hit = float64 [M] the label's hit
    probability, hit_state = the al_hit_ref state - for scoring another span under the same posterior); label / hit None and -1 on a
    pass that is not live"""
    post = S.step(s0, e0, v, aps, eps, nan_logit)
    out = dict(post=post, label=None, hit=np.full(len(thr), -1.0), hit_state=None)
    if post['status'] != Q.LIVE:
        return out
    ps, pe, read = read_probs(s0, e0, v, aps, eps, nan_logit)
    out['label'] = L.label_ref(ps, pe, v, read)
    assert out['label']['status'] == Q.LIVE and out['label']['full']
    out['hit_state'] = HL.state(ps, pe, v, read)
    out['hit'] = HL.cand_prob(out['hit_state'], [out['label']['label']], list(thr))[0]
    return out


def decide(p, k, cap, stop_hit=-1.0, stop_m=0, stop_entropy=-1.0, min_gain=0.0):
    """the stop conditions in the contract's order -> the reason, or None: ask.  p: pass_ref's dict"""
    post = p['post']
    if post['status'] == Q.POISONED:
        return S.POISONED
    if post['status'] == Q.CONTRADICTORY:
        return S.CONTRADICTORY
    if stop_hit >= 0 and p['hit'][stop_m] >= stop_hit:
        return RELIABLE
    return S.decide(post, k, cap, stop_entropy, min_gain)


def near_threshold(p, stop_hit=-1.0, stop_m=0, stop_entropy=-1.0, min_gain=0.0):
    """is this pass's decision within reach of a threshold (the GPU test skips it)"""
    if p['post']['status'] != Q.LIVE:
        return False
    if stop_hit >= 0 and abs(p['hit'][stop_m] - stop_hit) <= NEAR_HIT:
        return True
    if stop_hit >= 0 and p['hit'][stop_m] >= stop_hit:                # reliable by more than that: the rules in bits are not reached
        return False
    return S.near_threshold(p['post'], stop_entropy, min_gain)


def session(s0, e0, v, aps, gt, qmax, budget=None, stop_hit=-1.0, stop_m=0, stop_entropy=-1.0, min_gain=0.0, eps=0.0, flip=0, thr=THR,
            nan_logit=False, passer=None):
    """one sample's session -> al_session_ref.session's dict (posts: the passes' posteriors) plus passes (pass_ref's dicts), label,
    label_conf, label_hit: n_asked + 1 entries each, (-1, -1) / -1 where the pass is not live.  passer(aps): pass_ref of this row by
    other means (a cache)"""
    assert 1 <= qmax <= S.MAX_Q
    cap = qmax if budget is None else min(max(int(budget), 0), qmax)
    out = dict(asked=[], answer=[], q_asked=[], gain=[], entropy=[], posts=[], passes=[], label=[], label_conf=[], label_hit=[], aps=list(aps))
    if len(aps) + cap > S.MAX_POINTS:
        return dict(out, n_asked=0, stop_reason=S.OVERFLOW)
    k = 0
    while True:
        p = passer(out['aps']) if passer else pass_ref(s0, e0, v, out['aps'], eps, thr, nan_logit)
        post, live = p['post'], p['post']['status'] == Q.LIVE
        out['passes'].append(p)
        out['posts'].append(post)
        out['entropy'].append(post['post_entropy'] if live else -1.0)
        out['label'].append(p['label']['label'] if live else (-1, -1))
        out['label_conf'].append(p['label']['conf'] if live else -1.0)
        out['label_hit'].append(p['hit'])
        why = decide(p, k, cap, stop_hit, stop_m, stop_entropy, min_gain)
        if why is not None:
            return dict(out, n_asked=k, stop_reason=why)
        t = post['query_point']
        ans = Q.answer(gt, t) != bool((int(flip) >> k) & 1)
        out['asked'].append(t)
        out['answer'].append(ans)
        out['q_asked'].append(float(post['incl'][t]))
        out['gain'].append(post['query_gain'])
        out['aps'] = out['aps'] + [(t, ans)]
        k += 1


@functools.lru_cache(maxsize=None)
def case_pass(T, n, aps, eps):
    """pass_ref of row n of al_query_ref.case(T) on the list `aps` (a tuple of (frame, is_pos)), computed once"""
    c = Q.case(T)
    return pass_ref(c['s'][n].numpy(), c['e'][n].numpy(), int(c['v'][n]), list(aps), eps)


@functools.lru_cache(maxsize=None)
def sessions(T, start, eps, flipped, qmax, stop_hit=-1.0, stop_m=0, stop_entropy=-1.0, min_gain=0.0):
    """the reference sessions of the 16 rows of al_query_ref.case(T) from the lists `start` names: a list of session() dicts"""
    c, lists = Q.case(T), S.start_list(T, start)
    fm = S.flip_masks(T) if flipped else np.zeros(Q.N_ROWS, dtype=np.uint32)
    return [session(None, None, int(c['v'][n]), lists[n], c['gt'][n], qmax, None, stop_hit, stop_m, stop_entropy, min_gain, eps, int(fm[n]),
                    passer=lambda aps, n=n: case_pass(T, n, tuple(aps), eps))
            for n in range(Q.N_ROWS)]
