"""Reference of hual_al_session (include/hual_seqpan.h) for the tests: the contract as a plain Python loop in float64, built on
al_query_ref.posterior_ref (the brute-force posterior) and, under a noisy annotator, on al_noisy_ref.tilt_row (the float32 tilt,
operation by operation).

One step = `step(...)`: the posterior on the list so far.  One decision = `decide(...)`: the stop conditions in the contract's order.
`session(...)` loops the two; the GPU test calls them one at a time on the device's own list (teacher forcing).  Also here: the seeded
settings the CPU and GPU tests share, and the (row, step) pairs whose decision lies too close to a threshold to be compared."""
import functools

import numpy as np

import al_noisy_ref as NZ
import al_query_ref as Q

BUDGET, ENTROPY, GAIN, CONTRADICTORY, POISONED, OVERFLOW = range(6)      # HUAL_AL_STOP_*
MAX_Q, MAX_POINTS = 16, 64
NEAR = 1e-3                   # bits: a decision whose entropy / gain lies this close to its threshold is not compared
STARTS = (0, 3, 'flipped3')   # the lists a session starts from: al_query_ref's histories 0 and 3, al_noisy_ref's history 3 (the same
                              # three answers flipped at rate 0.3 after the fact: some rows are contradictory before the first question)
EPS = (0.0, 0.05, 0.2)        # 0: the hard rule
FLIP_RATE, FLIP_SEED = 0.3, 9300
# the thresholds of the teacher-forced comparison: a collapsed posterior (gain 0) is 0.02 bits away from min_gain, so it is compared
STOP_ENTROPY, MIN_GAIN = 1.0, 0.02


# the settings of the teacher-forced GPU comparison, (start, eps, flipped): Q = 6, STOP_ENTROPY, MIN_GAIN.  The flipped masks leave 70 %
# of the answers truthful, so only the first list is also run without them
TEACHER_GRID = tuple((st, eps, True) for st in STARTS for eps in EPS) + tuple((0, eps, False) for eps in EPS)


def step(s0, e0, v, aps, eps=0.0, nan_logit=False):
    """the posterior one step of a session reads: al_query_ref.posterior_ref of the row's probabilities on the list `aps` (eps == 0), or
    of the probabilities of the rows tilted by the whole list, with no active point (eps > 0).  s0 / e0: the row's float32 logits"""
    if v < 1 or nan_logit:
        return Q.posterior_ref(None, None, v, aps, nan_logit=True)
    ps, pe = NZ.probabilities(s0, e0, v)
    if eps == 0.0:
        return Q.posterior_ref(ps, pe, v, aps)
    Z = Q.weights(ps, pe, v)[0].sum()
    if not (Z > 0 and np.isfinite(Z)):                                # hual_al_noisy_tilt's gate: raw copies, which poison again
        return Q.posterior_ref(ps, pe, v, [])
    s_t, e_t = NZ.tilt_row(s0, e0, v, aps, eps)
    if np.isnan(s_t).any() or np.isnan(e_t).any():
        return Q.posterior_ref(None, None, v, [], nan_logit=True)
    pst, pet = NZ.probabilities(s_t, e_t, v)
    return Q.posterior_ref(pst, pet, v, [])


def decide(post, k, cap, stop_entropy=-1.0, min_gain=0.0):
    """the stop conditions in the contract's order -> the reason, or None: ask"""
    if post['status'] == Q.POISONED:
        return POISONED
    if post['status'] == Q.CONTRADICTORY:
        return CONTRADICTORY
    if stop_entropy >= 0 and post['post_entropy'] <= stop_entropy:
        return ENTROPY
    if not post['query_gain'] > min_gain:
        return GAIN
    if k >= cap:
        return BUDGET
    return None


def near_threshold(post, stop_entropy, min_gain):
    """is this step's decision within NEAR of a threshold (the GPU test skips it)"""
    if post['status'] != Q.LIVE:
        return False
    return (stop_entropy >= 0 and abs(post['post_entropy'] - stop_entropy) <= NEAR) or abs(post['query_gain'] - min_gain) <= NEAR


def session(s0, e0, v, aps, gt, qmax, budget=None, stop_entropy=-1.0, min_gain=0.0, eps=0.0, flip=0, nan_logit=False, stepper=None):
    """one sample's session -> dict(asked, answer, q_asked, gain: lists of n_asked entries; entropy: n_asked + 1 entries (-1 where the
    step is not live), n_asked, stop_reason, aps: the list afterwards, posts: every step's posterior).  stepper(aps): `step` of this
    row by other means (a cache)"""
    assert 1 <= qmax <= MAX_Q
    cap = qmax if budget is None else min(max(int(budget), 0), qmax)
    out = dict(asked=[], answer=[], q_asked=[], gain=[], entropy=[], posts=[], aps=list(aps))
    if len(aps) + cap > MAX_POINTS:
        return dict(out, n_asked=0, stop_reason=OVERFLOW)
    k = 0
    while True:
        post = stepper(out['aps']) if stepper else step(s0, e0, v, out['aps'], eps, nan_logit)
        out['posts'].append(post)
        out['entropy'].append(post['post_entropy'] if post['status'] == Q.LIVE else -1.0)
        why = decide(post, k, cap, stop_entropy, min_gain)
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


def flip_masks(T, rate=FLIP_RATE, seed=FLIP_SEED):
    """uint32 [16]: the seeded flip mask of case T, MAX_Q draws per row in row order"""
    rng = np.random.default_rng(seed + T)
    m = np.zeros(Q.N_ROWS, dtype=np.uint32)
    for n in range(Q.N_ROWS):
        for k in range(MAX_Q):
            if rng.random() < rate:
                m[n] |= np.uint32(1 << k)
    return m


@functools.lru_cache(maxsize=None)
def start_list(T, start):
    """per row the list of (frame, is_pos) a session of case T starts from"""
    return NZ.case(T)['naps'][3] if start == 'flipped3' else Q.case(T)['aps'][start]


@functools.lru_cache(maxsize=None)
def case_step(T, n, aps, eps):
    """step() of row n of al_query_ref.case(T) on the list `aps` (a tuple of (frame, is_pos)), computed once"""
    c = Q.case(T)
    return step(c['s'][n].numpy(), c['e'][n].numpy(), int(c['v'][n]), list(aps), eps)


@functools.lru_cache(maxsize=None)
def sessions(T, start, eps, flipped, qmax, stop_entropy=-1.0, min_gain=0.0):
    """the reference sessions of the 16 rows of al_query_ref.case(T) from the lists `start` names: a list of session() dicts"""
    c, lists = Q.case(T), start_list(T, start)
    fm = flip_masks(T) if flipped else np.zeros(Q.N_ROWS, dtype=np.uint32)
    return [session(None, None, int(c['v'][n]), lists[n], c['gt'][n], qmax, None, stop_entropy, min_gain, eps, int(fm[n]),
                    stepper=lambda aps, n=n: case_step(T, n, tuple(aps), eps))
            for n in range(Q.N_ROWS)]
