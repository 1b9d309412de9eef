"""Reference of hual_al_design (include/hual_seqpan.h) for the tests: the contract restated in float64 on the CPU, by enumeration, on
al_query_ref's `weights` / `consistent`.

A design D = (t_1, ..., t_m) is a set of frames asked together.  The answer at t_k is [i <= t_k <= j], a function of the span, so the
information D carries about the span is the entropy of its answer vector: every span of the consistent set A gets its answer
bit-pattern, the masses of equal patterns are grouped with bincount, and I(D) is the entropy of the groups.  No prefix sum, no cell
sum and no chain rule anywhere, so the kernel's factorisation into per-cell sums is checked against the definition itself.

`greedy` restates the launch's loop: the forced prefix, then the first frame of maximal I(D + t) until a stop rule holds; it also
returns, per step, every candidate's I(D + t) - what the GPU test evaluates the kernel's own frame by.  `adaptive_tree` is the
expected information of the adaptive greedy policy of the same depth (hual_al_session's, answered by the posterior itself), for the
adaptivity gap the README records."""
import functools

import numpy as np

import al_query_ref as Q

BUDGET, ENTROPY, GAIN, CONTRADICTORY, POISONED = range(5)     # HUAL_AL_STOP_*
MAX_M = 16
NEAR = 1e-5                   # bits: the family's near-tie threshold


class Row:
    """one sample's posterior opened for designs: the weights of A as a flat vector with every span's (i, j)"""

    def __init__(self, ps, pe, v, aps, nan_logit=False):
        self.v, self.aps = int(v), list(aps)
        self.post = Q.posterior_ref(ps, pe, v, aps, nan_logit=nan_logit)
        self.status = self.post['status']
        if self.status != Q.LIVE:
            return
        W, _ = Q.weights(ps, pe, v)
        ok = Q.consistent(v, aps)
        ii, jj = np.indices((v, v))
        self.w, self.i, self.j = W[ok], ii[ok], jj[ok]
        self.ZA = self.w.sum()
        self.H = self.post['post_entropy']
        self.answered = set(f for f, _ in aps if 0 <= f < v)

    def groups(self, D):
        """(group id of every span of A, number of groups) under the answer vector of the frames D (those outside [0, v) ignored)"""
        g = np.zeros(len(self.w), dtype=np.int64)
        n = 1
        for t in D:
            if not 0 <= t < self.v:
                continue
            _, g = np.unique(g * 2 + ((self.i <= t) & (t <= self.j)), return_inverse=True)
            n = int(g.max()) + 1 if len(g) else 1
        return g, n

    def entropy_of(self, ids, n):
        m = np.bincount(ids, weights=self.w, minlength=n)
        p = m[m > 0] / self.ZA
        return float(-(p * np.log2(p)).sum())

    def info(self, D):
        """I(D) in bits"""
        g, n = self.groups(D)
        return self.entropy_of(g, n)

    def candidates(self, D):
        """I(D + t) for every t < v, float64 [v]"""
        g, n = self.groups(D)
        out = np.empty(self.v)
        for t in range(self.v):
            out[t] = self.entropy_of(g * 2 + ((self.i <= t) & (t <= self.j)), 2 * n)
        return out

    def outcomes(self, D):
        """[(P(o), the answers of outcome o as (frame, is_pos) in D's order)] over the outcomes of positive mass"""
        D = [t for t in D if 0 <= t < self.v]
        g, n = self.groups(D)
        m = np.bincount(g, weights=self.w, minlength=n)
        out = []
        for o in range(n):
            if m[o] > 0:
                k = int(np.flatnonzero(g == o)[0])
                out.append((m[o] / self.ZA, [(t, bool(self.i[k] <= t <= self.j[k])) for t in D]))
        return out


def greedy(row, mmax, forced=(), min_gain=0.0, stop_entropy=-1.0):
    """the launch's loop on one Row -> dict(frames, info: lists of n_design entries; n_design, stop_reason, post_entropy, and per step
    that was decided greedily: cand (I(D + t) of every t), base (I(D)), best (the best marginal gain), keyed by the step)"""
    assert 1 <= mmax <= MAX_M
    out = dict(frames=[], info=[], cand={}, base={}, best={}, post_entropy=-1.0)
    if row.status != Q.LIVE:
        return dict(out, n_design=0, stop_reason=POISONED if row.status == Q.POISONED else CONTRADICTORY)
    out['post_entropy'] = row.H
    forced = [int(f) for f in forced]
    cur = 0.0
    while True:
        m = len(out['frames'])
        if m >= mmax:
            return dict(out, n_design=m, stop_reason=BUDGET)
        while forced and forced[0] >= row.v:                          # outside the clip: ignored
            forced.pop(0)
        if forced and forced[0] < 0:                                  # -1 ends the forced prefix
            forced = []
        if forced:
            t = forced.pop(0)
            cur = row.info(out['frames'] + [t])
        else:
            if stop_entropy >= 0 and row.H - cur <= stop_entropy:
                return dict(out, n_design=m, stop_reason=ENTROPY)
            cand = row.candidates(out['frames'])
            t = int(np.argmax(cand))                                  # the first maximal frame
            out['cand'][m], out['base'][m], out['best'][m] = cand, cur, float(cand[t] - cur)
            if not cand[t] - cur > min_gain:
                return dict(out, n_design=m, stop_reason=GAIN)
            cur = float(cand[t])
        out['frames'].append(t)
        out['info'].append(cur)


def adaptive_tree(row, depth):
    """the expected information, in bits, of `depth` adaptive greedy questions (each the first frame of maximal h2(q) under the
    posterior given the answers so far), the answers drawn from the posterior itself"""
    def walk(aps, d):
        if d == 0:
            return 0.0
        p = Q.posterior_ref(row_ps, row_pe, row.v, aps)
        if p['status'] != Q.LIVE or not p['query_gain'] > 0:
            return 0.0
        t, q = p['query_point'], float(p['incl'][p['query_point']])
        return p['query_gain'] + q * walk(aps + [(t, True)], d - 1) + (1.0 - q) * walk(aps + [(t, False)], d - 1)
    row_ps, row_pe = row.ps_pe
    return walk(list(row.aps), depth)


@functools.lru_cache(maxsize=None)
def case_row(T, h, n):
    """Row of sample n of al_query_ref.case(T) after h answers"""
    c = Q.case(T)
    r = Row(c['ps'][n], c['pe'][n], int(c['v'][n]), c['aps'][h][n])
    r.ps_pe = (c['ps'][n], c['pe'][n])
    return r


def rows_of(T):
    """the rows of case(T) the tests run: all 16, every fourth at T = 256 (the enumeration costs 0.1 s per row and step there)"""
    return range(0, Q.N_ROWS, 4) if T >= 256 else range(Q.N_ROWS)


@functools.lru_cache(maxsize=None)
def case_design(T, h, n, mmax, min_gain=0.0):
    """greedy(case_row(T, h, n), mmax), computed once"""
    return greedy(case_row(T, h, n), mmax, min_gain=min_gain)
