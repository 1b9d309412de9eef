"""Reference of hual_kcenter_greedy (include/hual_seqpan.h) for the tests: the contract restated in float64 numpy, the keys (score, w,
-i) included.  State is the selection after some centers - the init rows in their order, then picks - and answers what the next
step sees; greedy() runs it freely, and a test that hands State the kernel's own earlier picks gets every row's reference score at
the next step (teacher forcing)."""
import itertools

import numpy as np


class State:
    def __init__(self, x, weight=None, init=()):
        self.x = np.asarray(x, dtype=np.float64)
        self.N = self.x.shape[0]
        self.w = np.ones(self.N) if weight is None else np.asarray(weight, dtype=np.float64)
        self.finite = np.isfinite(self.x).all(axis=1)            # d(i, i) == 0: a row with a NaN or an infinity is never eligible
        self.mind = np.full(self.N, np.inf)
        self.assign = np.full(self.N, -1, dtype=np.int64)
        self.taken = np.zeros(self.N, dtype=bool)
        self.centers = []
        for c in init:
            self.add(int(c))

    def distance(self, c):
        with np.errstate(invalid='ignore', over='ignore'):
            return ((self.x - self.x[c]) ** 2).sum(axis=1)

    def add(self, c):
        """row c becomes a center; an index outside [0, N) - the -1 of an exhausted selection - changes nothing"""
        if not 0 <= c < self.N:
            return
        d = self.distance(c)
        with np.errstate(invalid='ignore'):
            closer = d < self.mind                               # strictly smaller replaces: the first center that attains the minimum stays
        self.assign[closer] = c
        self.mind = np.where(closer | np.isnan(d), d, self.mind)
        self.taken[c] = True
        self.centers.append(c)

    def scores(self):
        """-> (score of every row at the next step, eligible)"""
        with np.errstate(invalid='ignore'):
            score = self.w * self.mind if self.centers else self.w.copy()
            eligible = ~self.taken & self.finite & (self.w >= 0) & ~np.isnan(score)
        return score, eligible

    def best(self):
        """-> (the eligible row of maximal (score, w, -i), its mind before the pick) or (-1, -1.0)"""
        score, eligible = self.scores()
        idx = np.flatnonzero(eligible)
        if not len(idx):
            return -1, -1.0
        top = idx[np.lexsort((idx, -self.w[idx], -score[idx]))[0]]
        return int(top), float(self.mind[top])


def greedy(x, n_select, weight=None, init=(), snapshots=()):
    """-> dict(picked int64 [n_select], pick_dist float64 [n_select], mind, assign: the state after every center, and state[k] =
    (mind, assign) after the first k picks for k in snapshots)"""
    st = State(x, weight, init)
    picked, dist, snaps = [], [], {}
    if 0 in snapshots:
        snaps[0] = (st.mind.copy(), st.assign.copy())
    for s in range(n_select):
        i, d = st.best()
        picked.append(i)
        dist.append(d)
        st.add(i)
        if s + 1 in snapshots:
            snaps[s + 1] = (st.mind.copy(), st.assign.copy())
    return dict(picked=np.array(picked, dtype=np.int64), pick_dist=np.array(dist, dtype=np.float64), mind=st.mind, assign=st.assign, state=snaps)


def cover_radius(x, centers):
    """max_i min_c |x_i - x_c| (the distance, not its square)"""
    x = np.asarray(x, dtype=np.float64)
    d = np.sqrt(((x[:, None, :] - x[None, list(centers), :]) ** 2).sum(-1))
    return float(d.min(axis=1).max())


def optimal_radius(x, k):
    """the best covering radius of k centers chosen among the rows, by brute force"""
    return min(cover_radius(x, c) for c in itertools.combinations(range(len(x)), k))
