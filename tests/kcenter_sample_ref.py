"""Reference of hual_kcenter_sample (include/hual_seqpan.h) for the tests: the contract restated in float64 numpy - the k-center
state with an optional origin center, and the score (w * mind) / E under the unit exponentials E(i, s) of Philox4x32-7 (oracle/philox.py
gives the words).  State answers what the next step sees; run() walks it freely, and a test that hands State the kernel's own earlier
picks gets every row's reference score at the next step (teacher forcing)."""
import numpy as np

from oracle.philox import philox4x32

SITE_SELECT = 256        # include/hual_seqpan.h HUAL_SITE_SELECT


def exponentials(seed, offset, s, N):
    """E(i, s) for i in range(N): float32(-ln((k + 0.5) 2^-24)), the logarithm in float64, k the top 24 bits of word x of the call
    (c0 = s, c1 = i, c2 = SITE_SELECT, c3 = offset) under the key (seed low, seed high) -> float64 [N] holding float32 values"""
    words = philox4x32(np.uint64(s), np.arange(N, dtype=np.uint64), np.uint64(SITE_SELECT), np.uint64(int(offset) & 0xFFFFFFFF),
                       int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    k = (words[0] >> np.uint32(8)).astype(np.float64)
    return (-np.log((k + 0.5) * 2.0 ** -24)).astype(np.float32).astype(np.float64)


class State:
    def __init__(self, x, weight=None, init=(), seed=0, offset=0, sample=True, origin=True):
        self.x = np.asarray(x, dtype=np.float64)
        self.N = self.x.shape[0]
        self.w = np.ones(self.N) if weight is None else np.asarray(weight, dtype=np.float64)
        self.seed, self.offset, self.sample, self.origin = seed, offset, bool(sample), bool(origin)
        self.finite = np.isfinite(self.x).all(axis=1)            # d(i, i) == 0: a row with a NaN or an infinity is never eligible
        with np.errstate(invalid='ignore', over='ignore'):
            self.mind = (self.x ** 2).sum(axis=1) if origin else np.full(self.N, np.inf)      # the origin: d(i, 0), assign -1
        self.assign = np.full(self.N, -1, dtype=np.int64)
        self.taken = np.zeros(self.N, dtype=bool)
        self.has_center = bool(origin)
        self.step = 0
        for c in init:
            self.add(int(c))

    def add(self, c):
        """row c becomes a center; an index outside [0, N) - the -1 of an exhausted selection - changes nothing"""
        if not 0 <= c < self.N:
            return
        with np.errstate(invalid='ignore', over='ignore'):
            d = ((self.x - self.x[c]) ** 2).sum(axis=1)
            closer = d < self.mind                               # strictly smaller replaces: the first center that attains the minimum stays
        self.assign[closer] = c
        self.mind = np.where(closer | np.isnan(d), d, self.mind)
        self.taken[c] = True
        self.has_center = True

    def mass(self):
        """-> (w * mind, or w while there is no center; eligible)"""
        with np.errstate(invalid='ignore'):
            m = self.w * self.mind if self.has_center else self.w.copy()
            eligible = ~self.taken & self.finite & (self.w >= 0) & ~np.isnan(m)
        return m, eligible

    def scores(self):
        """-> (score of every row at step self.step, eligible)"""
        m, eligible = self.mass()
        if self.sample:
            with np.errstate(invalid='ignore'):
                m = m / exponentials(self.seed, self.offset, self.step, self.N)
        return m, eligible

    def best(self):
        """-> (the eligible row of maximal (score, w, -i), its mind before the pick, the relative gap of the runner-up's score below
        the best's - inf where there is no runner-up or the best score is 0 and decided by the other keys exactly) or (-1, -1.0, inf)"""
        score, eligible = self.scores()
        idx = np.flatnonzero(eligible)
        if not len(idx):
            return -1, -1.0, np.inf
        order = idx[np.lexsort((idx, -self.w[idx], -score[idx]))]
        top = order[0]
        gap = np.inf
        if len(order) > 1 and score[top] > 0 and np.isfinite(score[top]):
            gap = (score[top] - score[order[1]]) / score[top]
        return int(top), float(self.mind[top]), float(gap)

    def advance(self, c):
        """the pick of this step was c (the kernel's, or best()'s)"""
        self.add(int(c))
        self.step += 1


def run(x, n_select, weight=None, init=(), seed=0, offset=0, sample=True, origin=True, snapshots=()):
    """-> dict(picked int64 [n_select], pick_dist float64 [n_select], gap float64 [n_select], mind, assign: the state after every
    center, open_mind: mind before the first center of init, state[k] = (mind, assign) after the first k picks for k in snapshots)"""
    st = State(x, weight, (), seed, offset, sample, origin)
    open_mind = st.mind.copy()
    for c in init:
        st.add(int(c))
    picked, dist, gaps, snaps = [], [], [], {}
    if 0 in snapshots:
        snaps[0] = (st.mind.copy(), st.assign.copy())
    for s in range(n_select):
        i, d, gap = st.best()
        picked.append(i)
        dist.append(d)
        gaps.append(gap)
        st.advance(i)
        if s + 1 in snapshots:
            snaps[s + 1] = (st.mind.copy(), st.assign.copy())
    return dict(picked=np.array(picked, dtype=np.int64), pick_dist=np.array(dist, dtype=np.float64), gap=np.array(gaps), mind=st.mind,
                assign=st.assign, open_mind=open_mind, state=snaps)


def chi_square(counts, prob):
    """Pearson's statistic of observed counts against the probabilities prob"""
    counts, prob = np.asarray(counts, dtype=np.float64), np.asarray(prob, dtype=np.float64)
    expect = counts.sum() * prob / prob.sum()
    return float(((counts - expect) ** 2 / expect).sum())


# ---- the case of the sampler's law (tests/test_grad_embed.py on the reference, tests/test_gpu_kcenter_sample.py on the device)
LAW_SEED_BASE = 0        # chosen on the CPU so that the reference itself passes the bar below
LAW_SEEDS = 2000
LAW_BAR = 20.5           # the 0.001 quantile of chi-square with 5 degrees of freedom (20.515)


def law_case():
    """six eligible lattice rows around one init row at (0, 0), no origin center: mind = 1, 2, 4, 5, 8, 9 and w * mind = 1, 2, 4, 2.5,
    8, 2.25 - pairwise distinct, none zero, every product exact in float32 -> (x, w, init, the masses of rows 1..6)"""
    x = np.array([[0, 0], [1, 0], [1, 1], [2, 0], [2, 1], [2, 2], [3, 0]], dtype=np.float32)
    w = np.array([1, 1, 1, 1, 0.5, 1, 0.25], dtype=np.float32)
    mass = w[1:].astype(np.float64) * (x[1:].astype(np.float64) ** 2).sum(axis=1)
    return x, w, [0], mass
