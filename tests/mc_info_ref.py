"""Reference of hual_al_mc_fold_info / hual_al_score_info's model-uncertainty term (include/hual_seqpan.h) for the tests: numpy on the CPU,
in float64 - the yardstick the device's float32 arithmetic is measured against, not a restatement of it.

The probabilities are the float32 ones of tests/mc_uncert_ref.probs (torch.sigmoid, zero at t >= v_len).  Per head the fold keeps the
float64 mean of the passes' binary entropy h2 (bits) and the float64 mean of the passes' probabilities; the three statistics are read from
those two: ENTROPY = h2(mean p) (total), EXPECTED_ENTROPY = mean h2(p_k) (aleatoric), BALD = their difference (epistemic: the mutual
information between the prediction and the dropout mask), clamped at 0 as the device clamps it."""
import numpy as np

from mc_uncert_ref import F32, probs  # noqa: F401  (probs: where the tests' probabilities come from)

STATS = ('bald', 'entropy', 'expected_entropy')


def _h2(p):
    """binary entropy in bits of float64 p; 0 at p <= 0 and at p >= 1"""
    p = np.asarray(p, dtype=np.float64)
    inside = (p > 0.0) & (p < 1.0)
    ps = np.where(inside, p, 0.5)
    q = 1.0 - ps
    return np.where(inside, -(ps * np.log2(ps) + q * np.log2(q)), 0.0)


def h2_64(p):
    """float64 binary entropy in bits of FLOAT32 probabilities (the rule p <= 0 or p >= 1 -> 0 is applied to the float32 value)"""
    return _h2(np.asarray(p, dtype=F32).astype(np.float64))


class InfoFold:
    """one head of one bank row (or a block of rows): fold(p) for k = 1, 2, ..."""

    def __init__(self):
        self.k = 0

    def fold(self, p):
        p = np.asarray(p, dtype=F32)
        self.k += 1
        if self.k == 1:
            self.sum_p, self.sum_h = p.astype(np.float64), h2_64(p)
        else:
            self.sum_p, self.sum_h = self.sum_p + p.astype(np.float64), self.sum_h + h2_64(p)
        return self

    @property
    def mean(self):
        return self.sum_p / self.k

    @property
    def ent(self):
        """EXPECTED_ENTROPY of the head: the mean over the passes of h2(p_k)"""
        return self.sum_h / self.k

    def entropy(self):
        """ENTROPY of the head: h2 of the mean probability"""
        return _h2(self.mean)

    def mi(self):
        """h2(mean) - ent before the clamp: >= 0 by Jensen up to float64 rounding"""
        return self.entropy() - self.ent

    def bald(self):
        return np.maximum(0.0, self.mi())


def fold_passes(ps):
    """ps [K, ...] float32 probabilities -> InfoFold after K passes"""
    f = InfoFold()
    for p in ps:
        f.fold(p)
    return f


def uncert(fs, fe, stat):
    """the model-uncertainty term (float64) from the two heads' folds: the sum over the start and end heads"""
    if stat == 'bald':
        return fs.bald() + fe.bald()
    if stat == 'entropy':
        return fs.entropy() + fe.entropy()
    if stat == 'expected_entropy':
        return fs.ent + fe.ent
    raise ValueError(stat)
