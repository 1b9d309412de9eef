"""Reference of hual_al_mc_fold / hual_al_score_mc's model-uncertainty term (include/hual_seqpan.h) for the tests: numpy on the CPU.

The fold is restated in float32, operation by operation (numpy never fuses): float32 sigmoid probabilities zeroed at t >= v_len, running
minimum / maximum, Welford's mean and sum of squared deviations.  spread64 is the float64 yardstick of the STD statistic:
sqrt(2) times the sample deviation (ddof = 1) of the same float32 probabilities."""
import numpy as np

F32 = np.float32
SQRT2 = F32(np.sqrt(2.0))


def probs(logits, v_len):
    """float32 torch.sigmoid of logits [..., T], zero at t >= v_len: the probabilities of get_uncert_model (utils_hual.py:144-161, as
    oracle.al_ref restates it).  The kernel's 1/(1+expf(-x)) is within an ulp or two of it."""
    import torch
    x = np.ascontiguousarray(logits, dtype=F32)
    p = torch.sigmoid(torch.from_numpy(x)).numpy()
    v = np.asarray(v_len)[..., None]                            # a scalar, or one length per row
    return np.where(np.arange(x.shape[-1]) < v, p, F32(0)).astype(F32)


class Fold:
    """the state one bank row (or a block of rows) goes through: fold(p) for k = 1, 2, ..."""

    def __init__(self):
        self.k = 0

    def fold(self, p):
        p = np.asarray(p, dtype=F32)
        self.k += 1
        if self.k == 1:
            self.lo, self.hi, self.mean, self.m2 = p.copy(), p.copy(), p.copy(), np.zeros_like(p)
            return self
        self.lo, self.hi = np.minimum(self.lo, p), np.maximum(self.hi, p)
        d = (p - self.mean).astype(F32)
        self.mean = (self.mean + (d / F32(self.k)).astype(F32)).astype(F32)
        self.m2 = (self.m2 + (d * (p - self.mean).astype(F32)).astype(F32)).astype(F32)
        return self

    def range(self):
        return (self.hi - self.lo).astype(F32)

    def std(self):
        """sqrtf(2) * sqrtf(m2 / (K - 1)), float32"""
        return (SQRT2 * np.sqrt((self.m2 / F32(self.k - 1)).astype(F32)).astype(F32)).astype(F32)


def fold_passes(ps):
    """ps [K, ...] float32 probabilities -> Fold after K passes"""
    f = Fold()
    for p in ps:
        f.fold(p)
    return f


def uncert(fs, fe, stat):
    """the model-uncertainty term from the two heads' folds: RANGE (hi_s - lo_s) + (hi_e - lo_e), STD sqrtf(2) * (std_s + std_e)"""
    if stat == 'range':
        return (fs.range() + fe.range()).astype(F32)
    K = F32(fs.k - 1)
    return (SQRT2 * (np.sqrt((fs.m2 / K).astype(F32)) + np.sqrt((fe.m2 / K).astype(F32))).astype(F32)).astype(F32)


def spread64(ps):
    """sqrt(2) * the float64 sample deviation (ddof = 1) over the K passes"""
    return np.sqrt(2.0) * np.std(np.asarray(ps, dtype=np.float64), axis=0, ddof=1)
