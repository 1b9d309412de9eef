"""Reference of hual_span_hit_cover (include/hual_seqpan.h) for the tests: the contract restated on the CPU as a plain enumeration.

The probabilities are span_topk_ref.probabilities (float32, bit for bit the kernel's).  From there on everything is float64 and nothing
is clever: the weights p_s[i] * p_e[j] of the whole triangle, the integer hit rule of span_hit_ref.hits evaluated for every
(candidate, truth) pair, the coverage of a set as a boolean mask over the truths, the greedy picks through an explicit residual vector
(the weights with the covered truths zeroed) and the first maximiser in row-major order.  No interval of hitting ends, no prefix sums,
no lists - the kernel's shortcuts are what this checks.  For a clip too long for all pairs, `cands` restricts the candidates to a field
of spans; the truths are always the whole triangle."""
import numpy as np
import torch

import span_conf_ref as C
import span_hit_ref as H
import span_topk_ref as R


class ClipCover:
    """one clip and a list of (num, den) thresholds.  alive False: Z is not a positive finite number (nothing else may be called)"""

    def __init__(self, ps, pe, v, thr, cands=None, chunk=256):
        self.v, self.thr, self.chunk = int(v), list(thr), chunk
        ii, jj, self.w = C.span_weights(ps, pe, self.v)
        self.ii, self.jj = ii.astype(np.int32), jj.astype(np.int32)
        with np.errstate(invalid='ignore'):
            self.Z = self.w.sum()
        self.alive = bool(self.Z > 0 and np.isfinite(self.Z))
        if cands is None:                                             # the whole triangle, in row-major order
            self.ca, self.cb = self.ii, self.jj
        else:
            cands = np.asarray(cands, dtype=np.int32).reshape(-1, 2)
            self.ca, self.cb = cands[:, 0], cands[:, 1]
        self._hit, self._gains = {}, {}

    def valid(self, a, b):
        return 0 <= a <= b < self.v

    def index(self, a, b):
        """the first candidate equal to (a, b)"""
        return int(np.nonzero((self.ca == a) & (self.cb == b))[0][0])

    def hit(self, m):
        """bool [candidates, truths]: every pair through the integer rule"""
        if m not in self._hit:
            num, den = self.thr[m]
            out = np.empty((len(self.ca), len(self.ii)), dtype=bool)
            for c in range(0, len(self.ca), self.chunk):
                out[c:c + self.chunk] = H.hits(self.ca[c:c + self.chunk, None], self.cb[c:c + self.chunk, None], self.ii[None, :], self.jj[None, :], num, den)
            self._hit[m] = out
        return self._hit[m]

    def covered(self, m, spans):
        """bool per truth: some valid span of `spans` hits it"""
        num, den = self.thr[m]
        mask = np.zeros(len(self.ii), dtype=bool)
        for a, b in spans:
            if self.valid(a, b):
                mask |= H.hits(int(a), int(b), self.ii, self.jj, num, den)
        return mask

    def coverage(self, m, spans):
        """float64 per slot: the coverage of the valid spans among spans[0..q] (0.0 while there is none)"""
        num, den = self.thr[m]
        mask = np.zeros(len(self.ii), dtype=bool)
        out = []
        for a, b in spans:
            if self.valid(a, b):
                mask |= H.hits(int(a), int(b), self.ii, self.jj, num, den)
            out.append(self.w[mask].sum() / self.Z)
        return np.array(out)

    def gains(self, m, picks):
        """float64 per candidate: the mass of the truths it hits that no span of `picks` hits, over Z"""
        key = (m, tuple((int(a), int(b)) for a, b in picks))
        if key not in self._gains:
            resid = np.where(self.covered(m, picks), 0.0, self.w)
            hit = self.hit(m)
            g = np.empty(len(self.ca))
            for c in range(0, len(self.ca), self.chunk):
                g[c:c + self.chunk] = hit[c:c + self.chunk] @ resid
            self._gains[key] = g / self.Z
        return self._gains[key]

    def greedy(self, m, K, min_gain):
        """-> (spans [K] of (a, b) or (-1, -1), cumulative coverage [K], per step taken: the best gain and its distance to the best OTHER
        candidate (inf with a single one))"""
        picks, spans, prob, best, gap = [], [], [], [], []
        last, stopped = 0.0, False
        for s in range(K):
            if not stopped:
                g = self.gains(m, picks)
                x = int(np.argmax(g))                                 # (numpy: the first of equal maxima, candidates in row-major order)
                if g[x] <= min_gain:
                    stopped = True
                else:
                    picks.append((int(self.ca[x]), int(self.cb[x])))
                    best.append(g[x])
                    gap.append(g[x] - np.delete(g, x).max() if len(g) > 1 else np.inf)
                    last = self.coverage(m, picks)[-1]
            spans.append((-1, -1) if stopped else picks[-1])
            prob.append(last)
        return spans, np.array(prob), np.array(best), np.array(gap)


def clips(s_logits, e_logits, vlen, thr):
    """-> per row None (empty, poisoned or a dead Z) or its ClipCover over the whole triangle"""
    ps, pe, v, _ = R.probabilities(s_logits, e_logits, vlen)
    s = torch.as_tensor(s_logits, dtype=torch.float32).cpu().numpy()
    e = torch.as_tensor(e_logits, dtype=torch.float32).cpu().numpy()
    rows = []
    for b in range(ps.shape[0]):
        n = int(v[b])
        c = ClipCover(ps[b], pe[b], n, thr) if H.alive_row(s[b], e[b], n) else None
        rows.append(c if c is not None and c.alive else None)
    return rows
