"""Reference of hual_span_hit_prob (include/hual_seqpan.h) for the tests: the contract restated on the CPU as a plain enumeration.

The probabilities are span_topk_ref.probabilities (float32, bit for bit the kernel's).  From there on everything is float64 and nothing
is clever: the weights p_s[i] * p_e[j] of the whole triangle, the integer hit rule den * inter >= num * union evaluated for every
(candidate, span) pair, one sum per candidate.  No interval of hitting ends, no prefix sums - the kernel's shortcut is what this checks."""
import numpy as np
import torch

import span_conf_ref as C
import span_topk_ref as R
from span_clip_util import stable_order      # noqa: F401 (the tests reach it through this module)


def hits(a, b, ii, jj, num, den):
    """bool per span (ii, jj): it hits the candidate [a, b] at IoU >= num / den, in integers on the half-open frame intervals"""
    inter = np.maximum(0, np.minimum(b, jj) + 1 - np.maximum(a, ii))
    union = (b - a + 1) + (jj - ii + 1) - inter
    return den * inter >= num * union


def alive_row(s_row, e_row, n):
    return n >= 1 and not (np.isnan(s_row[:n]).any() or np.isnan(e_row[:n]).any())


def hit_mass(ii, jj, w, ca, cb, thr, chunk=64):
    """sum of w over the spans (ii, jj) that hit each candidate (ca, cb): float64 [len(ca), M].  `chunk` candidates at a time against
    every span, the rule of hits() as a matrix - every (candidate, span) pair is tested (int32: den * inter <= 1024 * 256)"""
    ii, jj = np.asarray(ii, dtype=np.int32), np.asarray(jj, dtype=np.int32)
    ca, cb = np.asarray(ca, dtype=np.int32), np.asarray(cb, dtype=np.int32)
    out = np.empty((len(ca), len(thr)))
    for c in range(0, len(ca), chunk):
        a, b = ca[c:c + chunk, None], cb[c:c + chunk, None]
        inter = np.maximum(0, np.minimum(b, jj[None, :]) + 1 - np.maximum(a, ii[None, :]))
        union = (b - a + 1) + (jj - ii + 1)[None, :] - inter
        for m, (num, den) in enumerate(thr):
            out[c:c + chunk, m] = (den * inter >= num * union).astype(np.float64) @ w
    return out


def clip_hit_prob(ps, pe, v, cands, thr):
    """one clip from its probabilities: hit probability float64 [len(cands), M] (-1.0 for an invalid candidate), or None when Z is not a
    positive finite number"""
    ii, jj, w = C.span_weights(ps, pe, v)
    with np.errstate(invalid='ignore'):
        Z = w.sum()
    if not (Z > 0 and np.isfinite(Z)):
        return None
    cands = np.asarray(cands, dtype=np.int64).reshape(-1, 2)
    ok = (cands[:, 0] >= 0) & (cands[:, 0] <= cands[:, 1]) & (cands[:, 1] < v)
    out = np.full((len(cands), len(thr)), -1.0)
    out[ok] = hit_mass(ii, jj, w, cands[ok, 0], cands[ok, 1], thr) / Z
    return out


def clip_all_spans(ps, pe, v, thr):
    """hit probability float64 [n, M] of EVERY span of the triangle as a candidate, in row-major order, with (ii, jj); None for a dead Z"""
    ii, jj, w = C.span_weights(ps, pe, v)
    with np.errstate(invalid='ignore'):
        Z = w.sum()
    if not (Z > 0 and np.isfinite(Z)):
        return None
    return ii, jj, hit_mass(ii, jj, w, ii, jj, thr) / Z


def span_hit_ref(s_logits, e_logits, vlen, starts, ends, thr):
    """-> hit probability float64 [B,k,M] (-1.0: invalid slot, empty or poisoned row), alive bool [B] (the rows a reorder may permute)"""
    ps, pe, v, _ = R.probabilities(s_logits, e_logits, vlen)
    s = torch.as_tensor(s_logits, dtype=torch.float32).cpu().numpy()
    e = torch.as_tensor(e_logits, dtype=torch.float32).cpu().numpy()
    st, en = np.asarray(starts, dtype=np.int64), np.asarray(ends, dtype=np.int64)
    B, k = st.shape
    hp = np.full((B, k, len(thr)), -1.0)
    alive = np.zeros(B, dtype=bool)
    for b in range(B):
        n = int(v[b])
        if not alive_row(s[b], e[b], n):
            continue
        got = clip_hit_prob(ps[b], pe[b], n, list(zip(st[b], en[b])), thr)
        if got is not None:
            hp[b], alive[b] = got, True
    return hp, alive


def bayes_ref(s_logits, e_logits, vlen, thr):
    """the full enumeration of every candidate -> per row None (empty or poisoned) or dict(ii, jj, prob [n,M], best [M] flat index of the
    first maximiser in row-major order, top [M] its value, gap [M] its distance to the best OTHER span (inf with a single span))"""
    ps, pe, v, _ = R.probabilities(s_logits, e_logits, vlen)
    s = torch.as_tensor(s_logits, dtype=torch.float32).cpu().numpy()
    e = torch.as_tensor(e_logits, dtype=torch.float32).cpu().numpy()
    rows = []
    for b in range(ps.shape[0]):
        n = int(v[b])
        got = clip_all_spans(ps[b], pe[b], n, thr) if alive_row(s[b], e[b], n) else None
        if got is None:
            rows.append(None)
            continue
        ii, jj, prob = got
        best = prob.argmax(axis=0)                                   # (numpy: the first of equal maxima)
        top = prob[best, np.arange(len(thr))]
        gap = np.full(len(thr), np.inf)
        if len(ii) > 1:
            for m in range(len(thr)):
                gap[m] = top[m] - np.delete(prob[:, m], best[m]).max()
        rows.append(dict(ii=ii, jj=jj, prob=prob, best=best, top=top, gap=gap))
    return rows
