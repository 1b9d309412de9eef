"""Reference of hual_al_hit_label (include/hual_seqpan.h) for the tests: the contract restated in float64 on the CPU, by enumeration.

The probabilities are span_topk_ref.probabilities (float32, bit for bit the kernel's).  The weights and the consistent set A are
al_query_ref.weights / consistent - a [v, v] matrix and a boolean mask over it - and every (candidate, truth) pair goes through
span_hit_ref.hit_mass, the integer hit rule as a matrix: one sum per candidate over the truths in A, divided by the sum over A.  No
interval of hitting ends, no prefix sum, no table of admissible ends - the kernel's shortcuts are what this checks."""
import functools

import numpy as np
import torch

import al_query_ref as Q
import span_hit_ref as H
import span_topk_ref as R

POISONED, CONTRADICTORY, LIVE = Q.POISONED, Q.CONTRADICTORY, Q.LIVE
THR3 = [(3, 10), (1, 2), (7, 10)]
FULL_MAX = 2500      # members of A up to which every member is enumerated as a candidate (T = 70 without answers: 2,485)


def state(ps, pe, v, aps, nan_logit=False):
    """one sample: dict(status, v) and on a live row the truths of A in row-major order - ii, jj, w float64 - with ZA, their sum; the
    edge rules are al_query_ref.posterior_ref's"""
    if v < 1 or nan_logit:
        return dict(status=POISONED, v=v)
    W, _ = Q.weights(ps, pe, v)
    with np.errstate(invalid='ignore'):
        Z = W[np.triu(np.ones((v, v), dtype=bool))].sum()
    if not (Z > 0 and np.isfinite(Z)):
        return dict(status=POISONED, v=v)
    ok = Q.consistent(v, aps)
    ii, jj = np.nonzero(ok)                                           # (row-major)
    w = W[ii, jj]
    ZA = w.sum()
    if not ZA > 0:
        return dict(status=CONTRADICTORY, v=v)
    return dict(status=LIVE, v=v, ii=ii, jj=jj, w=w, ZA=ZA, ok=ok)


def is_member(st, a, b):
    return 0 <= a <= b < st['v'] and bool(st['ok'][a, b])


def cand_prob(st, cands, thr):
    """hit probability float64 [k, M] of the spans cands [k, 2] under the posterior `st`: -1.0 for a slot that is no span of the
    clip, and everywhere on a row that is not live"""
    cands = np.asarray(cands, dtype=np.int64).reshape(-1, 2)
    out = np.full((len(cands), len(thr)), -1.0)
    if st['status'] != LIVE:
        return out
    valid = (cands[:, 0] >= 0) & (cands[:, 0] <= cands[:, 1]) & (cands[:, 1] < st['v'])
    if valid.any():
        out[valid] = np.clip(H.hit_mass(st['ii'], st['jj'], st['w'], cands[valid, 0], cands[valid, 1], thr) / st['ZA'], 0.0, 1.0)
    return out


def best_ref(st, thr):
    """every member of A as a candidate -> dict(prob [|A|, M], best [M] index into ii / jj of the first maximiser in row-major order,
    top [M] its value, gap [M] its distance to the best OTHER member (inf with a single member)); None on a row that is not live"""
    if st['status'] != LIVE:
        return None
    prob = cand_prob(st, np.stack([st['ii'], st['jj']], axis=1), thr)
    best = prob.argmax(axis=0)                                        # (numpy: the first of equal maxima)
    top = prob[best, np.arange(len(thr))]
    gap = np.full(len(thr), np.inf)
    if len(prob) > 1:
        for m in range(len(thr)):
            gap[m] = top[m] - np.delete(prob[:, m], best[m]).max()
    return dict(prob=prob, best=best, top=top, gap=gap)


def set_ref(s_logits, e_logits, vlen, tlen, aps):
    """a whole set -> the list of state() dicts; row n is read as its tlen[n] first columns, v = vlen clamped to [0, tlen]"""
    s = torch.as_tensor(s_logits, dtype=torch.float32).cpu()
    e = torch.as_tensor(e_logits, dtype=torch.float32).cpu()
    out = []
    for n in range(s.shape[0]):
        T = int(tlen[n])
        if not 1 <= T <= min(256, s.shape[1]):                        # a row the family does not handle: poisoned
            out.append(dict(status=POISONED, v=0))
            continue
        ps, pe, v, _ = R.probabilities(s[n:n + 1, :T], e[n:n + 1, :T], torch.as_tensor([int(vlen[n])]))
        v = int(v[0])
        nan = bool(torch.isnan(s[n, :v]).any() or torch.isnan(e[n, :v]).any())
        out.append(state(ps[0], pe[0], v, aps[n], nan_logit=nan))
    return out


@functools.lru_cache(maxsize=None)
def states(T, h):
    """the states of the shared case al_query_ref.case(T) after h answers, computed once"""
    c = Q.case(T)
    return [state(c['ps'][n], c['pe'][n], int(c['v'][n]), c['aps'][h][n]) for n in range(Q.N_ROWS)]


@functools.lru_cache(maxsize=None)
def full_best(T, h, thr=tuple(THR3)):
    """best_ref of every row of the shared case whose A holds at most FULL_MAX members (None for the larger ones), computed once"""
    return [best_ref(st, list(thr)) if st['status'] == LIVE and len(st['ii']) <= FULL_MAX else None for st in states(T, h)]


def mode(st):
    """the heaviest member of A, the first in row-major order"""
    q = int(np.argmax(st['w']))
    return int(st['ii'][q]), int(st['jj'][q])


def random_spans(st, count, seed, inside):
    """`count` spans of the clip drawn with replacement: members of A (inside) or any span of the triangle -> int64 [count, 2]"""
    rng = np.random.default_rng(seed)
    if inside:
        q = rng.integers(0, len(st['ii']), count)
        return np.stack([st['ii'][q], st['jj'][q]], axis=1).astype(np.int64)
    a = rng.integers(0, st['v'], count)
    b = np.array([rng.integers(x, st['v']) for x in a])
    return np.stack([a, b], axis=1).astype(np.int64)
