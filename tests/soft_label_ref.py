"""Reference of hual_al_span_marginals and of the soft-label blend of hual_assemble_batch_soft (include/hual_seqpan.h) for the tests:
the contracts restated on the CPU.

The marginals: the probabilities are span_topk_ref.probabilities (float32, bit for bit the kernel's); the weights and the consistent
set A are al_query_ref.weights / consistent.  From there on everything is float64 and enumeration of the [v, v] matrix only: the start
marginal is the row sums of the weights restricted to A over Z_A, the end marginal the column sums.  No prefix or suffix sum anywhere,
so the kernel's factorisation into interval sums is checked against the definition itself.

The blend: hual_amd.data.make_labels (the reference's labels) moved towards the banks in numpy float32, one rounding per operation -
what the kernel's three separately rounded operations compute, bit for bit."""
import functools

import numpy as np
import torch

import al_query_ref as Q
import span_topk_ref as R

POISONED, CONTRADICTORY, LIVE = Q.POISONED, Q.CONTRADICTORY, Q.LIVE


def marginals_ref(ps, pe, v, aps, nan_logit=False):
    """one sample: dict(status, y_start [v], y_end [v], ZA) in float64 by the row rules of the contract (zeros on a row that is not live)"""
    flag = dict(y_start=np.zeros(max(v, 0)), y_end=np.zeros(max(v, 0)), ZA=float('nan'))
    if v < 1 or nan_logit:
        return dict(flag, status=POISONED)
    W, _ = Q.weights(ps, pe, v)
    Z = W[np.triu(np.ones((v, v), dtype=bool))].sum()
    if not (Z > 0 and np.isfinite(Z)):
        return dict(flag, status=POISONED)
    WA = np.where(Q.consistent(v, aps), W, 0.0)
    ZA = WA.sum()
    if not ZA > 0:
        return dict(flag, status=CONTRADICTORY, ZA=ZA)
    return dict(status=LIVE, y_start=WA.sum(1) / ZA, y_end=WA.sum(0) / ZA, ZA=ZA)


def incl_from_marginals(r):
    """q(t) = sum_{i <= t} y_start[i] - sum_{j < t} y_end[j]: the spans that have started by t minus those that have ended before it"""
    cs, ce = np.cumsum(r['y_start']), np.cumsum(r['y_end'])
    return cs - np.concatenate([[0.0], ce[:-1]])


def set_ref(s_logits, e_logits, vlen, tlen, aps):
    """a whole set, as al_query_ref.set_ref reads it: row n is the tlen[n] first columns, v = vlen clamped to [0, tlen] -> the list of
    marginals_ref dicts (each with its v)"""
    s = torch.as_tensor(s_logits, dtype=torch.float32).cpu()
    e = torch.as_tensor(e_logits, dtype=torch.float32).cpu()
    out = []
    for n in range(s.shape[0]):
        T = int(tlen[n])
        ps, pe, v, _ = R.probabilities(s[n:n + 1, :T], e[n:n + 1, :T], torch.as_tensor([int(vlen[n])]))
        v = int(v[0])
        nan = bool(torch.isnan(s[n, :v]).any() or torch.isnan(e[n, :v]).any())
        out.append(dict(marginals_ref(ps[0], pe[0], v, aps[n], nan_logit=nan), v=v))
    return out


@functools.lru_cache(maxsize=None)
def case(T):
    """al_query_ref.case(T) with, for every history h, mref[h][n] = marginals_ref of that row-state - each computed once"""
    c = Q.case(T)
    mref = {h: [marginals_ref(c['ps'][n], c['pe'][n], int(c['v'][n]), c['aps'][h][n]) for n in range(Q.N_ROWS)] for h in Q.HISTORIES}
    return dict(c, mref=mref)


def blend(r, bank, lam, n):
    """one row: the reference's float32 labels r [T] moved towards bank [>= n] by the weight lam on the frames [0, n) - float32, one
    rounding per operation; lam == 0 returns r itself (the bank is not read)"""
    r = np.asarray(r, dtype=np.float32)
    lam = np.float32(lam)
    if lam == 0:
        return r.copy()
    out = r.copy()
    b = np.asarray(bank, dtype=np.float32)[:n]
    out[:n] = r[:n] + lam * (b - r[:n])                                # (float32 arrays and a float32 scalar: every operation rounds to float32)
    return out


def soft_labels_ref(s_ind, e_ind, lens, T, bank1, bank2, w):
    """the label feeds of a batch padded to T frames: (y1, y2 float32 [B, T] blended, match i32, inner f32 of the hard label); s_ind,
    e_ind, lens [B]; bank1 / bank2 [B, >= lens]; w [B]"""
    from hual_amd import data
    y1, y2, match, inner = data.make_labels(s_ind, e_ind, lens, max_len=T)
    o1 = np.stack([blend(y1[b], bank1[b], w[b], int(lens[b])) for b in range(len(lens))])
    o2 = np.stack([blend(y2[b], bank2[b], w[b], int(lens[b])) for b in range(len(lens))])
    return o1, o2, match, inner.astype(np.float32)
