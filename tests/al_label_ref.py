"""Reference of hual_al_mbr_label (include/hual_seqpan.h) for the tests: the contract restated in float64 on the CPU, by enumeration.

The probabilities are span_topk_ref.probabilities (float32, bit for bit the kernel's); the weights and the consistent set A are
al_query_ref.weights / consistent.  From there on everything is float64 and brute force: the expected tIoU R(a, e) of a candidate is
the sum over every member (i, j) of A of w(i,j) * inter / union, divided by Z_A; the label is the first maximum of R over every member
of A in row-major order.  No prefix or suffix sum anywhere, so the kernel's factorisation is checked against the definition itself.

Enumerating all pairs costs |A|^2: done for the row-states with |A| <= FULL_MAX (every one at T <= 70), in chunks of 512 candidates.
For the larger ones (the full 32,896-span triangles at T = 256 among them) the reference offers R of single spans at O(|A|) and a
set of probes around a given span."""
import functools

import numpy as np
import torch

import al_query_ref as Q
import span_topk_ref as R

POISONED, CONTRADICTORY, LIVE = Q.POISONED, Q.CONTRADICTORY, Q.LIVE
FULL_MAX = 8000      # |A| up to which R of every member is enumerated
CHUNK = 512


def state(ps, pe, v, aps, nan_logit=False):
    """one sample: dict(status, Z, ZA, ai, aj, w) - the members (ai[k], aj[k]) of A in row-major order with their float64 weights -
    by the row rules of the contract"""
    if v < 1 or nan_logit:
        return dict(status=POISONED)
    W, _ = Q.weights(ps, pe, v)
    Z = W[np.triu(np.ones((v, v), dtype=bool))].sum()
    if not (Z > 0 and np.isfinite(Z)):
        return dict(status=POISONED)
    ok = Q.consistent(v, aps)
    ai, aj = np.nonzero(ok)                                           # (row-major)
    w = W[ai, aj]
    ZA = w.sum()
    if not ZA > 0:
        return dict(status=CONTRADICTORY)
    return dict(status=LIVE, Z=Z, ZA=ZA, ai=ai, aj=aj, w=w, v=v)


def expected_iou(st, a, e):
    """R of the candidates (a[c], e[c]) under the live state `st`: float64 [C], one chunk (C * |A| terms)"""
    a, e = np.atleast_1d(np.asarray(a, dtype=np.int32)), np.atleast_1d(np.asarray(e, dtype=np.int32))
    ai, aj = st['ai'].astype(np.int32), st['aj'].astype(np.int32)
    inter = np.maximum(0, np.minimum(e[:, None], aj[None, :]) + 1 - np.maximum(a[:, None], ai[None, :]))      # (exact integers)
    union = (e - a + 1)[:, None] + (aj - ai + 1)[None, :] - inter
    return ((inter / union) * st['w'][None, :]).sum(axis=1) / st['ZA']      # (int32 / int32 is the float64 quotient)


def span_R(st, a, e):
    """R of one span, a member of A or not"""
    return float(expected_iou(st, [a], [e])[0])


def all_R(st):
    """R of every member of A, in chunks of CHUNK candidates"""
    n = len(st['ai'])
    return np.concatenate([expected_iou(st, st['ai'][c:c + CHUNK], st['aj'][c:c + CHUNK]) for c in range(0, n, CHUNK)])


def mode(st):
    """the posterior's mode: the first heaviest member of A"""
    k = int(np.argmax(st['w']))
    return int(st['ai'][k]), int(st['aj'][k])


def label_ref(ps, pe, v, aps, nan_logit=False):
    """dict(status, st, size = |A|, mode, and - where |A| <= FULL_MAX - label, conf, margin = conf minus the runner-up's R (inf with a
    single member), full=True); a row that gives no label: label (-1, -1), conf -1.0"""
    st = state(ps, pe, v, aps, nan_logit)
    if st['status'] != LIVE:
        return dict(status=st['status'], st=st, size=0, label=(-1, -1), conf=-1.0, full=True)
    out = dict(status=LIVE, st=st, size=len(st['ai']), mode=mode(st), full=len(st['ai']) <= FULL_MAX)
    if out['full']:
        val = all_R(st)
        k = int(np.argmax(val))                                         # the first maximum in row-major order
        rest = np.delete(val, k)
        out.update(label=(int(st['ai'][k]), int(st['aj'][k])), conf=float(val[k]), margin=float(val[k] - rest.max()) if len(rest) else np.inf)
    return out


def probes(st, span, seed):
    """the members of A a chosen span has to beat where all of A is too many: those within 3 frames of it at either end, the
    posterior's mode and 256 seeded random members -> (a [P], e [P])"""
    near = (np.abs(st['ai'] - span[0]) <= 3) & (np.abs(st['aj'] - span[1]) <= 3)
    rnd = np.random.default_rng(seed).integers(0, len(st['ai']), 256)
    m = mode(st)
    return (np.concatenate([st['ai'][near], [m[0]], st['ai'][rnd]]), np.concatenate([st['aj'][near], [m[1]], st['aj'][rnd]]))


def is_member(st, a, e):
    return bool(np.any((st['ai'] == a) & (st['aj'] == e)))


def old_valid(old, v):
    return bool(0 <= old[0] <= old[1] < v)


@functools.lru_cache(maxsize=None)
def case(T):
    """al_query_ref.case(T) with, for every history h, per row: ref[h][n] = label_ref of that state; old[h] int64 [16, 2] the old spans
    (seeded: the even rows a member of A, the odd ones anywhere in the clip) and old_conf[h] [16] their R - each computed once"""
    c = Q.case(T)
    ref, old, old_conf = {}, {}, {}
    for h in Q.HISTORIES:
        rng = np.random.default_rng(7300 + 16 * T + h)
        ref[h], old[h], old_conf[h] = [], np.zeros((Q.N_ROWS, 2), dtype=np.int64), np.zeros(Q.N_ROWS)
        for n in range(Q.N_ROWS):
            v = int(c['v'][n])
            r = label_ref(c['ps'][n], c['pe'][n], v, c['aps'][h][n])
            ref[h].append(r)
            a = int(rng.integers(0, v))
            o = (a, int(rng.integers(a, v)))
            k = int(rng.integers(0, max(r['size'], 1)))
            if n % 2 == 0 and r['status'] == LIVE:
                o = (int(r['st']['ai'][k]), int(r['st']['aj'][k]))
            old[h][n] = o
            old_conf[h][n] = span_R(r['st'], *o) if r['status'] == LIVE else -1.0
    return dict(c, lref=ref, old=old, old_conf=old_conf)


def set_ref(s_logits, e_logits, vlen, tlen, aps):
    """a whole set, as al_query_ref.set_ref reads it: row n is the tlen[n] first columns, v = vlen clamped to [0, tlen] -> the list of
    label_ref dicts"""
    s = torch.as_tensor(s_logits, dtype=torch.float32).cpu()
    e = torch.as_tensor(e_logits, dtype=torch.float32).cpu()
    out = []
    for n in range(s.shape[0]):
        T = int(tlen[n])
        ps, pe, v, _ = R.probabilities(s[n:n + 1, :T], e[n:n + 1, :T], torch.as_tensor([int(vlen[n])]))
        v = int(v[0])
        nan = bool(torch.isnan(s[n, :v]).any() or torch.isnan(e[n, :v]).any())
        out.append(label_ref(ps[0], pe[0], v, aps[n], nan_logit=nan))
    return out
