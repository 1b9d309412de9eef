"""Reference of hual_al_label_gain (include/hual_seqpan.h) for the tests: the contract restated in float64 on the CPU, by enumeration.

On top of al_label_ref: the state of a sample (the members of its consistent set A with their float64 weights) and V0 = the maximum of
all_R over it.  For a frame t the two states the annotator's answer can leave are the members of A that hold t and those that do not;
the value of a branch is the maximum, over its members c, of the sum over its members (i, j) of w(i,j) * IoU(c, (i,j)) - every pair
of spans enumerated, no prefix or suffix sum, so the kernel's regions and factorisation are checked against the definition itself.

The IoU of every pair of members of A is computed once per state where it fits (|A| <= MATRIX_MAX: every state at T <= 70) and a branch
is then one masked matrix-vector product; a larger A (T = 256, where only a few frames are asked for) is walked in chunks of candidates."""
import functools

import numpy as np
import torch

import al_label_ref as L
import al_query_ref as Q
import span_topk_ref as R

POISONED, CONTRADICTORY, LIVE = Q.POISONED, Q.CONTRADICTORY, Q.LIVE
MATRIX_MAX = 2600      # |A| up to which the pairwise IoU matrix is kept (the full triangle at T = 70 has 2485 spans)
ROWS = {2: range(Q.N_ROWS), 33: range(Q.N_ROWS), 70: range(4)}      # the rows of al_query_ref.case(T) the all-frames tests evaluate


def pair_iou(ci, cj, ai, aj):
    """frame-count IoU [C, K] of the spans (ci, cj) with the spans (ai, aj), as al_label_ref.expected_iou takes it"""
    ci, cj, ai, aj = (np.asarray(x, dtype=np.int32) for x in (ci, cj, ai, aj))
    inter = np.maximum(0, np.minimum(cj[:, None], aj[None, :]) + 1 - np.maximum(ci[:, None], ai[None, :]))
    union = (cj - ci + 1)[:, None] + (aj - ai + 1)[None, :] - inter
    return inter / union


def branch_value(st, m, iou=None):
    """(mass, M) of the members of A selected by the boolean mask m: M = the max over the selected c of the sum over the selected (i, j) of
    w * IoU(c, (i, j)); 0 where the mass is not positive"""
    z = st['w'][m].sum()
    if not z > 0:
        return z, 0.0
    if iou is not None:
        return z, float((iou @ np.where(m, st['w'], 0.0))[m].max())
    ai, aj, w = st['ai'][m], st['aj'][m], st['w'][m]
    return z, max(float((pair_iou(ai[c:c + L.CHUNK], aj[c:c + L.CHUNK], ai, aj) @ w).max()) for c in range(0, len(ai), L.CHUNK))


def gain_ref(ps, pe, v, aps, frames=None, nan_logit=False):
    """one sample -> dict(status, st, value = V0, frames = the evaluated frames in order, gain [v] (0 at a frame not evaluated), raw [v]
    (the gain before the clamp; nan where not evaluated, 0 where the answer is determined), zp / zn [v] (the two masses; nan where not
    evaluated), ask_point, ask_gain, margin = the best gain minus the second best over the other evaluated frames (inf with fewer than
    two)).  frames: the candidate list (entries outside [0, v) are skipped), None = every frame.  A row that has no answer to give:
    ask_point -1, ask_gain = value = -1.0."""
    st = L.state(ps, pe, v, aps, nan_logit)
    if st['status'] != LIVE:
        return dict(status=st['status'], st=st, value=-1.0, frames=[], gain=np.zeros(max(v, 0)), ask_point=-1, ask_gain=-1.0, margin=np.inf)
    ev = [int(t) for t in (range(v) if frames is None else frames) if 0 <= t < v]
    ai, aj = st['ai'], st['aj']
    iou = pair_iou(ai, aj, ai, aj) if len(ai) <= MATRIX_MAX else None
    if iou is not None:
        V0 = float((iou @ st['w']).max() / st['ZA'])
        assert abs(V0 - L.all_R(st).max()) <= 1e-14                    # the matrix-vector form is al_label_ref's enumeration
    else:
        V0 = float(L.all_R(st).max())
    gain, raw, zp, zn = np.zeros(v), np.full(v, np.nan), np.full(v, np.nan), np.full(v, np.nan)
    for t in ev:
        holds = (ai <= t) & (t <= aj)
        zp[t], mp = branch_value(st, holds, iou)
        zn[t], mn = branch_value(st, ~holds, iou)
        raw[t] = (mp + mn) / st['ZA'] - V0 if zp[t] > 0 and zn[t] > 0 else 0.0      # a determined answer: exactly 0
        gain[t] = min(max(raw[t], 0.0), 1.0)
    out = dict(status=LIVE, st=st, value=V0, frames=ev, gain=gain, raw=raw, zp=zp, zn=zn, ask_point=-1, ask_gain=0.0, margin=np.inf)
    if ev:
        g = gain[ev]
        k = int(np.argmax(g))                                           # the first evaluated frame of maximal gain
        out.update(ask_point=ev[k], ask_gain=float(g[k]), margin=float(g[k] - np.delete(g, k).max()) if len(ev) > 1 else np.inf)
    return out


@functools.lru_cache(maxsize=None)
def case(T):
    """al_label_ref.case(T), T in ROWS, with gref[h][n] = gain_ref over every frame of row n after the answers of history h (None for
    the rows outside ROWS[T]) - each computed once"""
    c = L.case(T)
    gref = {h: [gain_ref(c['ps'][n], c['pe'][n], int(c['v'][n]), c['aps'][h][n]) if n in ROWS[T] else None for n in range(Q.N_ROWS)]
            for h in Q.HISTORIES}
    return dict(c, gref=gref)


def set_ref(s_logits, e_logits, vlen, tlen, aps, cand=None):
    """a whole set, as al_label_ref.set_ref reads it: row n is the tlen[n] first columns, v = vlen clamped to [0, tlen]; cand: per row
    the candidate list (None: every frame) -> the list of gain_ref dicts"""
    s = torch.as_tensor(s_logits, dtype=torch.float32).cpu()
    e = torch.as_tensor(e_logits, dtype=torch.float32).cpu()
    out = []
    for n in range(s.shape[0]):
        T = int(tlen[n])
        ps, pe, v, _ = R.probabilities(s[n:n + 1, :T], e[n:n + 1, :T], torch.as_tensor([int(vlen[n])]))
        v = int(v[0])
        nan = bool(torch.isnan(s[n, :v]).any() or torch.isnan(e[n, :v]).any())
        out.append(gain_ref(ps[0], pe[0], v, aps[n], frames=None if cand is None else cand[n], nan_logit=nan))
    return out


def by_index(r):
    """is this state one whose ask_point the kernel has to reproduce exactly: a gain to be had, and a runner-up ten bars below it"""
    return r['status'] == LIVE and r['ask_gain'] > 1e-9 and r['margin'] > 1e-5
