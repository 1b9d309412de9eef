"""Reference of hual_al_query (include/hual_seqpan.h) for the tests: the contract restated in float64 on the CPU, by enumeration.

The probabilities are span_topk_ref.probabilities (float32, bit for bit the kernel's).  Everything from there on is float64 and brute
force: the weights w(i,j) = p_s[i] * p_e[j] of the whole triangle sit in a [v, v] matrix, the consistent set A is a boolean mask over
it, and every sum - Z, Z_A, q(t) Z_A, the entropy sums - adds the matrix entries of its own region.  No prefix or suffix sum and no
difference of sums anywhere, so the kernel's factorisation into segmented sums is checked against the definition itself.

Also here: the truthful annotator (given a ground-truth span, answer a frame) and the seeded cases the CPU and GPU tests share, each
computed once."""
import functools

import numpy as np
import torch

import span_topk_ref as R

HISTORIES = (0, 1, 3, 6)      # truthful answers given before the posterior is read
TS = (2, 33, 70, 256)
N_ROWS = 16


def h2_64(q):
    """binary entropy in bits, float64; 0 at q <= 0 and q >= 1"""
    q = np.asarray(q, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        h = -(q * np.log2(q) + (1.0 - q) * np.log2(1.0 - q))
    return np.where((q <= 0) | (q >= 1), 0.0, h)


def answer(gt, t):
    """the truthful annotator (append_AP, utils_hual.py:133-139): is frame t inside the ground-truth span gt = (start, end)?"""
    return bool(gt[0] <= t <= gt[1])


def weights(ps, pe, v):
    """W [v, v] float64: p_s[i] * p_e[j] on i <= j, 0 below the diagonal; LG: log2 p_s[i] + log2 p_e[j] (-inf where a factor is 0)"""
    a, b = ps[:v].astype(np.float64), pe[:v].astype(np.float64)
    W = np.triu(np.outer(a, b))
    with np.errstate(divide='ignore'):
        LG = np.log2(a)[:, None] + np.log2(b)[None, :]
    return W, LG


def consistent(v, aps):
    """boolean [v, v]: the spans (i, j), i <= j, that every active point inside [0, v) allows"""
    ii, jj = np.indices((v, v))
    ok = ii <= jj
    for f, is_pos in aps:
        if not 0 <= f < v:
            continue
        inside = (ii <= f) & (f <= jj)
        ok &= inside if is_pos else ~inside
    return ok


def region_entropy(W, LG, mask):
    """(mass, entropy in bits) of the distribution W restricted to `mask`; entropy None when the mass is not positive"""
    w = W[mask]
    z = w.sum()
    if not z > 0:
        return z, None
    nz = w > 0
    return z, float(np.log2(z) - (w[nz] * LG[mask][nz]).sum() / z)


POISONED, CONTRADICTORY, LIVE = 'poisoned', 'contradictory', 'live'


def posterior_ref(ps, pe, v, aps, nan_logit=False):
    """one sample: dict(status, incl [v], gain [v], query_point, query_gain, post_entropy, agree, Z, ZA) in float64, by the edge rules
    of the contract (a poisoned or contradictory row carries the flag values and zeros)"""
    flag = dict(incl=np.zeros(max(v, 0)), gain=np.zeros(max(v, 0)), query_point=-1, query_gain=-1.0, post_entropy=-1.0)
    if v < 1 or nan_logit:
        return dict(flag, status=POISONED, agree=-1.0, Z=float('nan'), ZA=float('nan'))
    W, LG = weights(ps, pe, v)
    Z = W[np.triu(np.ones((v, v), dtype=bool))].sum()             # (the triangle as `consistent` lists it: with no active point Z_A == Z)
    if not (Z > 0 and np.isfinite(Z)):
        return dict(flag, status=POISONED, agree=-1.0, Z=Z, ZA=float('nan'))
    ok = consistent(v, aps)
    WA = np.where(ok, W, 0.0)
    ZA, H = region_entropy(W, LG, ok)
    if not ZA > 0:
        return dict(flag, status=CONTRADICTORY, agree=0.0, Z=Z, ZA=ZA)
    incl = np.array([WA[:t + 1, t:].sum() for t in range(v)]) / ZA      # the spans of A with i <= t <= j
    incl = np.clip(incl, 0.0, 1.0)
    gain = h2_64(incl)
    qp = int(np.argmax(gain))                                       # the first maximal frame
    return dict(status=LIVE, incl=incl, gain=gain, query_point=qp, query_gain=float(gain[qp]), post_entropy=H, agree=float(ZA / Z),
                Z=Z, ZA=ZA)


def chain_rule_residual(ps, pe, v, aps):
    """max over t < v of |H_A - [q H_{A, t pos} + (1 - q) H_{A, t neg}] - h2(q(t))|: the information the answer at t carries about the
    span is the entropy of the answer.  Both branches are enumerated as regions of the matrix: the spans that hold t, [0, t] x [t, v);
    the spans that end before t and the spans that start after it."""
    W, LG = weights(ps, pe, v)
    ok = consistent(v, aps)
    WA = np.where(ok, W, 0.0)
    with np.errstate(invalid='ignore'):
        WL = np.where(WA > 0, WA * LG, 0.0)

    def entropy(blocks):
        z = sum(WA[b].sum() for b in blocks)
        return z, (float(np.log2(z) - sum(WL[b].sum() for b in blocks) / z) if z > 0 else 0.0)
    ZA, H = entropy([np.s_[:, :]])
    worst = 0.0
    for t in range(v):
        zp, hp = entropy([np.s_[:t + 1, t:]])
        zn, hn = entropy([np.s_[:t, :t], np.s_[t + 1:, t + 1:]])
        q = zp / ZA
        worst = max(worst, abs((H - (q * hp + (zn / ZA) * hn)) - float(h2_64(q))))
    return worst


def set_ref(s_logits, e_logits, vlen, tlen, aps):
    """a whole set: s / e logits [N, ld] (torch or numpy), vlen / tlen [N], aps: per sample a list of (frame, is_pos) -> the list of
    posterior_ref dicts.  Row n is read as the tlen[n] first columns; v = vlen clamped to [0, tlen]."""
    s = torch.as_tensor(s_logits, dtype=torch.float32).cpu()
    e = torch.as_tensor(e_logits, dtype=torch.float32).cpu()
    out = []
    for n in range(s.shape[0]):
        T = int(tlen[n])
        ps, pe, v, _ = R.probabilities(s[n:n + 1, :T], e[n:n + 1, :T], torch.as_tensor([int(vlen[n])]))
        v = int(v[0])
        nan = bool(torch.isnan(s[n, :v]).any() or torch.isnan(e[n, :v]).any())
        out.append(posterior_ref(ps[0], pe[0], v, aps[n], nan_logit=nan))
    return out


@functools.lru_cache(maxsize=None)
def case(T):
    """the seeded case of length T the CPU and GPU tests share: 16 rows of N(0, sigma = 2) logits clipped to |x| <= 8, rows 8.. shorter
    than T, one ground-truth span per row, and for every history length h in HISTORIES the active points after h truthful answers at the
    reference's own query frame (fewer once the posterior has collapsed) with the reference of that state.
    -> dict(s, e [16, T] torch; vlen [16]; gt [16, 2]; ps, pe; aps {h: per-row lists}; ref {h: per-row dicts}; steps: per row the
    dicts of every state 0..6 in order)"""
    g = torch.Generator().manual_seed(4100 + T)
    s = (torch.randn(N_ROWS, T, generator=g) * 2).clamp(-8, 8)
    e = (torch.randn(N_ROWS, T, generator=g) * 2).clamp(-8, 8)
    vl = torch.full((N_ROWS,), T, dtype=torch.int32)
    vl[N_ROWS // 2:] = torch.randint(1, T, (N_ROWS // 2,), generator=g, dtype=torch.int32)
    vl[N_ROWS // 2] = 1
    ps, pe, v, _ = R.probabilities(s, e, vl)
    rng = np.random.default_rng(4100 + T)
    gt = np.zeros((N_ROWS, 2), dtype=np.int64)
    aps = {h: [] for h in HISTORIES}
    ref = {h: [] for h in HISTORIES}
    steps = []
    for n in range(N_ROWS):
        a = int(rng.integers(0, v[n]))
        gt[n] = a, int(rng.integers(a, v[n]))
        cur, states = [], []
        for h in range(max(HISTORIES) + 1):
            r = posterior_ref(ps[n], pe[n], int(v[n]), cur)
            states.append(r)
            if h in HISTORIES:
                aps[h].append(list(cur))
                ref[h].append(r)
            if r['status'] == LIVE and r['query_gain'] > 0:
                cur = cur + [(r['query_point'], answer(gt[n], r['query_point']))]
        steps.append(states)
    return dict(s=s, e=e, vlen=vl, v=v, gt=gt, ps=ps, pe=pe, aps=aps, ref=ref, steps=steps)
