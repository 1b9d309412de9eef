"""Reference of hual_al_ensemble_query and hual_al_ensemble_label (include/hual_seqpan.h) for the tests: the contract restated in
float64 on the CPU, by enumeration.

Per row and pass the probabilities are span_topk_ref.probabilities (float32, bit for bit the kernels').  Everything from there on is
float64 and brute force over [v, v] matrices: pass k's weights w_k(i,j) = p_s,k[i] * p_e,k[j] on the triangle are multiplied, span by
span, with the likelihood of the answers - the hard indicator of the consistent set, or under an annotator who errs the product over the
answers of (1 - eps where the answer agrees with the span, eps where not), factor by factor, no logarithm, no tilt.  A pass's evidence is
the sum of that product over its Z; the weights, the mixture, q(t), the marginals, both entropies, the expected tIoU of every member of
A and its argmax are sums over matrix entries.  No prefix or suffix sum, no segment, no region, no G: nothing of the kernels' algebra.

Also here: the seeded cases the CPU and GPU tests share, each computed once."""
import functools
import math

import numpy as np
import torch

import al_query_ref as Q
import span_topk_ref as R

POISONED, CONTRADICTORY, LIVE = Q.POISONED, Q.CONTRADICTORY, Q.LIVE
N_ROWS = Q.N_ROWS
PASS_SIGMA = 0.7              # the spread of a stochastic pass's logits around the deterministic ones
PAIR_CHUNK = 4_000_000        # IoU entries held at once while R(a, e) of every member is enumerated


def likelihood(v, aps, eps=None):
    """[v, v] float64 on the triangle (0 below the diagonal): the probability of the answers inside [0, v) given the span (i, j) - the
    indicator of the consistent set, or with eps the product over the answers of (1 - eps | eps)"""
    ii, jj = np.indices((v, v))
    lik = (ii <= jj).astype(np.float64)
    eps = None if eps is None else float(np.float32(eps))          # as the C entry point reads it: a float32 widened
    for f, is_pos in aps:
        if not 0 <= f < v:
            continue
        agrees = ((ii <= f) & (f <= jj)) == bool(is_pos)
        lik = lik * (np.where(agrees, 1.0, 0.0) if eps is None else np.where(agrees, 1.0 - eps, eps))
    return lik


def entropy_bits(P):
    p = P[P > 0]
    return float(-(p * np.log2(p)).sum())


def iou_against(a, e, v):
    """[v, v] float64: the frame-count IoU of the span (a, e) with every span (i, j)"""
    ii, jj = np.indices((v, v))
    inter = np.maximum(0, np.minimum(e, jj) + 1 - np.maximum(a, ii))
    union = (e - a + 1) + (jj - ii + 1) - inter
    return np.where(union > 0, inter / np.maximum(union, 1), 0.0)


def expected_iou_of(ma, me, si, sj, p):
    """R [len(ma)] float64: sum over the spans (si, sj) of mass p of the frame-count IoU with each candidate (ma, me) - every pair of
    (candidate, span) is formed, PAIR_CHUNK of them at a time"""
    out = np.zeros(len(ma))
    step = max(1, PAIR_CHUNK // max(1, len(si)))
    for lo in range(0, len(ma), step):
        a, e = ma[lo:lo + step, None], me[lo:lo + step, None]
        inter = np.maximum(0, np.minimum(e, sj[None, :]) + 1 - np.maximum(a, si[None, :]))
        union = (e - a + 1) + (sj - si + 1)[None, :] - inter
        out[lo:lo + step] = (inter / union) @ p
    return out


def ensemble_ref(ps, pe, v, aps, logw=None, nan_logit=False, eps=None, old=None, label=True):
    """one row under K passes: ps / pe lists of K float32 arrays, aps its answers, logw None or K floats, eps None (the hard rule) or the
    annotator's error rate, old None or the old span -> dict(status, weight [K], log_evidence, incl [v], gain [v], query_point,
    query_gain, runner_gain (the best gain at another frame; -inf with one frame), y_start [v], y_end [v], post_entropy,
    expected_entropy, bald_raw (before the clamp), span_bald, P [v, v] the mixture, Pk the passes' posteriors, and with label=True:
    new_idx, conf, runner_conf (the best R of another member; -inf with one member), members, old_conf)"""
    K = len(ps)
    z = np.zeros(max(v, 0))
    flag = dict(weight=np.zeros(K), incl=z, gain=z, y_start=z, y_end=z, query_point=-1, query_gain=-1.0, post_entropy=-1.0,
                expected_entropy=-1.0, span_bald=-1.0, new_idx=(-1, -1), conf=-1.0, old_conf=-1.0)
    if v < 1 or nan_logit:
        return dict(flag, status=POISONED, log_evidence=float('nan'))
    tri = np.triu(np.ones((v, v), dtype=bool))
    lik = likelihood(v, aps, eps)
    Wk = [np.triu(np.outer(ps[k][:v].astype(np.float64), pe[k][:v].astype(np.float64))) for k in range(K)]
    Zk = [W[tri].sum() for W in Wk]
    # passes whose factor rows are equal bit for bit are ONE component of the mixture, with the sum of their weights
    group = [min(j for j in range(K) if np.array_equal(ps[j][:v], ps[k][:v]) and np.array_equal(pe[j][:v], pe[k][:v])) for k in range(K)]
    if any(not (Z > 0 and np.isfinite(Z)) for Z in Zk):
        return dict(flag, status=POISONED, log_evidence=float('nan'))
    Ek = [(Wk[k] * lik)[tri].sum() for k in range(K)]             # pass k's evidence of the answers, times Z_k
    lw = np.zeros(K) if logw is None else np.asarray(logw, dtype=np.float64)
    with np.errstate(divide='ignore'):
        u = np.array([np.log(Ek[k] / Zk[k]) + lw[k] if Ek[k] > 0 else -np.inf for k in range(K)])
    if not np.isfinite(u.max()):
        return dict(flag, status=CONTRADICTORY, log_evidence=-np.inf)
    x = np.exp(u - u.max())
    w = x / x.sum()
    log_evidence = float(u.max() + np.log(x.sum()) - np.log(K))
    Pk = [Wk[k] * lik / Ek[k] if Ek[k] > 0 else np.zeros((v, v)) for k in range(K)]
    comp = sorted(set(group))                                     # ascending k
    wc = {g: math.fsum(w[k] for k in range(K) if group[k] == g) for g in comp}
    P = np.zeros((v, v))
    for g in comp:
        P = P + wc[g] * Pk[g]
    incl = np.clip(np.array([P[:t + 1, t:].sum() for t in range(v)]), 0.0, 1.0)
    gain = Q.h2_64(incl)
    qp = int(np.argmax(gain))
    Hk = [entropy_bits(Pk[k]) for k in range(K)]
    ee = float(sum(wc[g] * Hk[g] for g in comp if wc[g] > 0))
    hm = entropy_bits(P)
    out = dict(status=LIVE, weight=w, log_evidence=log_evidence, incl=incl, gain=gain, query_point=qp, query_gain=float(gain[qp]),
               runner_gain=float(np.delete(gain, qp).max()) if v > 1 else -np.inf, y_start=P.sum(axis=1), y_end=P.sum(axis=0),
               post_entropy=hm, expected_entropy=ee, bald_raw=hm - ee, span_bald=max(0.0, hm - ee), P=P, Pk=Pk, Hk=Hk)
    if label:
        mem = np.argwhere(lik > 0) if eps is None else np.argwhere(tri)      # the members of A, row-major
        sup = np.argwhere(P > 0)                                  # the spans that carry mass
        Rm = expected_iou_of(mem[:, 0], mem[:, 1], sup[:, 0], sup[:, 1], P[P > 0])
        b = int(np.argmax(Rm))                                    # the first maximal member in row-major order
        out.update(new_idx=(int(mem[b, 0]), int(mem[b, 1])), conf=float(min(max(Rm[b], 0.0), 1.0)), members=mem, R=Rm,
                   runner_conf=float(np.delete(Rm, b).max()) if len(mem) > 1 else -np.inf)
    if old is not None:
        oa, oe = int(old[0]), int(old[1])
        ok = 0 <= oa <= oe < v
        out['old_conf'] = float(min(max((P * iou_against(oa, oe, v)).sum(), 0.0), 1.0)) if ok else -1.0
    return out


def probabilities(s, e, vlen):
    """s / e [N, T] float32 logits -> per row (p_s, p_e) float32 [T], v [N] and whether a logit below v is NaN"""
    s, e = torch.as_tensor(s, dtype=torch.float32), torch.as_tensor(e, dtype=torch.float32)
    ps, pe, v, _ = R.probabilities(s, e, torch.as_tensor(vlen, dtype=torch.int32))
    nan = [bool(torch.isnan(s[n, :int(v[n])]).any() or torch.isnan(e[n, :int(v[n])]).any()) for n in range(s.shape[0])]
    return ps, pe, v, nan


def passes_of(s, e, K, seed, sigma=PASS_SIGMA):
    """K stochastic passes around the logits s / e [N, T] (torch): [K, N, T] twice, seeded"""
    g = torch.Generator().manual_seed(seed)
    return (s[None] + sigma * torch.randn(K, *s.shape, generator=g)).contiguous(), (e[None] + sigma * torch.randn(K, *e.shape, generator=g)).contiguous()


def flip(aps, rng, rate):
    """every answer flipped with probability `rate`"""
    return [(f, bool(p) != bool(rng.random() < rate)) for f, p in aps]


# (T, K, answers per row, eps or None, logw given, extra columns beyond T).  Every T of al_query_ref.TS, every K of (1, 2, 5, 16), 0, 1,
# 3 and 6 answers, the hard rule and eps = 0.1 with a seeded 30 % of the answers flipped, logw NULL and given, ld > T in two cases.
CASES = ((2, 1, 0, None, False, 0), (33, 2, 1, None, True, 0), (70, 5, 3, None, False, 6), (256, 16, 6, None, True, 0),
         (70, 16, 0, None, False, 3), (256, 2, 6, None, False, 0), (33, 5, 3, 0.1, False, 0), (70, 2, 6, 0.1, True, 0),
         (33, 1, 6, 0.1, False, 0))
NOISE_EPS, FLIP_RATE = 0.1, 0.3


@functools.lru_cache(maxsize=None)
def case(T, K, h, eps, with_logw, pad):
    """one seeded case: al_query_ref.case(T)'s 16 rows (rows 8.. shorter than T, row 8 of one frame) as the deterministic logits, K
    passes around them, the row's h truthful answers (under eps: 30 % of them flipped, seeded), logw [K, N] or None, the old spans, and
    ref[n] = ensemble_ref of the row, the label of every row enumerated
    -> dict(T, K, ld, pass_s / pass_e [K, 16, ld] torch, vlen, v, aps, logw, old [16, 2], ps / pe per pass, ref)"""
    c = Q.case(T)
    seed = 7300 + 97 * T + 7 * K + h + (1000 if eps else 0)
    ss, ee = passes_of(c['s'], c['e'], K, seed)
    rng = np.random.default_rng(seed)
    aps = [list(a) for a in c['aps'][h]]
    if eps is not None:
        aps = [flip(a, rng, FLIP_RATE) for a in aps]
    logw = rng.normal(0.0, 1.0, (K, N_ROWS)).astype(np.float32) if with_logw else None
    v = [int(x) for x in c['v']]
    old = np.zeros((N_ROWS, 2), dtype=np.int32)
    for n in range(N_ROWS):
        a = int(rng.integers(0, v[n]))
        old[n] = a, int(rng.integers(a, v[n]))
    old[3] = (2, 1)                                                # not a span: old_conf -1
    pp = [probabilities(ss[k], ee[k], c['vlen']) for k in range(K)]
    ref = []
    for n in range(N_ROWS):
        ref.append(ensemble_ref([pp[k][0][n] for k in range(K)], [pp[k][1][n] for k in range(K)], v[n], aps[n],
                                logw=None if logw is None else logw[:, n], eps=eps, old=old[n]))
    ld = T + pad
    if pad:
        ss, ee = torch.nn.functional.pad(ss, (0, pad)), torch.nn.functional.pad(ee, (0, pad))
    return dict(T=T, K=K, ld=ld, pass_s=ss.contiguous(), pass_e=ee.contiguous(), vlen=c['vlen'], v=v, aps=aps, logw=logw, old=old,
                ps=[p[0] for p in pp], pe=[p[1] for p in pp], ref=ref, eps=eps)


def excused(refs, key_best, key_runner, margin):
    """the live rows whose index the kernel need not reproduce: the enumeration's runner-up lies within `margin` of its best"""
    return [n for n, r in enumerate(refs) if r['status'] == LIVE and key_best in r and r[key_best] - r[key_runner] < margin]


# ---------------------------------------------------------------------------------------------------------------------
# the edge rows: T = 33, K = 5, ld = 40, every row's passes around one seeded row of logits
EDGE_T, EDGE_K, EDGE_LD = 33, 5, 40
EDGE_ROWS = ('plain', 'nan_in_one_pass', 'too_long', 'contradictory', 'one_pass_underflows', 'collapsed', 'one_frame', 'all_underflow',
             'empty_clip', 'points_outside')


@functools.lru_cache(maxsize=None)
def edge_case():
    """dict(pass_s / pass_e [5, 10, 40] torch, vlen, tlen, aps, ref per row, names): the rows the contract names.  'too_long' is a row
    of tlen 300 in a set of ld 40 (the kernel refuses it by its length alone); 'one_pass_underflows': pass 2's start probabilities are 0
    on every start the answers allow, so its Z_A is 0 while the other passes live; 'all_underflow': every pass's are"""
    N, T, K = len(EDGE_ROWS), EDGE_T, EDGE_K
    g = torch.Generator().manual_seed(8800)
    s = (torch.randn(N, T, generator=g) * 2).clamp(-8, 8)
    e = (torch.randn(N, T, generator=g) * 2).clamp(-8, 8)
    ss, ee = passes_of(s, e, K, 8801)
    vlen = np.full(N, T, dtype=np.int32)
    tlen = np.full(N, T, dtype=np.int32)
    aps = [[] for _ in range(N)]
    ix = {name: i for i, name in enumerate(EDGE_ROWS)}
    aps[ix['plain']] = [(10, True), (25, False)]
    ss[3, ix['nan_in_one_pass'], 7] = float('nan')
    aps[ix['nan_in_one_pass']] = [(10, True)]
    tlen[ix['too_long']] = 300
    vlen[ix['too_long']] = 300
    aps[ix['contradictory']] = [(10, True), (20, True), (15, False)]
    aps[ix['one_pass_underflows']] = [(10, True), (3, False)]
    ss[2, ix['one_pass_underflows'], 4:11] = -200.0              # the starts (3, 10] of A: float32 probabilities exactly 0
    aps[ix['collapsed']] = [(5, True), (4, False), (6, False)]
    vlen[ix['one_frame']] = 1
    aps[ix['all_underflow']] = [(10, True), (3, False)]
    ss[:, ix['all_underflow'], 4:11] = -200.0
    vlen[ix['empty_clip']] = 0
    aps[ix['points_outside']] = [(-3, True), (40, False), (33, True), (12, True)]
    vlen[ix['points_outside']] = 20
    pad = EDGE_LD - T
    ssp, eep = torch.nn.functional.pad(ss, (0, pad)), torch.nn.functional.pad(ee, (0, pad))
    pp = [probabilities(ss[k], ee[k], np.minimum(vlen, T)) for k in range(K)]
    old = np.tile(np.array([[4, 12]], dtype=np.int32), (N, 1))
    ref = []
    for n in range(N):
        v = 0 if tlen[n] > 256 else min(max(int(vlen[n]), 0), T)
        ref.append(ensemble_ref([pp[k][0][n] for k in range(K)], [pp[k][1][n] for k in range(K)], v, aps[n],
                                nan_logit=any(pp[k][3][n] for k in range(K)), old=old[n]))
    return dict(T=T, K=K, ld=EDGE_LD, pass_s=ssp.contiguous(), pass_e=eep.contiguous(), vlen=vlen, tlen=tlen, aps=aps, ref=ref, old=old,
                names=ix)


# ---------------------------------------------------------------------------------------------------------------------
# the random row-states behind the README's finding: how often the ensemble asks another frame, or gives another label, than the
# deterministic pass
def disagreement(T=33, K=8, histories=(0, 1, 3, 6)):
    """-> (states, query frames that differ, labels that differ) over al_query_ref.case(T)'s live rows and histories, the passes seeded
    as in `case`; rows whose own runner-up is within 1e-5 bits / 1e-9 tIoU of its best on either side are left out of the count"""
    import al_label_ref as L
    c = Q.case(T)
    ss, ee = passes_of(c['s'], c['e'], K, 9900 + T)
    pp = [probabilities(ss[k], ee[k], c['vlen']) for k in range(K)]
    states = dq = dl = 0
    for h in histories:
        for n in range(N_ROWS):
            v = int(c['v'][n])
            det = c['ref'][h][n]
            if det['status'] != LIVE or v < 2:
                continue
            r = ensemble_ref([pp[k][0][n] for k in range(K)], [pp[k][1][n] for k in range(K)], v, c['aps'][h][n])
            if r['status'] != LIVE:
                continue
            lab = L.label_ref(c['ps'][n], c['pe'][n], v, c['aps'][h][n])
            states += 1
            dq += int(r['query_point'] != det['query_point'] and r['query_gain'] - r['runner_gain'] >= 1e-5)
            dl += int(tuple(r['new_idx']) != tuple(lab['label']))
    return states, dq, dl
