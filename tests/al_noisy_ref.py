"""Reference of hual_al_noisy_tilt and hual_al_label_gain_noisy (include/hual_seqpan.h) for the tests: the contract restated on the CPU.

The tilt is restated in numpy float32 operation by operation (one product, one subtraction or addition, each rounded on its own): the
kernel has to reproduce every bit.  Everything else is float64 and brute force:
  - the DIRECT noisy posterior: the weights w(i,j) = p_s[i] * p_e[j] of the untilted float32 probabilities times the product over the
    answers of (1 - eps where the answer agrees with the span, eps where not), span by span in the log domain - no G, no tilt - and its
    evidence ln(sum of those) - ln Z;
  - the TILTED posterior: the weights of the float32 probabilities of the tilted rows over the whole triangle, which is what the launches
    of the family compute from those rows and a set without answers (al_query_ref / al_label_ref / soft_label_ref with no active point);
  - the noisy label gain: the IoU of every pair of spans of the triangle, and per frame t the two re-weighted sums and their maxima over
    every candidate span - no prefix or suffix sum, no region, so the kernel's clamped factorisation is checked against the definition.

Also here: the seeded noisy cases the CPU and GPU tests share - al_query_ref.case(T) with its truthful answers flipped at rate 0.3 -
each computed once."""
import functools

import numpy as np
import torch

import al_gain_ref as G
import al_label_ref as L
import al_query_ref as Q
import soft_label_ref as S
import span_topk_ref as R

POISONED, LIVE = Q.POISONED, Q.LIVE
HISTORIES = (1, 3, 6)         # answers given before the posterior is read (al_query_ref's histories that hold an answer)
EPS = (0.05, 0.2)
FLIP_RATE, FLIP_SEED = 0.3, 9100
ROWS = G.ROWS                 # the rows of the case the all-frames gain tests evaluate


def eps64(eps):
    """eps as the C entry point reads it: the float32 argument widened to float64"""
    return float(np.float32(eps))


def lam32(eps):
    """(float)log((1.0 - (double)eps) / (double)eps)"""
    e = eps64(eps)
    return np.float32(np.log((1.0 - e) / e))


def counts(v, aps):
    """G [v + 1] int: G[t + 1] = (positive answers at frames <= t) - (negative answers at frames <= t), G[0] = G(-1) = 0; points
    outside [0, v) are ignored, duplicates count once each"""
    d = np.zeros(v + 1, dtype=np.int64)
    for f, is_pos in aps:
        if 0 <= f < v:
            d[f + 1] += 1 if is_pos else -1
    return np.cumsum(d)


def tilt_row(s0, e0, v, aps, eps):
    """one row's first v columns, float32, operation by operation: (s_t, e_t)"""
    lam = lam32(eps)
    g = counts(v, aps)
    gm, gc = g[:v].astype(np.float32), g[1:v + 1].astype(np.float32)
    s0, e0 = np.asarray(s0[:v], dtype=np.float32), np.asarray(e0[:v], dtype=np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        s = (s0 - (gm * lam).astype(np.float32)).astype(np.float32)
        e = (e0 + (gc * lam).astype(np.float32)).astype(np.float32)
    copy = np.float32(lam) == 0                                       # where the count or lam is 0 the logit is copied
    return np.where((gm == 0) | copy, s0, s), np.where((gc == 0) | copy, e0, e)


def tilt_set(s0, e0, vlen, tlen, aps, eps, poisoned=()):
    """a whole set [N, ld] (numpy float32): columns [0, v) of a live row tilted, everything else the input; `poisoned`: the rows the
    kernel copies raw"""
    s_t, e_t = np.array(s0, dtype=np.float32), np.array(e0, dtype=np.float32)
    for n in range(s_t.shape[0]):
        T = int(tlen[n])
        v = min(max(int(vlen[n]), 0), T)
        if n in poisoned or v < 1 or T > 256:
            continue
        s_t[n, :v], e_t[n, :v] = tilt_row(s_t[n], e_t[n], v, aps[n], eps)
    return s_t, e_t


def probabilities(s_row, e_row, v):
    """the float32 probabilities of one row's first v frames (span_topk_ref.probabilities, bit for bit the kernels')"""
    s = torch.as_tensor(np.asarray(s_row, dtype=np.float32))[None, :]
    e = torch.as_tensor(np.asarray(e_row, dtype=np.float32))[None, :]
    ps, pe, vv, _ = R.probabilities(s, e, torch.as_tensor([int(v)]))
    return ps[0], pe[0]


def log_likelihood(v, aps, eps):
    """[v, v] float64: the sum over the answers inside [0, v) of ln(1 - eps) where the answer agrees with the span (i, j), ln(eps) where
    not - answer by answer, span by span"""
    e = eps64(eps)
    ii, jj = np.indices((v, v))
    ll = np.zeros((v, v))
    for f, is_pos in aps:
        if 0 <= f < v:
            inside = (ii <= f) & (f <= jj)
            ll += np.where(inside == bool(is_pos), np.log1p(-e), np.log(e))
    return ll


def direct(ps, pe, v, aps, eps):
    """the direct noisy posterior of one row from its UNTILTED probabilities: dict(P [v, v] float64 (0 below the diagonal),
    log_evidence)"""
    W, _ = Q.weights(ps, pe, v)
    tri = np.triu(np.ones((v, v), dtype=bool))
    with np.errstate(divide='ignore'):
        lw = np.where(tri, np.log(W), -np.inf) + log_likelihood(v, aps, eps)
    top = lw[tri].max()
    x = np.where(tri, np.exp(lw - top), 0.0)
    tot = x[tri].sum()
    return dict(P=x / tot, log_evidence=float(top + np.log(tot) - np.log(W[tri].sum())))


def tilted(ps_t, pe_t, v):
    """the posterior the family's launches read from the tilted rows: P [v, v] float64 over the whole triangle"""
    W, _ = Q.weights(ps_t, pe_t, v)
    return W / W[np.triu(np.ones((v, v), dtype=bool))].sum()


def marginals_of(P):
    return P.sum(axis=1), P.sum(axis=0)


def noisy_gain_ref(ps_t, pe_t, v, eps, frames=None, nan_logit=False):
    """one row's tilted probabilities -> dict(status, value = V0, frames = the evaluated frames in order, gain [v] (0 at a frame not
    evaluated), raw [v] (before the clamp; nan where not evaluated), ask_point, ask_gain, margin = the best gain minus the second best
    over the other evaluated frames (inf with fewer than two)).  frames: the candidate list (entries outside [0, v) are skipped), None =
    every frame.  A poisoned row: ask_point -1, ask_gain = value = -1.0."""
    st = L.state(ps_t, pe_t, v, [], nan_logit)
    if st['status'] != LIVE:
        return dict(status=st['status'], value=-1.0, frames=[], gain=np.zeros(max(v, 0)), ask_point=-1, ask_gain=-1.0, margin=np.inf)
    e = eps64(eps)
    ev = [int(t) for t in (range(v) if frames is None else frames) if 0 <= t < v]
    ai, aj, w = st['ai'], st['aj'], st['w']
    iou = G.pair_iou(ai, aj, ai, aj)                                   # every candidate against every span of the triangle
    Z = st['Z']
    V0 = float((iou @ w).max() / Z)
    gain, raw = np.zeros(v), np.full(v, np.nan)
    for t in ev:
        holds = (ai <= t) & (t <= aj)
        f_in, f_out = iou @ np.where(holds, w, 0.0), iou @ np.where(holds, 0.0, w)
        raw[t] = (((1.0 - e) * f_in + e * f_out).max() + (e * f_in + (1.0 - e) * f_out).max()) / Z - V0
        gain[t] = min(max(raw[t], 0.0), 1.0)
    out = dict(status=LIVE, value=V0, frames=ev, gain=gain, raw=raw, ask_point=-1, ask_gain=0.0, margin=np.inf)
    if ev:
        g = gain[ev]
        k = int(np.argmax(g))                                           # the first evaluated frame of maximal gain
        out.update(ask_point=ev[k], ask_gain=float(g[k]), margin=float(g[k] - np.delete(g, k).max()) if len(ev) > 1 else np.inf)
    return out


def by_index(r):
    """is this state one whose ask_point the kernel has to reproduce exactly: a gain to be had, and a runner-up ten bars below it"""
    return r['status'] == LIVE and r['ask_gain'] > 1e-9 and r['margin'] > 1e-5


def flip(aps, rng, rate=FLIP_RATE):
    """every answer flipped with probability `rate`"""
    return [(f, bool(p) != bool(rng.random() < rate)) for f, p in aps]


@functools.lru_cache(maxsize=None)
def case(T):
    """al_query_ref.case(T) with, per history h in HISTORIES, naps[h][n] = its truthful answers flipped at rate FLIP_RATE by a seeded
    generator (drawn in the order h, n, answer), and hard[h][n] = al_query_ref.posterior_ref of those answers under the hard rule"""
    c = Q.case(T)
    rng = np.random.default_rng(FLIP_SEED + T)
    naps = {h: [flip(c['aps'][h][n], rng) for n in range(Q.N_ROWS)] for h in HISTORIES}
    hard = {h: [Q.posterior_ref(c['ps'][n], c['pe'][n], int(c['v'][n]), naps[h][n]) for n in range(Q.N_ROWS)] for h in HISTORIES}
    return dict(c, naps=naps, hard=hard)


@functools.lru_cache(maxsize=None)
def tilted_case(T, eps):
    """case(T) tilted by eps: per history s_t, e_t float32 [16, T] (numpy restatement), pst / pet = their float32 probabilities per
    row, and dir[h][n] = direct(...) of the row from the untilted probabilities"""
    c = case(T)
    s0, e0 = c['s'].numpy(), c['e'].numpy()
    out = dict(c, s_t={}, e_t={}, pst={}, pet={}, dir={})
    for h in HISTORIES:
        out['s_t'][h], out['e_t'][h] = tilt_set(s0, e0, c['vlen'].numpy(), [T] * Q.N_ROWS, c['naps'][h], eps)
        pp = [probabilities(out['s_t'][h][n], out['e_t'][h][n], int(c['v'][n])) for n in range(Q.N_ROWS)]
        out['pst'][h], out['pet'][h] = [p[0] for p in pp], [p[1] for p in pp]
        out['dir'][h] = [direct(c['ps'][n], c['pe'][n], int(c['v'][n]), c['naps'][h][n], eps) for n in range(Q.N_ROWS)]
    return out


@functools.lru_cache(maxsize=None)
def gain_case(T, eps):
    """tilted_case(T, eps), T in ROWS, with gref[h][n] = noisy_gain_ref over every frame of row n (None outside ROWS[T]), qref / lref /
    mref[h][n] = al_query_ref.posterior_ref / al_label_ref.label_ref / soft_label_ref.marginals_ref of the tilted row without answers"""
    c = tilted_case(T, eps)
    out = dict(c, gref={}, qref={}, lref={}, mref={})
    for h in HISTORIES:
        rows = [(c['pst'][h][n], c['pet'][h][n], int(c['v'][n])) for n in range(Q.N_ROWS)]
        out['gref'][h] = [noisy_gain_ref(*rows[n], eps) if n in ROWS[T] else None for n in range(Q.N_ROWS)]
        out['qref'][h] = [Q.posterior_ref(*rows[n], []) for n in range(Q.N_ROWS)]
        out['lref'][h] = [L.label_ref(*rows[n], []) if n in ROWS[T] else None for n in range(Q.N_ROWS)]
        out['mref'][h] = [S.marginals_ref(*rows[n], []) for n in range(Q.N_ROWS)]
    return out


def many_answers(v, n_answers=64, seed=77):
    """a history of n_answers clicks on one clip of v frames: a ground-truth span, frames drawn at random (duplicates included), every
    answer truthful but flipped at rate FLIP_RATE"""
    rng = np.random.default_rng(seed)
    a = int(rng.integers(0, v))
    gt = (a, int(rng.integers(a, v)))
    frames = rng.integers(0, v, n_answers)
    return flip([(int(f), Q.answer(gt, int(f))) for f in frames], rng)


# ---------------------------------------------------------------------------------------------------------------------
# the synthetic label-update set of the tests: 32 records of 33 frames that earlier rounds left with truthful answers at both ends of
# the ground truth (so the consistent set is what lies around that hull), ranked by a recorded prop_conf - the selection is known on
# the CPU and is the same half every round -, and an annotator who errs on 30 % of the answers
ROUND_N, ROUND_T, ROUND_FLIP, ROUND_SEED, ROUNDS = 32, 33, 0.3, 13, 3


@functools.lru_cache(maxsize=None)
def round_set():
    """dict(prop = the records (vid, v_len, prop_logits / 1 / 2, prop_conf), data_gt, data_old (with the earlier answers), vlen, gt
    [N, 2], sel = the half update_labels(rank_by='span_risk') selects): clips of 12-33 frames whose duration is v_len - 1 seconds, so a
    time in whole seconds is its own frame index"""
    g = torch.Generator().manual_seed(5200)
    rng = np.random.default_rng(5200)
    prop, data_gt, data_old, gt = [], [], [], np.zeros((ROUND_N, 2), dtype=np.int64)
    vlen = rng.integers(12, ROUND_T + 1, ROUND_N)
    conf = rng.permutation(ROUND_N) / float(ROUND_N)                  # distinct: the ranking by span risk has no ties
    for n in range(ROUND_N):
        lg = [(torch.randn(2, ROUND_T, generator=g) * 2).clamp(-8, 8).numpy() for _ in range(3)]
        v = int(vlen[n])
        a = int(rng.integers(0, v - 4))
        b = int(rng.integers(a + 3, v))
        oa = int(rng.integers(0, v))
        ob = int(rng.integers(oa, v))
        gt[n] = a, b
        prop.append({'vid': 'v%d' % n, 'v_len': v, 'prop_logits': (lg[0][0], lg[0][1]), 'prop_logits1': (lg[1][0], lg[1][1]),
                     'prop_logits2': (lg[2][0], lg[2][1]), 'prop_conf': float(conf[n])})
        data_gt.append(['v%d' % n, float(v - 1), [float(a), float(b)], 'a b'])
        data_old.append(['v%d' % n, float(v - 1), [float(oa), float(ob)], 'a b', {'pos_idx': [a, b], 'neg_idx': []}])
    sel = np.argsort(1.0 - conf, kind='stable')[:(ROUND_N + 1) // 2]
    return dict(prop=prop, data_gt=data_gt, data_old=data_old, vlen=vlen, gt=gt, sel=sel)


def replay_hard_rounds(asked, flipped):
    """the answers of ROUNDS label updates on round_set() under the HARD rule, given what was asked: asked[k] int [N] the frame every
    selected sample was asked about in round k, flipped[k] bool [N] whether the annotator erred -> per round the sorted selected rows
    whose answers so far leave no consistent span (al_query_ref.posterior_ref: contradictory), which renew_by='posterior' has to hand
    to the reference's renew"""
    S = round_set()
    pp = [probabilities(p['prop_logits'][0], p['prop_logits'][1], p['v_len']) for p in S['prop']]
    aps = [[(int(S['gt'][n, 0]), True), (int(S['gt'][n, 1]), True)] for n in range(ROUND_N)]
    out = []
    for k in range(len(asked)):
        for i in S['sel']:
            t = int(asked[k][i])
            aps[i] = aps[i] + [(t, Q.answer(S['gt'][i], t) != bool(flipped[k][i]))]
        out.append(sorted(int(i) for i in S['sel']
                          if Q.posterior_ref(pp[i][0], pp[i][1], int(S['vlen'][i]), aps[i])['status'] == Q.CONTRADICTORY))
    return out


def annotator_flips(rounds=ROUNDS):
    """flipped[k] bool [N] of annotator_flip=(ROUND_FLIP, default_rng(ROUND_SEED)) carried through `rounds` updates: one draw per
    selected sample, in selection order"""
    S = round_set()
    rng = np.random.default_rng(ROUND_SEED)
    out = []
    for _ in range(rounds):
        f = np.zeros(ROUND_N, dtype=bool)
        for i in S['sel']:
            f[i] = rng.random() < ROUND_FLIP
        out.append(f)
    return out


