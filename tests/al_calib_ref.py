"""Reference of hual_al_evidence_grid (include/hual_seqpan.h) for the tests: the contract restated on the CPU in float64.

A cell (a, b) of one row: the row scaled in numpy float32 - one product per logit, as the kernel's -, al_noisy_ref.probabilities of the
scaled row (bit for bit the kernel's), and the triangle enumerated with the direct product of the answers' likelihoods:
  - cell_direct: al_noisy_ref.direct itself, span by span, answer by answer - the definition;
  - row_cells: the same enumeration for every eps of a grid at once.  The likelihood of the answers under a span depends on the span only
    through the number g of answers it agrees with, (1 - eps)^g eps^(n - g): the weights of the triangle are summed per g once (every
    span is still visited, no prefix sum, no G, no power of r) and each eps costs n + 1 terms.  tests/test_al_calib.py holds the two
    within 1e-12 of each other; the GPU tests need the second, whose cost does not grow with the grid.
Also here: the fold (totals and counts), the cases the CPU and GPU tests share - al_noisy_ref.case(T) with the history without answers
beside its three - and the planted set of the recovery test."""
import functools

import numpy as np

import al_noisy_ref as NR
import al_query_ref as Q
import span_topk_ref as R

HISTORIES = (0,) + NR.HISTORIES        # answers given before the evidence is read
TS = (2, 33, 70, 256)


def inv32(tau):
    """float32(1 / tau): what LabelUpdater hands the launch for a temperature"""
    return np.float32(1.0 / float(tau))


def scale(x, inv_tau):
    """x * inv_tau in float32, one product rounded on its own"""
    with np.errstate(invalid='ignore', over='ignore'):
        return (np.asarray(x, dtype=np.float32) * np.float32(inv_tau)).astype(np.float32)


def counted(v, aps):
    """the answers inside [0, v)"""
    return [(int(f), bool(p)) for f, p in aps if 0 <= f < v]


def cell_direct(s_row, e_row, v, aps, inv_tau, eps):
    """one cell of one row by al_noisy_ref.direct: float64, NaN where the cell is poisoned, 0 without a counted answer"""
    s, e = np.asarray(s_row, dtype=np.float32)[:max(v, 0)], np.asarray(e_row, dtype=np.float32)[:max(v, 0)]
    if v < 1 or np.isnan(s).any() or np.isnan(e).any():
        return float('nan')
    ps, pe = NR.probabilities(scale(s, inv_tau), scale(e, inv_tau), v)
    W, _ = Q.weights(ps, pe, v)
    Z = W[np.triu(np.ones((v, v), dtype=bool))].sum()
    if not (Z > 0.0 and np.isfinite(Z)):
        return float('nan')
    if not counted(v, aps):
        return 0.0
    return NR.direct(ps, pe, v, aps, eps)['log_evidence']


@functools.lru_cache(maxsize=None)
def _triangle(v):
    return np.triu_indices(v)


def classes(v, aps):
    """per span of the triangle (row-major, i <= j) the number of counted answers it agrees with, and the number of counted answers"""
    ii, jj = _triangle(v)
    ans = counted(v, aps)
    agree = np.zeros(len(ii), dtype=np.int64)
    for f, is_pos in ans:
        agree += ((ii <= f) & (f <= jj)) == is_pos
    return agree, len(ans)


def row_cells(ps, pe, v, aps, eps_list, cls=None):
    """[B] float64: one row's cells at one temperature, from the float32 probabilities of the scaled row (cls: classes(v, aps), for a
    caller that evaluates several temperatures)"""
    B = len(eps_list)
    ii, jj = _triangle(v)
    w = ps[:v].astype(np.float64)[ii] * pe[:v].astype(np.float64)[jj]      # every span of the triangle: al_query_ref.weights
    Z = w.sum()
    if not (Z > 0.0 and np.isfinite(Z)):
        return np.full(B, np.nan)
    agree, n = classes(v, aps) if cls is None else cls
    if n == 0:
        return np.zeros(B)
    mass = np.bincount(agree, weights=w, minlength=n + 1)             # the weight of the spans that agree with g answers
    g = np.arange(n + 1)
    out = np.zeros(B)
    with np.errstate(divide='ignore'):
        lm = np.log(mass)
    for b, eps in enumerate(eps_list):
        e = NR.eps64(eps)
        lw = lm + g * np.log1p(-e) + (n - g) * np.log(e)
        top = lw.max()
        out[b] = top + np.log(np.exp(lw - top).sum()) - np.log(Z)
    return out


def set_table(s, e, vlen, tlen, aps, inv_taus, eps_list):
    """a whole set [N, ld] (numpy float32) -> (table float64 [N, A * B], status int [N], answers int [N] = the counted answers)"""
    s, e = np.asarray(s, dtype=np.float32), np.asarray(e, dtype=np.float32)
    N, ld = s.shape
    A, B = len(inv_taus), len(eps_list)
    table = np.full((N, A * B), np.nan)
    v = np.array([min(max(int(vlen[n]), 0), int(tlen[n])) if 1 <= int(tlen[n]) <= min(256, ld) else 0 for n in range(N)])
    ok = np.array([v[n] >= 1 and not (np.isnan(s[n, :v[n]]).any() or np.isnan(e[n, :v[n]]).any()) for n in range(N)])
    cls = [classes(int(v[n]), aps[n]) if ok[n] else None for n in range(N)]
    for a, k in enumerate(inv_taus):
        with np.errstate(invalid='ignore', over='ignore'):
            ps, pe, _, _ = R.probabilities(scale(s, k), scale(e, k), v)
        for n in range(N):
            if ok[n]:
                table[n, a * B:(a + 1) * B] = row_cells(ps[n], pe[n], int(v[n]), aps[n], eps_list, cls[n])
    status = np.isfinite(table).all(axis=1).astype(np.int64)
    answers = np.array([len(counted(int(v[n]), aps[n])) for n in range(N)])
    return table, status, answers


def fold(table, status, answers, sel=None):
    """(total [A * B], counts [4], scale [A * B] = the sum of |cell| over the summed rows: what the bars on a total are relative to)"""
    N = table.shape[0]
    ids = [int(i) for i in (range(N) if sel is None else sel) if 0 <= int(i) < N]
    live = [i for i in ids if status[i] == 1]
    total = table[live].sum(axis=0) if live else np.zeros(table.shape[1])
    scale_ = np.abs(table[live]).sum(axis=0) if live else np.zeros(table.shape[1])
    best = int(np.argmax(total)) if live else -1
    return total, np.array([len(live), int(answers[live].sum()) if live else 0, len(ids) - len(live), best]), scale_


def margin(total):
    """the best total minus the second best (inf with one cell)"""
    t = np.sort(np.asarray(total).reshape(-1))[::-1]
    return float(t[0] - t[1]) if t.size > 1 else float('inf')


@functools.lru_cache(maxsize=None)
def case(T):
    """al_noisy_ref.case(T) with naps[0] = no answers: dict(s, e torch [16, T], vlen, v, naps {h: per-row lists}, ...)"""
    c = NR.case(T)
    naps = dict(c['naps'])
    naps[0] = [[] for _ in range(Q.N_ROWS)]
    return dict(c, naps=naps)


GRIDS = {'1x1': ((1.0,), (0.1,)),
         '3x2': ((0.5, 1.0, 2.0), (0.05, 0.2)),
         '32x16': (tuple(2.0 ** (k / 8.0) for k in range(-16, 16)),
                   (1e-6, 1e-4, 0.001, 0.005, 0.01, 0.02, 0.03, 0.05, 0.075, 0.1, 0.15, 0.2, 0.25, 0.3, 0.4, 0.5))}


def grid(name):
    """(inv_tau float32 [A], eps float32 [B]) of a named grid (its temperatures as float32(1 / tau))"""
    taus, eps = GRIDS[name]
    return np.array([inv32(t) for t in taus], dtype=np.float32), np.array(eps, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def case_table(T, h, name):
    """(table, status, answers) of case(T) after history h on the named grid: computed once, shared"""
    c = case(T)
    it, ep = grid(name)
    return set_table(c['s'].numpy(), c['e'].numpy(), c['vlen'].numpy(), [T] * Q.N_ROWS, c['naps'][h], it, ep)


# ---------------------------------------------------------------------------------------------------------------------
# the planted set: rows whose span is drawn from the posterior at a known temperature and answered by an annotator who errs at a known
# rate - the fit has to find both
PLANT_T, PLANT_N, PLANT_ANSWERS = 33, 192, 6
PLANT_TAUS = tuple(2.0 ** (k / 2.0) for k in range(-4, 5))
PLANT_EPS = (0.01, 0.02, 0.05, 0.1, 0.2, 0.3, 0.4, 0.5)
PLANTED = ((2.0, 0.1, 3.0), (0.5, 0.2, 1.5))      # (tau*, eps*, scale)


@functools.lru_cache(maxsize=None)
def planted(tau, eps, scale_, seed):
    """dict(s, e float32 [N, T] = N(0, 1) * scale, vlen, tlen, gt [N, 2] drawn from the posterior of softmax(s / tau), softmax(e / tau),
    aps: per row PLANT_ANSWERS answers at distinct random frames, each flipped with probability eps)"""
    rng = np.random.default_rng(seed)
    s = (rng.standard_normal((PLANT_N, PLANT_T)) * scale_).astype(np.float32)
    e = (rng.standard_normal((PLANT_N, PLANT_T)) * scale_).astype(np.float32)
    v = np.full(PLANT_N, PLANT_T)
    ps, pe, _, _ = R.probabilities(scale(s, inv32(tau)), scale(e, inv32(tau)), v)
    ii, jj = np.triu_indices(PLANT_T)
    gt, aps = np.zeros((PLANT_N, 2), dtype=np.int64), []
    for n in range(PLANT_N):
        w = ps[n].astype(np.float64)[ii] * pe[n].astype(np.float64)[jj]
        k = int(rng.choice(len(w), p=w / w.sum()))
        gt[n] = ii[k], jj[k]
        frames = rng.choice(PLANT_T, PLANT_ANSWERS, replace=False)
        aps.append([(int(f), Q.answer(gt[n], int(f)) != bool(rng.random() < eps)) for f in frames])
    return dict(s=s, e=e, vlen=v.astype(np.int32), tlen=v.astype(np.int32), gt=gt, aps=aps)


def planted_records(p):
    """the planted set as the records LabelUpdater takes"""
    return [{'vid': 'v%d' % n, 'v_len': int(p['vlen'][n]), 'prop_logits': (p['s'][n], p['e'][n]), 'prop_logits1': (p['s'][n], p['e'][n]),
             'prop_logits2': (p['s'][n], p['e'][n])} for n in range(len(p['vlen']))]


def set_totals(p, taus, eps_list, rows=None):
    """the reference totals [A, B] of a set dict (s, e, vlen, tlen, aps) on the grid taus x eps_list, and the fold's counts and scale"""
    it = np.array([inv32(t) for t in taus], dtype=np.float32)
    table, status, answers = set_table(p['s'], p['e'], p['vlen'], p['tlen'], p['aps'], it, list(eps_list))
    total, counts, scale_ = fold(table, status, answers, rows)
    return total.reshape(len(taus), len(eps_list)), counts, scale_
