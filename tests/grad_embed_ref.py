"""Reference of hual_al_grad_embed (include/hual_seqpan.h) for the tests: the contract restated in float64 numpy, with the error bars
of the float32 launch worked out beside every value.

u = 2^-24.  The bars (from the contract's arithmetic; not tuned):
  desc     per column c: (T + 8) u sum_t (p(t) + y(t)) |h(t, c)| - at most T roundings of the running float32 sum, each below u times
           the sum of the absolute terms, and 8 u for the weights: the masked softmax's few ulp and the one rounding of p - 1.
  gnorm2   |g'^2 - g^2| <= 2 |g| bar + bar^2 per column, summed (the float64 sum itself adds nothing visible), plus 2 u of the value for
           the final rounding to float32.
  egl      the launch takes d' = float32(h - mu') with |mu' - mu| <= bar_mu (desc's bar without y): |d' - d| <= eps = bar_mu +
           u (|d| + bar_mu).  p' d'^2 against p d^2: p (2 |d| eps + eps^2) + 8 u p d^2 per frame and column, summed in float64, plus 2 u
           of the value for the final rounding."""
import numpy as np

U = 2.0 ** -24
H = 128


def softmax(z):
    z = np.asarray(z, dtype=np.float64)
    e = np.exp(z - z.max())
    return e / e.sum()


def head(h, z, v, y):
    """one head of one sample: h [T, 128], z [>= v] logits, v frames, y the hypothesised frame (outside [0, v): none)
    -> dict(g, mu, egl, p, abs_g = sum_t (p + y) |h|, abs_mu = sum_t p |h|, d = h - mu)"""
    h = np.asarray(h, dtype=np.float64)[:v]
    p =softmax(np.asarray(z, dtype=np.float64)[:v])
    onehot = np.zeros(v)
    if 0 <= y < v:
        onehot[y] = 1.0
    mu = p @ h
    g = (p - onehot) @ h
    d = h - mu[None, :]
    egl = float((p[:, None] * d * d).sum())
    return dict(g=g, mu=mu, egl=egl, p=p, abs_g=(p + onehot) @ np.abs(h), abs_mu=p @ np.abs(h), d=d)


def embed(hs, he, zs, ze, v_len, hyp, T):
    """hs / he [B * T, 128], zs / ze [B, >= T], v_len [B], hyp [B, 2] -> dict of desc [B, 256], desc_bar [B, 256], gnorm2 [B],
    gnorm2_bar [B], egl [B], egl_bar [B], poisoned bool [B]; a poisoned row holds NaN / -1 and zero bars"""
    B = len(v_len)
    hs = np.asarray(hs, dtype=np.float64).reshape(B, T, H)
    he = np.asarray(he, dtype=np.float64).reshape(B, T, H)
    out = dict(desc=np.full((B, 2 * H), np.nan), desc_bar=np.zeros((B, 2 * H)), gnorm2=np.full(B, -1.0), gnorm2_bar=np.zeros(B),
               egl=np.full(B, -1.0), egl_bar=np.zeros(B), poisoned=np.zeros(B, dtype=bool))
    for b in range(B):
        v = min(max(int(v_len[b]), 0), T)
        if v < 1 or not (np.isfinite(np.asarray(zs[b][:v], dtype=np.float64)).all() and np.isfinite(np.asarray(ze[b][:v], dtype=np.float64)).all()):
            out['poisoned'][b] = True
            continue
        gn = gn_bar = egl = egl_bar = 0.0
        for k, (h, z) in enumerate(((hs[b], zs[b]), (he[b], ze[b]))):
            r = head(h, z, v, int(hyp[b][k]))
            bar = (T + 8) * U * r['abs_g']
            out['desc'][b, k * H:(k + 1) * H] = r['g']
            out['desc_bar'][b, k * H:(k + 1) * H] = bar
            gn += float((r['g'] ** 2).sum())
            gn_bar += float((2 * np.abs(r['g']) * bar + bar ** 2).sum())
            bar_mu = (T + 8) * U * r['abs_mu']
            ad = np.abs(r['d'])
            eps = bar_mu[None, :] + U * (ad + bar_mu[None, :])
            egl += r['egl']
            egl_bar += float((r['p'][:, None] * (2 * ad * eps + eps ** 2 + 8 * U * ad ** 2)).sum())
        out['gnorm2'][b], out['gnorm2_bar'][b] = gn, gn_bar + 2 * U * gn
        out['egl'][b], out['egl_bar'][b] = egl, egl_bar + 2 * U * egl
    return out


def egl_by_enumeration(h, z, v):
    """sum_t p(t) |g(onehot_t)|^2: the expectation of the squared gradient length over y ~ p, term by term"""
    p = softmax(np.asarray(z, dtype=np.float64)[:v])
    return float(sum(p[t] * (head(h, z, v, t)['g'] ** 2).sum() for t in range(v)))
