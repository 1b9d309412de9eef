"""Reference of hual_span_expected_iou (include/hual_seqpan.h) for the tests: the contract restated in float64 on the CPU.

The probabilities are span_topk_ref.probabilities (float32, bit for bit the kernel's); everything from there on - the weights
p_s[i] * p_e[j], Z, the IoU ratio, the sums, the logarithms - is float64, so the distance of the kernel's float32 steps from this
reference is what tests/test_gpu_span_conf.py bounds.  Candidates usually come from span_topk_ref.span_topk_ref or lib.span_topk."""
import numpy as np
import torch

import span_topk_ref as R
from span_clip_util import stable_order      # noqa: F401 (the tests reach it through this module)


def span_iou(a, b, ii, jj):
    """IoU of the frame span [a, b] with the spans [ii, jj] on the half-open intervals [i, j + 1) (float64)"""
    inter = np.maximum(0, np.minimum(b, jj) + 1 - np.maximum(a, ii))
    union = (b - a + 1) + (jj - ii + 1) - inter
    return inter.astype(np.float64) / union.astype(np.float64)


def span_weights(ps, pe, v):
    """(ii, jj, w) of the triangle 0 <= i <= j < v, w = p_s[i] * p_e[j] in float64"""
    ii, jj = np.triu_indices(v)
    return ii, jj, ps[:v].astype(np.float64)[ii] * pe[:v].astype(np.float64)[jj]


def distribution_ref(ps, pe, v, cands):
    """one clip from its probabilities: (expected IoU float64 per candidate (a, b), -1.0 for an invalid one; entropy in bits), or
    (all -1.0, -1.0) when Z is not a positive finite number"""
    ii, jj, w = span_weights(ps, pe, v)
    Z = w.sum()
    if not (Z > 0 and np.isfinite(Z)):
        return np.full(len(cands), -1.0), -1.0
    out = np.full(len(cands), -1.0)
    for q, (a, b) in enumerate(cands):
        if a < 0 or b < 0 or a > b or b >= v:
            continue
        out[q] = float((w * span_iou(int(a), int(b), ii, jj)).sum() / Z)
    nz = w > 0
    with np.errstate(divide='ignore'):
        lg = np.log2(ps[:v].astype(np.float64))[ii] + np.log2(pe[:v].astype(np.float64))[jj]
    H = np.log2(Z) - (w[nz] * lg[nz]).sum() / Z
    return out, max(0.0, float(H))


def span_conf_ref(s_logits, e_logits, vlen, starts, ends):
    """-> expected IoU float64 [B,k] (-1.0: invalid slot, empty or poisoned row), span entropy float64 [B] in bits (-1.0: empty or
    poisoned row), alive bool [B] (the rows a reorder may permute)"""
    ps, pe, v, _ = R.probabilities(s_logits, e_logits, vlen)
    s = torch.as_tensor(s_logits, dtype=torch.float32).cpu().numpy()
    e = torch.as_tensor(e_logits, dtype=torch.float32).cpu().numpy()
    st, en = np.asarray(starts, dtype=np.int64), np.asarray(ends, dtype=np.int64)
    B, k = st.shape
    ei = np.full((B, k), -1.0)
    ent = np.full(B, -1.0)
    alive = np.zeros(B, dtype=bool)
    for b in range(B):
        n = int(v[b])
        if n < 1 or np.isnan(s[b, :n]).any() or np.isnan(e[b, :n]).any():
            continue
        ei[b], ent[b] = distribution_ref(ps[b], pe[b], n, list(zip(st[b], en[b])))
        alive[b] = ent[b] >= 0
    return ei, ent, alive
