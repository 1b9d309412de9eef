"""Reference of hual_span_topk (include/hual_seqpan.h) for the tests: numpy / torch on the CPU, bit for bit the kernel's contract.

Probabilities: oracle.seqpan_ref.softmax_cr of mask_logits (the arithmetic of hual_span_argmax); candidates p_s[i] * p_e[j] in float32
for i <= j < vlen (j - i < max_len when max_len > 0), sorted by score descending and key i * 256 + j ascending; plain greedy NMS over
the whole sorted list, the overlap test in float32."""
import numpy as np
import torch

F32 = np.float32


def probabilities(s_logits, e_logits, vlen):
    """(p_s, p_e) float32 [B,T] and the clamped lengths [B] (vlen > T reads as T, < 1 as 0)"""
    from oracle.seqpan_ref import mask_logits, softmax_cr
    s = torch.as_tensor(s_logits, dtype=torch.float32).cpu()
    e = torch.as_tensor(e_logits, dtype=torch.float32).cpu()
    T = s.shape[1]
    v = torch.as_tensor(vlen).cpu().long().clamp(0, T)
    mask = torch.arange(T)[None, :] < v[:, None]
    # logits at t >= vlen are not read by the kernel: a finite stand-in makes mask_logits give exactly its -1e30 there
    s, e = torch.where(mask, s, torch.zeros_like(s)), torch.where(mask, e, torch.zeros_like(e))
    return softmax_cr(mask_logits(s, mask)).numpy(), softmax_cr(mask_logits(e, mask)).numpy(), v.numpy(), mask.numpy()


def candidates(ps, pe, v, max_len=0):
    """(i, j, score) of one clip in the contract's order"""
    ii, jj = np.triu_indices(v)
    if max_len > 0:
        keep = jj - ii < max_len
        ii, jj = ii[keep], jj[keep]
    sc = (ps[:v, None] * pe[None, :v]).astype(F32)[ii, jj]       # one float32 product each
    ok = ~np.isnan(sc)
    ii, jj, sc = ii[ok], jj[ok], sc[ok]
    order = np.lexsort((ii * 256 + jj, -sc))
    return ii[order], jj[order], sc[order]


def suppressed(si, sj, ii, jj, nms_iou):
    inter = np.maximum(0, np.minimum(sj, jj) + 1 - np.maximum(si, ii))
    union = (sj - si + 1) + (jj - ii + 1) - inter
    return inter.astype(F32) >= F32(nms_iou) * union.astype(F32)


def greedy_nms(ii, jj, sc, k, nms_iou):
    """plain greedy NMS over a sorted candidate list: each pick is the first candidate no earlier pick suppresses"""
    alive = np.ones(len(ii), dtype=bool)
    out = []
    while len(out) < k and alive.any():
        x = int(np.argmax(alive))
        out.append((int(ii[x]), int(jj[x]), sc[x]))
        alive &= ~suppressed(ii[x], jj[x], ii, jj, nms_iou)
    return out


def span_topk_ref(s_logits, e_logits, vlen, k, max_len=0, nms_iou=1.0):
    """-> start int64 [B,k], end int64 [B,k], score float32 [B,k] (numpy)"""
    ps, pe, v, mask = probabilities(s_logits, e_logits, vlen)
    s = torch.as_tensor(s_logits, dtype=torch.float32).cpu().numpy()
    e = torch.as_tensor(e_logits, dtype=torch.float32).cpu().numpy()
    B = ps.shape[0]
    st = np.full((B, k), -1, dtype=np.int64)
    en = np.full((B, k), -1, dtype=np.int64)
    sc = np.full((B, k), -1.0, dtype=F32)
    for b in range(B):
        n = int(v[b])
        if n < 1 or np.isnan(s[b, :n]).any() or np.isnan(e[b, :n]).any():
            continue
        for r, (i, j, x) in enumerate(greedy_nms(*candidates(ps[b], pe[b], n, max_len), k, nms_iou)):
            st[b, r], en[b, r], sc[b, r] = i, j, x
    return st, en, sc


def non_product_tie(ps, pe, v):
    """True when slot 0 of the contract can differ from ans_predictor's span: the smallest start and the smallest end among the
    maximal pairs are not themselves a maximal pair (different products that round to the same maximal float)"""
    ii, jj, sc = candidates(ps, pe, v)
    top = sc == sc[0]
    i0, j0 = ii[top].min(), jj[top].min()
    return not bool(np.any(top & (ii == i0) & (jj == j0)))
