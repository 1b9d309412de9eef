"""What the tests of the per-clip span launches (hual_span_topk, hual_span_expected_iou, hual_span_hit_prob) share: guarded output
buffers, the host's stable order, and the learnable task of test_gpu_runner.py for the evaluation tests."""
import numpy as np
import torch


def _sentinel(shape, dtype, dev, value, pad=64):
    """a tensor of `shape` in the middle of a larger allocation filled with `value`: (view, whole buffer, pad)"""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * pad,), value, dtype=dtype, device=dev)
    return whole[pad:pad + n].view(*shape), whole, pad


def _pads_intact(whole, pad, value):
    return bool((whole[:pad] == value).all()) and bool((whole[-pad:] == value).all())


def stable_order(values):
    """the permutation of a reorder: values descending, equal ones (and the -1 of invalid slots, last) in their incoming order"""
    return np.argsort(-np.asarray(values), kind='stable')


def _videos(nvid, vdim, seed):
    g = np.random.default_rng(seed)
    vis = {}
    for v in range(nvid):
        T = int(g.integers(20, 33))
        f = 0.1 * g.standard_normal((T, vdim)).astype(np.float32)
        f[:, 0] = np.linspace(-1, 1, T)                    # position signal
        vis['v%d' % v] = f
    return vis


def _task(n, vis, seed):
    g = np.random.default_rng(seed)
    recs = []
    for i in range(n):
        vid = 'v%d' % int(g.integers(0, len(vis)))
        T = vis[vid].shape[0]
        part = int(g.integers(0, 3))                       # early / middle / late third, named by the first word
        s = part * T // 3 + 1
        e = min(T - 1, s + T // 3 - 2)
        words = ['w%d' % (2 + part), 'w%d' % int(g.integers(5, 30)), 'w%d' % int(g.integers(5, 30))]
        recs.append(dict(vid=vid, duration=float(T), v_len=T, words=words, w_ids=[int(w[1:]) for w in words],
                         c_ids=[[1 + part, 2, 3, 4]] * 3, s_ind=s, e_ind=e))
    return recs
