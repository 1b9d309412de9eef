"""hual_span_hit_prob timing on the GPU box: device events around --iters back-to-back launches after warm-up (the method of
scripts/bench_span_topk.py) of its three modes - the proposals' hit probabilities alone, the Bayes spans alone, both in one launch -
at k proposals and the thresholds 3/10, 1/2, 7/10, beside hual_span_expected_iou on the same proposals and the label-free forward
(model.forward, drop 0) of a synthetic batch of the same shape and lengths.  The kernel's loops depend on the lengths and the
thresholds, not on the logits' values: seeded random logits N(0, 2) stand in for the forward's.  --rounds rounds, the modes alternating
inside each; median and max - min spread reported.  One JSON line per shape.

    python scripts/bench_span_hit.py [--iters 200] [--k 5] [--shapes 64x128,32x256]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import synth_batch  # noqa: E402
from hual_amd import lib  # noqa: E402
from hual_amd.model import SeqPAN  # noqa: E402

THRESHOLDS = ((3, 10), (1, 2), (7, 10))


def _time(fn, iters, warm=10):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters      # us per call


def _median_spread(xs):
    xs = sorted(xs)
    return round(xs[len(xs) // 2], 2), round(xs[-1] - xs[0], 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--k', type=int, default=5)
    ap.add_argument('--shapes', default='64x128,32x256')
    ap.add_argument('--L', type=int, default=20)
    ap.add_argument('--vdim', type=int, default=1024)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    wv = np.random.default_rng(777).normal(0, 0.4, size=(998, 300)).astype(np.float32)
    M = len(THRESHOLDS)
    for shape in a.shapes.split(','):
        B, T = (int(x) for x in shape.split('x'))
        cfg = lib.make_cfg(vdim=a.vdim, max_vlen=max(T, a.L), num_words=1000, num_chars=40)
        model = SeqPAN(cfg, wv, device=dev, seed=12345, rng_seed=12345)
        b = synth_batch(B, T, a.L, 8, a.vdim, 1000, 40, 12345)
        video, lens = torch.from_numpy(b['video']).to(dev), torch.from_numpy(b['lens']).to(dev)
        wid, cid = torch.from_numpy(b['word_ids']).to(dev), torch.from_numpy(b['char_ids']).to(dev)
        g = torch.Generator().manual_seed(12345)
        s, e = (torch.randn(B, T, generator=g) * 2).to(dev), (torch.randn(B, T, generator=g) * 2).to(dev)
        st, en, sc = lib.span_topk(s, e, lens, a.k, nms_iou=0.5)
        hp = torch.empty(B, a.k, M, dtype=torch.float32, device=dev)
        best = (torch.empty(B, M, dtype=torch.int64, device=dev), torch.empty(B, M, dtype=torch.int64, device=dev),
                torch.empty(B, M, dtype=torch.float32, device=dev))
        conf = (torch.empty(B, a.k, dtype=torch.float32, device=dev), torch.empty(B, dtype=torch.float32, device=dev))
        fns = dict(proposals=lambda: lib.span_hit_prob(s, e, lens, THRESHOLDS, st, en, score=sc, out=(hp, None)),
                   bayes=lambda: lib.span_hit_prob(s, e, lens, THRESHOLDS, best=True, out=(None, best)),
                   both=lambda: lib.span_hit_prob(s, e, lens, THRESHOLDS, st, en, score=sc, best=True, out=(hp, best)),
                   expected_iou=lambda: lib.span_expected_iou(s, e, lens, st, en, score=sc, reorder=False, out=conf),
                   forward=lambda: model.forward(video, lens, wid, cid, drop_rate=0.0))
        us = {n: [] for n in fns}
        for _ in range(a.rounds):
            for n, f in fns.items():
                us[n].append(_time(f, max(20, a.iters // 4) if n == 'forward' else a.iters))
        res = dict(kernel='hual_span_hit_prob', B=B, T=T, k=a.k, M=M, iters=a.iters, rounds=a.rounds,
                   mean_len=round(float(lens.float().mean()), 1))
        for n in fns:
            res[n + '_us'], res[n + '_spread'] = _median_spread(us[n])
        res['bayes_share_of_forward'] = round(res['bayes_us'] / res['forward_us'], 3)
        res['proposals_share_of_forward'] = round(res['proposals_us'] / res['forward_us'], 4)
        res['mean_hit_prob_slot0'] = [round(float(x), 4) for x in hp[:, 0, :].mean(dim=0)]
        res['mean_best_prob'] = [round(float(x), 4) for x in best[2].mean(dim=0)]
        print(json.dumps(res))


if __name__ == '__main__':
    main()
