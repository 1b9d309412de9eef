"""hual_span_hit_cover timing on the GPU box: device events around --iters back-to-back launches after warm-up (the method of
scripts/bench_span_hit.py) at K = k = 5 and 16 and the thresholds 3/10, 1/2, 7/10 - the proposals' cumulative coverage alone, the
greedy sets alone, both in one launch - beside hual_span_hit_prob(best=True), whose search is the cover's step 0, and the label-free
forward (model.forward, drop 0) of a synthetic batch of the same shape and lengths.  The kernel's loops depend on the lengths, the
thresholds and - through the lists of covered ends - on where the picks fall, so the logits matter here: seeded random logits N(0, 2)
stand in for the forward's, and the number of steps taken before the sets stop is reported with the times.  --rounds rounds, the modes
alternating inside each; median and max - min spread reported.  One JSON line per shape.

    python scripts/bench_span_cover.py [--iters 50] [--ks 5,16] [--shapes 64x128,32x256]
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
from scripts.bench_span_hit import THRESHOLDS, _median_spread, _time  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--ks', default='5,16')
    ap.add_argument('--min-gain', type=float, default=1e-6)
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
        best = (torch.empty(B, M, dtype=torch.int64, device=dev), torch.empty(B, M, dtype=torch.int64, device=dev),
                torch.empty(B, M, dtype=torch.float32, device=dev))
        fns = dict(bayes_span=lambda: lib.span_hit_prob(s, e, lens, THRESHOLDS, best=True, out=(None, best)),
                   forward=lambda: model.forward(video, lens, wid, cid, drop_rate=0.0))
        outs = {}
        for k in (int(x) for x in a.ks.split(',')):
            st, en, _ = lib.span_topk(s, e, lens, k, nms_iou=0.5)
            sp = torch.empty(B, k, M, dtype=torch.float32, device=dev)
            cover = (torch.empty(B, M, k, dtype=torch.int64, device=dev), torch.empty(B, M, k, dtype=torch.int64, device=dev),
                     torch.empty(B, M, k, dtype=torch.float32, device=dev))
            outs[k] = (sp, cover)
            fns['proposals_k%d' % k] = lambda st=st, en=en, sp=sp: lib.span_hit_cover(s, e, lens, THRESHOLDS, st, en, out=(sp, None))
            fns['sets_K%d' % k] = lambda k=k, cover=cover: lib.span_hit_cover(s, e, lens, THRESHOLDS, K=k, min_gain=a.min_gain, out=(None, cover))
            fns['both_%d' % k] = lambda st=st, en=en, sp=sp, k=k, cover=cover: lib.span_hit_cover(s, e, lens, THRESHOLDS, st, en, K=k, min_gain=a.min_gain,
                                                                                               out=(sp, cover))
        us = {n: [] for n in fns}
        for _ in range(a.rounds):
            for n, f in fns.items():
                us[n].append(_time(f, max(20, a.iters // 2) if n == 'forward' else a.iters, warm=3))
        res = dict(kernel='hual_span_hit_cover', B=B, T=T, M=M, min_gain=a.min_gain, iters=a.iters, rounds=a.rounds,
                   mean_len=round(float(lens.float().mean()), 1))
        for n in fns:
            res[n + '_us'], res[n + '_spread'] = _median_spread(us[n])
        for k, (sp, cover) in outs.items():
            res['both_%d_share_of_forward' % k] = round(res['both_%d_us' % k] / res['forward_us'], 3)
            res['sets_K%d_over_bayes_span' % k] = round(res['sets_K%d_us' % k] / res['bayes_span_us'], 2)
            res['mean_steps_K%d' % k] = [round(float(x), 2) for x in (cover[0] >= 0).float().sum(dim=2).mean(dim=0)]
            res['mean_set_prob_k%d' % k] = [round(float(x), 4) for x in sp[:, k - 1, :].mean(dim=0)]
            res['mean_cover_prob_K%d' % k] = [round(float(x), 4) for x in cover[2][:, :, k - 1].mean(dim=0)]
        print(json.dumps(res))


if __name__ == '__main__':
    main()
