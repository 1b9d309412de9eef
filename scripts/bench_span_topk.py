"""hual_span_topk timing on the GPU box: device events around --iters back-to-back launches after warm-up, next to the label-free
forward (model.forward, drop 0) of a synthetic batch of the same shape.  One JSON line per shape.

    python scripts/bench_span_topk.py [--iters 200] [--k 5] [--nms-iou 0.5] [--shapes 64x128,32x256]
(rocprofv3 --kernel-trace --stats -- python scripts/bench_span_topk.py gives the kernel's own dispatch time.)
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


def _time(fn, iters, warm=20):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--k', type=int, default=5)
    ap.add_argument('--nms-iou', type=float, default=0.5)
    ap.add_argument('--shapes', default='64x128,32x256')
    ap.add_argument('--L', type=int, default=20)
    ap.add_argument('--vdim', type=int, default=1024)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    wv = np.random.default_rng(777).normal(0, 0.4, size=(998, 300)).astype(np.float32)
    for shape in a.shapes.split(','):
        B, T = (int(x) for x in shape.split('x'))
        cfg = lib.make_cfg(vdim=a.vdim, max_vlen=max(T, a.L), num_words=1000, num_chars=40)
        model = SeqPAN(cfg, wv, device=dev, seed=12345, rng_seed=12345)
        b = synth_batch(B, T, a.L, 8, a.vdim, 1000, 40, 12345)
        video, lens = torch.from_numpy(b['video']).to(dev), torch.from_numpy(b['lens']).to(dev)
        wid, cid = torch.from_numpy(b['word_ids']).to(dev), torch.from_numpy(b['char_ids']).to(dev)
        o = model.forward(video, lens, wid, cid, drop_rate=0.0)
        out = tuple(torch.empty(B, a.k, dtype=dt, device=dev) for dt in (torch.int64, torch.int64, torch.float32))

        def topk():
            lib.span_topk(o['start_logits'], o['end_logits'], lens, a.k, nms_iou=a.nms_iou, out=out)
        us_topk = _time(topk, a.iters)
        us_fwd = _time(lambda: model.forward(video, lens, wid, cid, drop_rate=0.0), max(20, a.iters // 4))
        print(json.dumps(dict(kernel='hual_span_topk', B=B, T=T, k=a.k, nms_iou=a.nms_iou, us_per_launch=round(us_topk, 2),
                              forward_us=round(us_fwd, 1), share_of_forward=round(us_topk / us_fwd, 4),
                              filled=int((out[0] >= 0).sum().item()))))


if __name__ == '__main__':
    main()
