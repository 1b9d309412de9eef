"""hual_span_expected_iou timing on the GPU box beside hual_span_topk at the same shape, from the same library: device events
around --iters back-to-back launches after warm-up (the method of scripts/bench_span_topk.py; at these kernel times the host's enqueue
can be what it measures) and around replays of a graph of --per-graph launches (the device alone), on seeded random logits; the
kernels alternate over --rounds rounds, median and max - min spread reported.  One JSON line per shape.

    python scripts/bench_span_conf.py [--iters 2000] [--k 5] [--nms-iou 0.5] [--shapes 64x128,32x256]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hual_amd import lib  # noqa: E402


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


def _graph_of(fn, n):
    """n back-to-back launches of fn captured once: a replay pays no per-launch host work, so the events see the device alone"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(n):
            fn()
    return g


def _median_spread(xs):
    xs = sorted(xs)
    return round(xs[len(xs) // 2], 2), round(xs[-1] - xs[0], 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=2000, help='eager launches per timing')
    ap.add_argument('--per-graph', type=int, default=100, help='launches captured into one graph')
    ap.add_argument('--replays', type=int, default=100, help='graph replays per timing')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--k', type=int, default=5)
    ap.add_argument('--nms-iou', type=float, default=0.5)
    ap.add_argument('--shapes', default='64x128,32x256')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    for shape in a.shapes.split(','):
        B, T = (int(x) for x in shape.split('x'))
        g = torch.Generator().manual_seed(12345)
        s = (torch.randn(B, T, generator=g) * 2).clamp(-8, 8).to(dev)
        e = (torch.randn(B, T, generator=g) * 2).clamp(-8, 8).to(dev)
        lens = torch.randint(T // 2, T + 1, (B,), generator=g, dtype=torch.int32).to(dev)
        out = tuple(torch.empty(B, a.k, dtype=dt, device=dev) for dt in (torch.int64, torch.int64, torch.float32))
        conf = (torch.empty(B, a.k, dtype=torch.float32, device=dev), torch.empty(B, dtype=torch.float32, device=dev))
        lib.span_topk(s, e, lens, a.k, nms_iou=a.nms_iou, out=out)
        fns = dict(topk=lambda: lib.span_topk(s, e, lens, a.k, nms_iou=a.nms_iou, out=out),
                   conf=lambda: lib.span_expected_iou(s, e, lens, out[0], out[1], score=out[2], reorder=False, out=conf),
                   # (a re-ordered row is sorted from then on: later launches permute nothing, but do all the arithmetic)
                   conf_reorder=lambda: lib.span_expected_iou(s, e, lens, out[0], out[1], score=out[2], reorder=True, out=conf))
        graphs = {n: _graph_of(f, a.per_graph) for n, f in fns.items()}
        eager, dev_only = {n: [] for n in fns}, {n: [] for n in fns}
        for _ in range(a.rounds):                                   # the three alternate inside every round
            for n, f in fns.items():
                eager[n].append(_time(f, a.iters))
                dev_only[n].append(_time(graphs[n].replay, a.replays, warm=3) / a.per_graph)
        res = dict(kernel='hual_span_expected_iou', B=B, T=T, k=a.k, rounds=a.rounds)
        for n in fns:
            res[n + '_us_eager'], res[n + '_eager_spread'] = _median_spread(eager[n])
            res[n + '_us_graph'], res[n + '_graph_spread'] = _median_spread(dev_only[n])
        res['ratio_to_span_topk_graph'] = round(res['conf_us_graph'] / res['topk_us_graph'], 2)
        res['mean_conf_slot0'] = round(float(conf[0][:, 0].mean()), 4)
        res['mean_entropy_bits'] = round(float(conf[1].mean()), 3)
        print(json.dumps(res))


if __name__ == '__main__':
    main()
