#!/usr/bin/env python3
"""What core-set selection costs: hual_kcenter_greedy (lib.kcenter_select: one call, 2 + n_select launches) against the sync-free
torch loop it replaces - per step d = ((x - x[c]) ** 2).sum(1), mind = minimum(mind, d), a masked argmax of w * mind, with the pick c
kept as a device index, so neither leg synchronises between steps.  x: N(0, 1) float32 [N, D]; n_select = N // 2; with uniform(0, 1)
weights and without.  Per leg: wall clock around the whole selection with a synchronisation at its end (host time included: that is
what a caller pays); the legs alternate within a round; medians of --rounds rounds after a short warm-up of both, with the spread.
Also the share of steps at which the two legs picked the same row (they round differently, so near-ties part them).  Nothing is
gated on the times.
    python scripts/bench_kcenter.py [--n 4096 12403] [--d 128 1024] [--rounds 3]
Prints one JSON line (milliseconds)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, nargs='+', default=[4096, 12403])
    ap.add_argument('--d', type=int, nargs='+', default=[128, 1024])
    ap.add_argument('--rounds', type=int, default=3)
    a = ap.parse_args()
    import torch
    from hual_amd import lib
    if not torch.cuda.is_available():
        raise SystemExit('bench_kcenter: no GPU - nothing is measured without one')
    dev = torch.device('cuda:0')
    out = dict(rounds=a.rounds)

    def torch_loop(x, w, n_select, picked):
        N = x.shape[0]
        mind = torch.full((N,), float('inf'), device=dev)
        taken = torch.zeros(N, dtype=torch.bool, device=dev)
        ninf = torch.full((N,), float('-inf'), device=dev)
        score = w if w is not None else torch.ones(N, device=dev)
        for s in range(n_select):
            c = torch.where(taken, ninf, score).argmax().view(1)          # a device index: nothing is read back
            picked[s:s + 1] = c
            taken.index_fill_(0, c, True)
            d = ((x - x.index_select(0, c)) ** 2).sum(1)
            mind = torch.minimum(mind, d)
            score = w * mind if w is not None else mind
        return mind

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for N in a.n:
        for D in a.d:
            g = torch.Generator(device='cpu').manual_seed(N + D)
            x = torch.randn(N, D, generator=g).to(dev)
            for weighted in (False, True):
                w = torch.rand(N, generator=g).to(dev) if weighted else None
                n_select = N // 2
                ws = torch.empty(lib.kcenter_workspace_bytes(N), dtype=torch.uint8, device=dev)
                outs = (torch.empty(n_select, dtype=torch.int32, device=dev), torch.empty(n_select, device=dev), torch.empty(N, device=dev),
                        torch.empty(N, dtype=torch.int32, device=dev))
                t_picked = torch.empty(n_select, dtype=torch.int64, device=dev)
                legs = dict(launch=lambda k=n_select: lib.kcenter_select(x, k, weight=w, out=(outs[0][:k], outs[1][:k], outs[2], outs[3]), workspace=ws),
                            torch=lambda k=n_select: torch_loop(x, w, k, t_picked))
                for fn in legs.values():                                  # warm-up: 64 steps of each
                    fn(64)
                torch.cuda.synchronize()
                wall = {k: [] for k in legs}
                for _ in range(a.rounds):
                    for k, fn in legs.items():
                        wall[k].append(timed(fn))
                key = 'N%d_D%d_%s' % (N, D, 'weighted' if weighted else 'plain')
                for k in legs:
                    out['%s_%s_wall_ms' % (key, k)] = round(float(np.median(wall[k])), 2)
                    out['%s_%s_wall_spread_ms' % (key, k)] = [round(float(min(wall[k])), 2), round(float(max(wall[k])), 2)]
                out['%s_launch_us_per_step' % key] = round(1e3 * float(np.median(wall['launch'])) / n_select, 2)
                out['%s_torch_over_launch' % key] = round(float(np.median(wall['torch'])) / float(np.median(wall['launch'])), 2)
                out['%s_same_picks' % key] = round(float((outs[0].long() == t_picked).float().mean()), 4)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
