#!/usr/bin/env python3
"""What a gradient-space batch asks about, on a set with several queries per video (CPU, float64, seeded; the contract's
reference, tests/kcenter_sample_ref.py - no GPU).  The queries' videos are the reference's own (tests/golden/lengths_<task>.npz: the
first --n queries in annotation order; seeded multiplicities of 1 to 5 if a fixture holds no video ids).  A query's descriptor is its
video's seeded unit direction plus --spread of a direction of its own, scaled by the square root of its score, and the score - read
here as the expected gradient length, egl - is its video's hardness plus --noise of its own, through exp(): hard videos hold many
long, nearly parallel gradients.  That is an ASSUMPTION about the scores and the geometry, not a measurement of a model: the more of a
gradient's direction is per query, the smaller the gap.  Reported per task, for the asked half by three rules - the top half by egl,
greedy k-center from the origin, D^2 sampling from the origin (BADGE) -: the distinct videos asked about and the half's mean egl.
    python scripts/grad_embed_gap.py [--n 2000] [--d 32] [--noise 0.3] [--spread 0.3] [--seed 0]
Prints one JSON line."""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=2000)
    ap.add_argument('--d', type=int, default=32)
    ap.add_argument('--noise', type=float, default=0.3)
    ap.add_argument('--spread', type=float, default=0.3)
    ap.add_argument('--seed', type=int, default=0)
    a = ap.parse_args()
    import kcenter_sample_ref as SR
    out = dict(n=a.n, d=a.d, noise=a.noise, spread=a.spread, seed=a.seed)
    for task in ('charades', 'anet'):
        g = np.random.default_rng(a.seed)
        fix = np.load(os.path.join(ROOT, 'tests', 'golden', 'lengths_%s.npz' % task))
        if 'vid' in fix.files:
            vid = np.unique(np.asarray(fix['vid'])[:a.n], return_inverse=True)[1]
        else:
            vid = np.repeat(np.arange(a.n), g.integers(1, 6, size=a.n))[:a.n]
        N, V = len(vid), int(vid.max()) + 1
        unit = lambda m: m / np.linalg.norm(m, axis=1, keepdims=True)
        direction = unit(unit(g.standard_normal((V, a.d)))[vid] + a.spread * unit(g.standard_normal((N, a.d))))
        egl = np.exp(g.standard_normal(V)[vid] + a.noise * g.standard_normal(N))
        x = direction * np.sqrt(egl)[:, None]                             # |x|^2 = egl
        k = math.ceil(N / 2)
        halves = dict(ranked_by_egl=np.argsort(-egl, kind='stable')[:k],
                      greedy_from_origin=SR.run(x, k, sample=False, origin=True)['picked'],
                      sampled_from_origin=SR.run(x, k, seed=a.seed, sample=True, origin=True)['picked'])
        res = dict(queries=N, videos=V, asked=k, mean_egl_all=round(float(egl.mean()), 4))
        for name, sel in halves.items():
            res[name] = dict(distinct_videos=int(len(np.unique(vid[sel]))), mean_egl=round(float(egl[sel].mean()), 4))
        out[task] = res
    print(json.dumps(out))


if __name__ == '__main__':
    main()
