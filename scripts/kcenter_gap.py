#!/usr/bin/env python3
"""What a diverse half buys on a set with several queries per video (CPU, float64, seeded; the contract's reference,
tests/kcenter_ref.py - no GPU).  The queries' videos are the reference's own (tests/golden/lengths_<task>.npz: the first --n queries
in annotation order, so queries of one video stay together, as in the training lists; seeded multiplicities of 1 to 5 if a fixture
holds no video ids).  A video's descriptor is a seeded unit vector shared by its queries, as DeviceDataset.clip_descriptors() gives
them; a query's score is its video's hardness plus --noise of its own, so hard videos fill the top of the ranking with near-duplicate
clips - the situation the selection is for, and an ASSUMPTION about the scores: the more of a score's variance is per query, the
smaller the gap.  Reported per task: the distinct videos in the asked half and the covering radius (the largest distance of any query
to its nearest asked one), for the ranked half against the k-center half, weighted by rank and unweighted.
    python scripts/kcenter_gap.py [--n 2000] [--d 32] [--noise 0.3] [--seed 0]
Prints one JSON line."""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=2000)
    ap.add_argument('--d', type=int, default=32)
    ap.add_argument('--noise', type=float, default=0.3)
    ap.add_argument('--seed', type=int, default=0)
    a = ap.parse_args()
    import kcenter_ref as KR
    out = dict(n=a.n, d=a.d, noise=a.noise, seed=a.seed)
    for task in ('charades', 'anet'):
        g = np.random.default_rng(a.seed)
        fix = np.load(os.path.join(ROOT, 'tests', 'golden', 'lengths_%s.npz' % task))
        if 'vid' in fix.files:
            vid = np.unique(np.asarray(fix['vid'])[:a.n], return_inverse=True)[1]
        else:
            vid = np.repeat(np.arange(a.n), g.integers(1, 6, size=a.n))[:a.n]
        N, V = len(vid), int(vid.max()) + 1
        desc = g.standard_normal((V, a.d))
        desc /= np.linalg.norm(desc, axis=1, keepdims=True)
        x = desc[vid]
        score = g.standard_normal(V)[vid] + a.noise * g.standard_normal(N)
        order = np.argsort(-score, kind='stable')
        rank = np.empty(N, dtype=np.int64)
        rank[order] = np.arange(N)
        w = ((N - rank) / N).astype(np.float32)
        k = math.ceil(N / 2)
        plain_w = np.full(N, 0.5)
        plain_w[order[0]] = 1.0
        halves = dict(ranked=order[:k], kcenter_weighted=KR.greedy(x, k, w)['picked'], kcenter_plain=KR.greedy(x, k, plain_w)['picked'])
        res = dict(queries=N, videos=V, asked=k)
        for name, sel in halves.items():
            st = KR.State(x)
            for c in sel:
                st.add(int(c))
            res[name] = dict(distinct_videos=int(len(np.unique(vid[sel]))), cover_radius=round(float(np.sqrt(st.mind.max())), 4),
                             mean_rank=round(float(rank[sel].mean()), 1))
        out[task] = res
    print(json.dumps(out))


if __name__ == '__main__':
    main()
