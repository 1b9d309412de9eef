#!/usr/bin/env python3
"""What the information-gain query costs beside the scoring launch of the label update: hual_al_query and hual_al_score from the same
build on the same set - N samples of ld frames (random logits, v_len in [ld / 2, ld]), with 0 and with 3 truthful active points per
sample.  Device events around --iters back-to-back launches of one kind into preallocated outputs; medians of --rounds interleaved
rounds in one process (one warm-up round first).
    python scripts/bench_al_query.py [--n 4096] [--ld 100] [--rounds 5] [--iters 50]
Prints one JSON line (microseconds per launch)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=4096)
    ap.add_argument('--ld', type=int, default=100)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=50)
    a = ap.parse_args()
    import torch
    from hual_amd import al, lib
    if not torch.cuda.is_available():
        raise SystemExit('bench_al_query: no GPU - nothing is measured without one')
    g = np.random.default_rng(5)
    N, ld = a.n, a.ld
    vlen = g.integers(ld // 2, ld + 1, size=N)
    lg = (g.standard_normal((3, 2, N, ld)) * 2).astype(np.float32)
    prop = [{'vid': 'v%d' % n, 'v_len': int(vlen[n]), 'prop_logits': [lg[0, 0, n], lg[0, 1, n]], 'prop_logits1': [lg[1, 0, n], lg[1, 1, n]],
             'prop_logits2': [lg[2, 0, n], lg[2, 1, n]]} for n in range(N)]
    aps3 = []
    for n in range(N):
        s = int(g.integers(0, vlen[n]))
        e = int(g.integers(s, vlen[n]))
        aps3.append([(int(f), bool(s <= f <= e)) for f in g.choice(int(vlen[n]), size=3, replace=False)])
    ups = {0: al.LabelUpdater(prop, [[] for _ in range(N)]), 3: al.LabelUpdater(prop, aps3)}
    outs = {k: lib.al_query(u.set, u._s0, u._e0, u.tlen_h) for k, u in ups.items()}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1000.0 / a.iters

    legs = {}
    for k, u in ups.items():
        legs['score_ap%d_us' % k] = lambda u=u: u.score(0.25)
        legs['query_ap%d_us' % k] = lambda u=u, k=k: lib.al_query(u.set, u._s0, u._e0, u.tlen_h, out=outs[k])
        legs['query_ap%d_no_frames_us' % k] = lambda u=u, k=k: lib.al_query(u.set, u._s0, u._e0, u.tlen_h, out=(None, None) + outs[k][2:])
    times = {k: [] for k in legs}
    for rnd in range(a.rounds + 1):                 # round 0 warms up
        for k, fn in legs.items():
            t = timed(fn)
            if rnd:
                times[k].append(t)
    out = dict(n_samples=N, ld=ld, rounds=a.rounds, iters=a.iters)
    for k, v in times.items():
        out[k] = round(float(np.median(v)), 2)
        out[k.replace('_us', '_spread_us')] = [round(float(min(v)), 2), round(float(max(v)), 2)]
    for k in ups:
        out['query_over_score_ap%d' % k] = round(out['query_ap%d_us' % k] / out['score_ap%d_us' % k], 3)
    out['asked_ap3'] = int((outs[3][3] > 0).sum())
    print(json.dumps(out))


if __name__ == '__main__':
    main()
