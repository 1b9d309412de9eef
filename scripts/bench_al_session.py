#!/usr/bin/env python3
"""What Q adaptive questions per clip cost: one hual_al_session launch beside the path that existed before it - per question
LabelUpdater.query() (under noise: tilt() first), a read-back of the frame and its gain, a host append of the simulated annotator's
answer, and set_active_points() (the CSR rebuilt and uploaded).  N samples of exactly T frames (random logits, one random ground-truth
span each), sessions from empty lists, no thresholds, hard rule and eps = 0.1.  Per leg: wall clock around the whole leg with a
synchronisation at its end (host time included: that is what a caller pays), and device events around the same region; medians of
--rounds repetitions after one warm-up.
    python scripts/bench_al_session.py [--n 4096] [--t 64 128] [--q 6] [--rounds 5]
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
    ap.add_argument('--n', type=int, default=4096)
    ap.add_argument('--t', type=int, nargs='+', default=[64, 128])
    ap.add_argument('--q', type=int, default=6)
    ap.add_argument('--rounds', type=int, default=5)
    a = ap.parse_args()
    import torch
    from hual_amd import al, lib
    if not torch.cuda.is_available():
        raise SystemExit('bench_al_session: no GPU - nothing is measured without one')
    N, Qn = a.n, a.q
    out = dict(n_samples=N, questions=Qn, rounds=a.rounds)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        res = fn()
        e1.record()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1), res

    for T in a.t:
        g = np.random.default_rng(7 + T)
        lg = (g.standard_normal((3, 2, N, T)) * 2).astype(np.float32)
        prop = [{'vid': 'v%d' % n, 'v_len': T, 'prop_logits': [lg[0, 0, n], lg[0, 1, n]], 'prop_logits1': [lg[1, 0, n], lg[1, 1, n]],
                 'prop_logits2': [lg[2, 0, n], lg[2, 1, n]]} for n in range(N)]
        gt = np.sort(g.integers(0, T, size=(N, 2)), axis=1).astype(np.int32)
        empty = [[] for _ in range(N)]
        up, up0 = al.LabelUpdater(prop, empty), al.LabelUpdater(prop, empty)      # up0 keeps its empty lists: the bare launch's set
        gt_d = torch.from_numpy(gt).to(up.dev)
        for eps, tag in ((0.0, 'hard'), (0.1, 'eps0.1')):
            noise = eps if eps > 0 else None
            outs = lib.al_session(up0.set, up0._s0, up0._e0, up0.tlen_h, gt_d, Qn, eps=eps)

            def launch():
                lib.al_session(up0.set, up0._s0, up0._e0, up0.tlen_h, gt_d, Qn, eps=eps, out=outs)

            def session():
                up.set_active_points(empty)
                return up.session(gt, Qn, noise=noise)[2]

            def loop():
                lists = [[] for _ in range(N)]
                up.set_active_points(lists)
                going = np.ones(N, dtype=bool)
                for _ in range(Qn):
                    up.query(frames=noise is not None, noise=noise)
                    qp, qg = up.query_point.cpu().numpy(), up.query_gain.cpu().numpy()
                    going &= qg > 0
                    for i in np.flatnonzero(going):
                        t = int(qp[i])
                        lists[i].append((t, bool(gt[i, 0] <= t <= gt[i, 1])))
                    up.set_active_points(lists)
                return np.array([len(x) for x in lists])

            legs = dict(launch=launch, session=session, loop=loop)
            wall, dev, res = {k: [] for k in legs}, {k: [] for k in legs}, {}
            for rnd in range(a.rounds + 1):             # round 0 warms up
                for k, fn in legs.items():
                    w, d, res[k] = timed(fn)
                    if rnd:
                        wall[k].append(w)
                        dev[k].append(d)
            key = 'T%d_%s' % (T, tag)
            for k in legs:
                out['%s_%s_wall_ms' % (key, k)] = round(float(np.median(wall[k])), 3)
                out['%s_%s_device_ms' % (key, k)] = round(float(np.median(dev[k])), 3)
                out['%s_%s_wall_spread_ms' % (key, k)] = [round(float(min(wall[k])), 3), round(float(max(wall[k])), 3)]
            out['%s_questions_asked' % key] = int(res['session'].sum())
            out['%s_loop_questions_asked' % key] = int(res['loop'].sum())
            out['%s_loop_over_launch' % key] = round(out['%s_loop_wall_ms' % key] / out['%s_launch_wall_ms' % key], 1)
            out['%s_loop_over_session' % key] = round(out['%s_loop_wall_ms' % key] / out['%s_session_wall_ms' % key], 1)
        up.set_active_points(empty)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
