#!/usr/bin/env python3
"""What the evidence of a set's answers on a grid of temperatures and error rates costs: one hual_al_evidence_grid call (three launches:
the cells, the fold, the best cell) beside the loop it replaces - per cell a torch product of both logit matrices by float32(1 / tau),
hual_al_noisy_tilt on the scaled rows, and a torch sum of its log_evidence -, which is what a caller could do before.  N samples of
exactly T frames (random logits, one random ground-truth span each), --answers answers per sample at distinct random frames, a tenth
of them wrong, the default grid of LabelUpdater.calibrate (17 temperatures x 10 error rates).  Per leg: wall clock around the whole
leg with a synchronisation at its end (host time included: that is what a caller pays), and device events around the same region;
medians of --rounds repetitions after one warm-up.  `calibrate` is the whole fit: the coarse grid and two zooms, read-backs included.
    python scripts/bench_al_calib.py [--n 4096 12403] [--t 64 128] [--answers 3] [--rounds 5]
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
    ap.add_argument('--n', type=int, nargs='+', default=[4096, 12403])      # 12,403: the Charades-STA training set
    ap.add_argument('--t', type=int, nargs='+', default=[64, 128])
    ap.add_argument('--answers', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=5)
    a = ap.parse_args()
    import torch
    from hual_amd import al, lib
    if not torch.cuda.is_available():
        raise SystemExit('bench_al_calib: no GPU - nothing is measured without one')
    taus, eps = np.array(al.CALIB_TAUS), np.array(al.CALIB_EPS, dtype=np.float32)
    inv = np.array([np.float32(1.0 / t) for t in taus], dtype=np.float32)
    out = dict(answers_per_sample=a.answers, grid=[len(taus), len(eps)], rounds=a.rounds)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        res = fn()
        e1.record()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1), res

    for N in a.n:
        for T in a.t:
            g = np.random.default_rng(7 + T + N)
            lg = (g.standard_normal((2, N, T)) * 2).astype(np.float32)
            prop = [{'vid': 'v%d' % n, 'v_len': T, 'prop_logits': [lg[0, n], lg[1, n]], 'prop_logits1': [lg[0, n], lg[1, n]],
                     'prop_logits2': [lg[0, n], lg[1, n]]} for n in range(N)]
            gt = np.sort(g.integers(0, T, size=(N, 2)), axis=1)
            aps = []
            for n in range(N):
                fr = g.choice(T, a.answers, replace=False)
                aps.append([(int(f), bool(gt[n, 0] <= f <= gt[n, 1]) != bool(g.random() < 0.1)) for f in fr])
            up = al.LabelUpdater(prop, aps)
            outs = lib.al_evidence_grid(up.set, up._s0, up._e0, up.tlen_h, inv, eps)
            tilt_out = lib.al_noisy_tilt(up.set, up._s0, up._e0, up.tlen_h, 0.1)

            def launch():
                lib.al_evidence_grid(up.set, up._s0, up._e0, up.tlen_h, inv, eps, out=outs)
                return outs[2]

            def loop():
                tot = torch.empty(len(inv) * len(eps), dtype=torch.float64, device=up.dev)
                for ia, k in enumerate(inv):
                    for ib, e in enumerate(eps):
                        s, e_ = up._s0 * float(k), up._e0 * float(k)
                        lib.al_noisy_tilt(up.set, s, e_, up.tlen_h, float(e), out=tilt_out)
                        tot[ia * len(eps) + ib] = tilt_out[2].double().sum()
                return tot

            def calibrate():
                return up.calibrate(at_eps=0.1)

            legs = dict(launch=launch, loop=loop, calibrate=calibrate)
            wall, dev, res = {k: [] for k in legs}, {k: [] for k in legs}, {}
            for rnd in range(a.rounds + 1):             # round 0 warms up
                for k, fn in legs.items():
                    w, d, res[k] = timed(fn)
                    if rnd:
                        wall[k].append(w)
                        dev[k].append(d)
            key = 'N%d_T%d' % (N, T)
            for k in legs:
                out['%s_%s_wall_ms' % (key, k)] = round(float(np.median(wall[k])), 3)
                out['%s_%s_device_ms' % (key, k)] = round(float(np.median(dev[k])), 3)
                out['%s_%s_wall_spread_ms' % (key, k)] = [round(float(min(wall[k])), 3), round(float(max(wall[k])), 3)]
            out['%s_loop_over_launch' % key] = round(out['%s_loop_wall_ms' % key] / out['%s_launch_wall_ms' % key], 1)
            # the two legs compute the same totals: the loop's from float32 evidences
            d = (res['launch'] - res['loop']).abs() / res['launch'].abs().clamp_min(1.0)
            out['%s_max_rel_total_diff' % key] = float(d.max())
            out['%s_fit' % key] = {k: round(float(res['calibrate'][k]), 5) for k in ('tau', 'eps', 'per_answer')}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
