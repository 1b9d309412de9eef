#!/usr/bin/env python3
"""What a question set of M frames per clip costs: one hual_al_design launch, and beside it - for scale, not as a ratio: the design
replaces no existing launch sequence - one hual_al_session launch with Q = M at the same shapes (the adaptive questions of an annotator
who is in the loop).  N samples of exactly T frames (random logits, one random ground-truth span each for the session), empty lists, no
thresholds, the hard rule.  Legs: the bare launches into preallocated outputs, and LabelUpdater.design() / .session() as a caller pays
for them (uploads, allocations and read-backs included).  Per leg: wall clock around the whole leg with a synchronisation at its end
(host time included), and device events around the same region; the legs alternate within a round; medians of --rounds repetitions after
one warm-up, with the spread.
    python scripts/bench_al_design.py [--n 4096 12403] [--t 64 128] [--m 6 16] [--rounds 7]
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
    ap.add_argument('--t', type=int, nargs='+', default=[64, 128])
    ap.add_argument('--m', type=int, nargs='+', default=[6, 16])
    ap.add_argument('--rounds', type=int, default=7)
    a = ap.parse_args()
    import torch
    from hual_amd import al, lib
    if not torch.cuda.is_available():
        raise SystemExit('bench_al_design: no GPU - nothing is measured without one')
    out = dict(rounds=a.rounds)

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
            g = np.random.default_rng(7 + T)
            lg = (g.standard_normal((3, 2, N, T)) * 2).astype(np.float32)
            prop = [{'vid': 'v%d' % n, 'v_len': T, 'prop_logits': [lg[0, 0, n], lg[0, 1, n]], 'prop_logits1': [lg[1, 0, n], lg[1, 1, n]],
                     'prop_logits2': [lg[2, 0, n], lg[2, 1, n]]} for n in range(N)]
            gt = np.sort(g.integers(0, T, size=(N, 2)), axis=1).astype(np.int32)
            empty = [[] for _ in range(N)]
            up, up0 = al.LabelUpdater(prop, empty), al.LabelUpdater(prop, empty)      # up0 keeps its empty lists: a session installs its answers
            gt_d = torch.from_numpy(gt).to(up.dev)
            for M in a.m:
                d_out = lib.al_design(up0.set, up0._s0, up0._e0, up0.tlen_h, M)
                s_out = lib.al_session(up0.set, up0._s0, up0._e0, up0.tlen_h, gt_d, M)

                def design_launch():
                    lib.al_design(up0.set, up0._s0, up0._e0, up0.tlen_h, M, out=d_out)

                def session_launch():
                    lib.al_session(up0.set, up0._s0, up0._e0, up0.tlen_h, gt_d, M, out=s_out)

                def design():
                    return up0.design(M)[1]

                def session():
                    up.set_active_points(empty)
                    return up.session(gt, M)[2]

                legs = dict(design_launch=design_launch, session_launch=session_launch, design=design, session=session)
                wall, dev, res = {k: [] for k in legs}, {k: [] for k in legs}, {}
                for rnd in range(a.rounds + 1):         # round 0 warms up
                    for k, fn in legs.items():
                        w, d, res[k] = timed(fn)
                        if rnd:
                            wall[k].append(w)
                            dev[k].append(d)
                key = 'N%d_T%d_M%d' % (N, T, M)
                for k in legs:
                    out['%s_%s_wall_ms' % (key, k)] = round(float(np.median(wall[k])), 3)
                    out['%s_%s_device_ms' % (key, k)] = round(float(np.median(dev[k])), 3)
                    out['%s_%s_wall_spread_ms' % (key, k)] = [round(float(min(wall[k])), 3), round(float(max(wall[k])), 3)]
                out['%s_frames_designed' % key] = int(res['design'].sum())
                out['%s_questions_asked' % key] = int(res['session'].sum())
                info = d_out[1].cpu().numpy().astype(np.float64)
                nd = d_out[3].cpu().numpy()
                last = info[np.arange(N), np.maximum(nd, 1) - 1]
                out['%s_mean_design_bits' % key] = round(float(np.where(nd > 0, last, 0.0).mean()), 4)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
