#!/usr/bin/env python3
"""What label reliability costs: hual_al_hit_label in the two forms the round launches it in - the candidates-only launch over the
whole set with k = 2 spans per sample (no search), and the search over the selected half with M = 3 thresholds (3/10, 1/2, 7/10) and
the same two candidates - and beside them, for scale, hual_al_mbr_label on the same selected rows.  N samples of exactly T frames
(random logits N(0, 2): the loops depend on the lengths, the thresholds and the consistent set, not on the logits' values), after 0
and after 3 truthful answers per sample at distinct random frames.  Bare launches into preallocated outputs.  Per leg: wall clock
around the launch with a synchronisation at its end (host time included: that is what a caller pays), and device events around the
same region; the legs alternate within a round; medians of --rounds repetitions after one warm-up, with the spread.  Nothing is gated
on the times.
    python scripts/bench_al_hit_label.py [--n 4096 12403] [--t 64 128] [--rounds 7]
Prints one JSON line (milliseconds)."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

THRESHOLDS = ((3, 10), (1, 2), (7, 10))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, nargs='+', default=[4096, 12403])
    ap.add_argument('--t', type=int, nargs='+', default=[64, 128])
    ap.add_argument('--rounds', type=int, default=7)
    a = ap.parse_args()
    import torch
    from hual_amd import al, lib
    if not torch.cuda.is_available():
        raise SystemExit('bench_al_hit_label: no GPU - nothing is measured without one')
    out = dict(rounds=a.rounds, k=2, M=len(THRESHOLDS))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)

    for N in a.n:
        for T in a.t:
            g = np.random.default_rng(11 + T)
            lg = (g.standard_normal((2, N, T)) * 2).astype(np.float32)
            prop = [{'vid': 'v%d' % n, 'v_len': T, 'prop_logits': [lg[0, n], lg[1, n]], 'prop_logits1': [lg[0, n], lg[1, n]],
                     'prop_logits2': [lg[0, n], lg[1, n]]} for n in range(N)]
            gt = np.sort(g.integers(0, T, size=(N, 2)), axis=1)
            old = np.sort(g.integers(0, T, size=(N, 2)), axis=1).astype(np.int32)
            aps3 = [[(int(f), bool(gt[n, 0] <= f <= gt[n, 1])) for f in g.choice(T, size=3, replace=False)] for n in range(N)]
            sel = np.sort(g.permutation(N)[:math.ceil(N / 2)]).astype(np.int32)
            for h, aps in ((0, [[] for _ in range(N)]), (3, aps3)):
                up = al.LabelUpdater(prop, aps)
                sel_d, old_d = torch.from_numpy(sel).to(up.dev), torch.from_numpy(old).to(up.dev)
                head = (up.set, up._s0, up._e0, up.tlen_h)
                lab = lib.al_mbr_label(*head, sel=sel_d, old_idx=old_d)
                cand = torch.stack([old_d, torch.where(lab[0] >= 0, lab[0], old_d)], dim=1).contiguous()      # (old label, MBR label)
                c_out = lib.al_hit_label(*head, thresholds=THRESHOLDS, cand=cand, best=False)
                s_out = lib.al_hit_label(*head, thresholds=THRESHOLDS, sel=sel_d, cand=cand)
                legs = dict(candidates_all=lambda: lib.al_hit_label(*head, thresholds=THRESHOLDS, cand=cand, best=False, out=c_out),
                            search_half=lambda: lib.al_hit_label(*head, thresholds=THRESHOLDS, sel=sel_d, cand=cand, out=s_out),
                            mbr_label_half=lambda: lib.al_mbr_label(*head, sel=sel_d, old_idx=old_d, out=lab))
                wall, dev = {k: [] for k in legs}, {k: [] for k in legs}
                for rnd in range(a.rounds + 1):         # round 0 warms up
                    for k, fn in legs.items():
                        w, d = timed(fn)
                        if rnd:
                            wall[k].append(w)
                            dev[k].append(d)
                key = 'N%d_T%d_ap%d' % (N, T, h)
                for k in legs:
                    out['%s_%s_wall_ms' % (key, k)] = round(float(np.median(wall[k])), 3)
                    out['%s_%s_device_ms' % (key, k)] = round(float(np.median(dev[k])), 3)
                    out['%s_%s_wall_spread_ms' % (key, k)] = [round(float(min(wall[k])), 3), round(float(max(wall[k])), 3)]
                hit, bp = c_out[0].cpu().numpy(), s_out[1][1].cpu().numpy()[sel]
                live = bp[:, 0] >= 0
                out['%s_live_selected' % key] = int(live.sum())
                out['%s_mean_label_hit' % key] = [round(float(x), 4) for x in hit[:, 1][hit[:, 1, 0] >= 0].mean(axis=0)]
                out['%s_mean_best_prob' % key] = [round(float(x), 4) for x in bp[live].mean(axis=0)]
    print(json.dumps(out))


if __name__ == '__main__':
    main()
