#!/usr/bin/env python3
"""What sessions that stop on label reliability cost: one hual_al_session_label launch (LabelUpdater.session_label, stop_hit 0.9 at
IoU 0.7) beside the two things next to it, in the same run:
  session  hual_al_session alone (LabelUpdater.session) - what the label trail and the rule add to a session;
  loop     the launches the new one replaces - per pass LabelUpdater.query(), mbr_label() and hit_label() (under noise behind
           tilt()), a read-back, the decision from the stored float32 values, a host append of the simulated annotator's answer and
           set_active_points() (the CSR rebuilt and uploaded).
N samples of exactly T frames (random logits, one random ground-truth span each), sessions from empty lists, Q questions, the hard
rule and eps = 0.1.  Per leg: wall clock around the whole leg with a synchronisation at its end (host time included: that is what a
caller pays) and device events around the same region; the legs alternate within a round, medians of --rounds rounds after one
warm-up round.
    python scripts/bench_al_session_label.py [--n 4096 12403] [--t 64 128] [--q 6] [--rounds 5]
Prints one JSON line (milliseconds)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STOP_HIT, STOP_AT = 0.9, 0.7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, nargs='+', default=[4096, 12403])
    ap.add_argument('--t', type=int, nargs='+', default=[64, 128])
    ap.add_argument('--q', type=int, default=6)
    ap.add_argument('--rounds', type=int, default=5)
    a = ap.parse_args()
    import torch
    from hual_amd import al, lib
    if not torch.cuda.is_available():
        raise SystemExit('bench_al_session_label: no GPU - nothing is measured without one')
    Qn = a.q
    col = al.HIT_IOUS.index(STOP_AT)
    reliable = lib.AL_STOP_REASONS.index('reliable')
    out = dict(questions=Qn, rounds=a.rounds, stop_hit=STOP_HIT, stop_at=STOP_AT)

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
            rows = np.arange(N)
            up = al.LabelUpdater(prop, empty)
            for eps, tag in ((0.0, 'hard'), (0.1, 'eps0.1')):
                noise = eps if eps > 0 else None

                def label_session():
                    up.set_active_points(empty)
                    n_asked = up.session_label(gt, Qn, stop_hit=STOP_HIT, stop_at=STOP_AT, noise=noise)[2]
                    return n_asked, int((up.stop_reason.cpu().numpy() == reliable).sum())

                def session():
                    up.set_active_points(empty)
                    return up.session(gt, Qn, noise=noise)[2], 0

                def loop():
                    lists = [[] for _ in range(N)]
                    up.set_active_points(lists)
                    going = np.ones(N, dtype=bool)
                    stopped_reliable = 0
                    for k in range(Qn + 1):
                        up.query(frames=noise is not None, noise=noise)
                        new_idx = up.mbr_label(rows, np.zeros((N, 2), dtype=np.int32), noise=noise)[0]
                        up.hit_label(cand=new_idx[:, None, :], thresholds=al.HIT_IOUS, best=False, noise=noise)
                        qp, qg, hit = up.query_point.cpu().numpy(), up.query_gain.cpu().numpy(), up.cand_hit.cpu().numpy()[:, 0, col]
                        safe = going & (qp >= 0) & (hit >= np.float32(STOP_HIT))
                        stopped_reliable += int(safe.sum())
                        going &= ~safe & (qg > 0)
                        if k == Qn or not going.any():
                            break
                        for i in np.flatnonzero(going):
                            t = int(qp[i])
                            lists[i].append((t, bool(gt[i, 0] <= t <= gt[i, 1])))
                        up.set_active_points(lists)
                    return np.array([len(x) for x in lists]), stopped_reliable

                legs = dict(label_session=label_session, session=session, loop=loop)
                wall, dev, res = {k: [] for k in legs}, {k: [] for k in legs}, {}
                for rnd in range(a.rounds + 1):             # round 0 warms up
                    for k, fn in legs.items():
                        w, d, res[k] = timed(fn)
                        if rnd:
                            wall[k].append(w)
                            dev[k].append(d)
                key = 'N%d_T%d_%s' % (N, T, tag)
                for k in legs:
                    out['%s_%s_wall_ms' % (key, k)] = round(float(np.median(wall[k])), 3)
                    out['%s_%s_device_ms' % (key, k)] = round(float(np.median(dev[k])), 3)
                    out['%s_%s_wall_spread_ms' % (key, k)] = [round(float(min(wall[k])), 3), round(float(max(wall[k])), 3)]
                    out['%s_%s_questions_asked' % (key, k)] = int(res[k][0].sum())
                out['%s_stopped_reliable' % key] = res['label_session'][1]
                out['%s_loop_stopped_reliable' % key] = res['loop'][1]
                out['%s_label_session_over_session' % key] = round(out['%s_label_session_wall_ms' % key] / out['%s_session_wall_ms' % key], 2)
                out['%s_loop_over_label_session' % key] = round(out['%s_loop_wall_ms' % key] / out['%s_label_session_wall_ms' % key], 2)
            up.set_active_points(empty)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
