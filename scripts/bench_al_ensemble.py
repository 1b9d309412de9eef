#!/usr/bin/env python3
"""What the span posterior as a model average over K stochastic passes costs: hual_al_ensemble_query (one launch: weights, q(t), the
marginals, both entropies, span_bald) beside the loop it replaces - per pass hual_al_query and hual_al_span_marginals on that pass's
plane, then the torch weighting (softmax of ln agree over the passes) and fold of incl and the marginals, which is what a caller could do
before, and which still has neither the mixture's entropy nor span_bald - and hual_al_ensemble_label beside K hual_al_mbr_label launches
(for scale only: K single-pass labels are not the label of the mixture, which no loop over the old launches gives).  N samples of exactly
T frames (random logits, K passes of sigma 0.7 around them, one random ground-truth span each), --answers truthful answers per sample at
distinct random frames.  Per leg: wall clock around the whole leg with a synchronisation at its end (host time included: that is what a
caller pays), and device events around the same region; medians of --rounds repetitions after one warm-up.
What post_entropy adds - the walk over the pairs of A, the one part with no closed form - is the difference to the same launch of a
library built with -DHUAL_ENS_NO_WALK (build_exp/ens_nowalk.so, built here if missing), timed by a child process of this script.
    python scripts/bench_al_ensemble.py [--n 4096 12403] [--t 64 128] [--k 8] [--answers 3] [--rounds 5]
Prints one JSON line (milliseconds)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NOWALK = os.path.join(ROOT, 'build_exp', 'ens_nowalk.so')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, nargs='+', default=[4096, 12403])      # 12,403: the Charades-STA training set
    ap.add_argument('--t', type=int, nargs='+', default=[64, 128])
    ap.add_argument('--k', type=int, default=8)
    ap.add_argument('--answers', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--query-only', action='store_true', help='time hual_al_ensemble_query alone (the child run on the no-walk library)')
    a = ap.parse_args()
    import torch
    from hual_amd import al, lib
    if not torch.cuda.is_available():
        raise SystemExit('bench_al_ensemble: no GPU - nothing is measured without one')
    K = a.k
    out = dict(K=K, answers_per_sample=a.answers, rounds=a.rounds)

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
            aps = [[(int(f), bool(gt[n, 0] <= f <= gt[n, 1])) for f in g.choice(T, a.answers, replace=False)] for n in range(N)]
            up = al.LabelUpdater(prop, aps)
            tg = torch.Generator(device='cpu').manual_seed(N + T)
            ps = (up._s0[None].cpu() + 0.7 * torch.randn(K, N, T, generator=tg)).to(up.dev).contiguous()
            pe = (up._e0[None].cpu() + 0.7 * torch.randn(K, N, T, generator=tg)).to(up.dev).contiguous()
            outs = lib.al_ensemble_query(up.set, ps, pe, up.tlen_h)
            q_out = [lib.al_query(up.set, ps[k], pe[k], up.tlen_h) for k in range(K)]
            m_out = [lib.al_span_marginals(up.set, ps[k], pe[k], up.tlen_h) for k in range(K)]
            old = torch.zeros(N, 2, dtype=torch.int32, device=up.dev)
            l_out = lib.al_ensemble_label(up.set, ps, pe, up.tlen_h, old_idx=old)
            l1_out = lib.al_mbr_label(up.set, ps[0], pe[0], up.tlen_h, old_idx=old)

            def ens_query():
                lib.al_ensemble_query(up.set, ps, pe, up.tlen_h, out=outs)
                return outs

            def loop_query():
                for k in range(K):
                    lib.al_query(up.set, ps[k], pe[k], up.tlen_h, out=q_out[k])
                    lib.al_span_marginals(up.set, ps[k], pe[k], up.tlen_h, out=m_out[k])
                agree = torch.stack([q[5] for q in q_out]).double()                     # [K, N]: Z_A,k / Z_k
                w = torch.softmax(torch.log(agree.clamp_min(0.0)), dim=0)
                incl = (w[:, :, None] * torch.stack([q[0] for q in q_out]).double()).sum(0).clamp(0.0, 1.0).float()
                ys = (w[:, :, None] * torch.stack([m[0] for m in m_out]).double()).sum(0).float()
                ye = (w[:, :, None] * torch.stack([m[1] for m in m_out]).double()).sum(0).float()
                x, y = incl.clamp(1e-30, 1.0), (1.0 - incl).clamp(1e-30, 1.0)
                gain = -(x * torch.log2(x) + y * torch.log2(y))
                return w, incl, ys, ye, gain, gain.argmax(dim=1)

            def ens_label():
                lib.al_ensemble_label(up.set, ps, pe, up.tlen_h, old_idx=old, out=l_out)
                return l_out

            def loop_label():
                for k in range(K):
                    lib.al_mbr_label(up.set, ps[k], pe[k], up.tlen_h, old_idx=old, out=l1_out)
                return l1_out

            legs = dict(ens_query=ens_query) if a.query_only else dict(ens_query=ens_query, loop_query=loop_query, ens_label=ens_label,
                                                                       loop_label=loop_label)
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
            if not a.query_only:
                out['%s_loop_over_ens_query' % key] = round(out['%s_loop_query_wall_ms' % key] / out['%s_ens_query_wall_ms' % key], 2)
                out['%s_loop_over_ens_label' % key] = round(out['%s_loop_label_wall_ms' % key] / out['%s_ens_label_wall_ms' % key], 2)
                # the two query legs compute the same q(t): the loop's from float32 per-pass values
                live = res['ens_query'][11] == 1
                out['%s_max_incl_diff' % key] = float((res['ens_query'][2] - res['loop_query'][1]).abs()[live].max())
    if not a.query_only:
        # the same launch without the walk, in a child process on the measuring build
        if not os.path.exists(NOWALK):
            from hual_amd import build as hb
            hb.build(out=NOWALK, defines=['HUAL_ENS_NO_WALK'])
        cmd = [sys.executable, os.path.abspath(__file__), '--query-only', '--k', str(K), '--answers', str(a.answers), '--rounds', str(a.rounds),
               '--n'] + [str(n) for n in a.n] + ['--t'] + [str(t) for t in a.t]
        child = json.loads(subprocess.run(cmd, env=dict(os.environ, HUAL_LIB_PATH=NOWALK), stdout=subprocess.PIPE, check=True,
                                          timeout=600).stdout.decode().strip().splitlines()[-1])
        for N in a.n:
            for T in a.t:
                key = 'N%d_T%d' % (N, T)
                out['%s_ens_query_nowalk_device_ms' % key] = child['%s_ens_query_device_ms' % key]
                out['%s_post_entropy_walk_device_ms' % key] = round(out['%s_ens_query_device_ms' % key] - child['%s_ens_query_device_ms' % key], 3)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
