#!/usr/bin/env python3
"""What training on the span posterior costs: the hual_al_span_marginals launch over a whole training set, and the epoch loop with the
soft-label banks in the batch assembly beside the loop without them.
  marginals   N samples of T frames (random logits, v_len in [T / 2, T]) with 0 and with 3 truthful active points per sample, at the
              Charades set size and T = 64, and at T = 256.  Kernel time by the library's own profiling hook (hual_prof_begin /
              hual_prof_end: the begin / end timestamps of the dispatch), --iters launches after one unprofiled warm-up.
  loop        shuffled epochs over the synthetic set of bench.py's epoch-loop leg (4096 samples, vdim 1024, clips of 64..128 frames,
              batch 64; tests/al_synth.py), two datasets and two trainers on one model in one process: banks not enabled, and banks
              enabled with every weight 1 (dense random rows).  Two untimed epochs each (eager launches, captures), then --epochs timed
              epochs ALTERNATING between the two; host clock around run_epoch between device synchronisations.  ms/step as the mean
              over the timed epochs, with the smallest and largest epoch beside it: the spread a difference has to exceed.
  --parent DIR  a built checkout of the parent commit: the banks-not-enabled loop is timed again in fresh child processes, this tree
              and DIR alternating, --reps each (`--loop-only --root DIR` is what a child runs).
    python scripts/bench_soft_labels.py [--n 12404] [--iters 5] [--epochs 6] [--parent DIR] [--reps 3]
Prints one JSON line (microseconds per launch, milliseconds per step)."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def marginals(a, out):
    import torch
    from hual_amd import al, lib
    l = lib.load()
    for ld in (64, 256):
        g = np.random.default_rng(5)
        N = a.n
        vlen = g.integers(ld // 2, ld + 1, size=N)
        lg = (g.standard_normal((2, N, ld)) * 2).astype(np.float32)
        prop = [{'vid': 'v%d' % n, 'v_len': int(vlen[n]), 'prop_logits': [lg[0, n], lg[1, n]], 'prop_logits1': [lg[0, n], lg[1, n]],
                 'prop_logits2': [lg[0, n], lg[1, n]]} for n in range(N)]
        aps3 = []
        for n in range(N):
            s = int(g.integers(0, vlen[n]))
            e = int(g.integers(s, vlen[n]))
            aps3.append([(int(f), bool(s <= f <= e)) for f in g.choice(int(vlen[n]), size=3, replace=False)])
        for k, aps in ((0, [[] for _ in range(N)]), (3, aps3)):
            u = al.LabelUpdater(prop, aps)
            u.span_marginals()                                        # (warm-up)
            torch.cuda.synchronize()
            lib.check(l.hual_prof_begin())
            for _ in range(a.iters):
                u.span_marginals()
            torch.cuda.synchronize()
            for i in range(l.hual_prof_end()):
                name = ctypes.create_string_buffer(256)
                cnt, us = ctypes.c_int64(), ctypes.c_double()
                lib.check(l.hual_prof_get(i, name, 256, ctypes.byref(cnt), ctypes.byref(us), None, None))
                assert cnt.value == a.iters
                out['%s_T%d_ap%d_us' % (name.value.decode().replace('_kernel', ''), ld, k)] = round(us.value / cnt.value, 1)
            out['live_T%d_ap%d' % (ld, k)] = int((u.marg_status == 1).sum())


def loop(a, root, soft):
    """ms/step of every timed epoch: {'plain': [...]} and, with soft, {'soft': [...]} from epochs alternating with the plain ones"""
    import torch
    sys.path.insert(0, os.path.join(root, 'tests'))
    import al_synth
    from hual_amd import al, lib
    from hual_amd.dataset import DeviceDataset
    from hual_amd.model import SeqPAN
    from hual_amd.train import Trainer
    N, vdim, max_vlen, L, bs = a.samples, 1024, 128, 20, 64
    recs, vis, data_gt, _ = al_synth.make_trainset(N, 512, vdim, max_vlen, seed=11, num_words=1000, num_chars=40, max_words=L)
    cfg = lib.make_cfg(vdim=vdim, max_vlen=max_vlen, num_words=1000, num_chars=40)
    wv = np.random.default_rng(777).normal(0, 0.4, size=(998, 300)).astype(np.float32)
    model = SeqPAN(cfg, wv, seed=12345, rng_seed=12345)
    legs = {}
    for name in ('plain', 'soft') if soft else ('plain',):
        ds = DeviceDataset(recs, vis)
        ds.set_labels(*al.labels_from_times(data_gt, ds.vlen_h))
        if name == 'soft':
            g = torch.Generator(device=ds.dev).manual_seed(3)
            y = torch.rand(2, N, int(ds.vlen_h.max()), device=ds.dev, generator=g)
            y = y / y.sum(2, keepdim=True)
            ds.set_soft_labels(y[0], y[1], np.ones(N, dtype=np.float32))
        legs[name] = (ds, Trainer(model, world=1, use_graph=True))
    nsteps = (N + bs - 1) // bs
    g = np.random.default_rng(0)

    def epoch(name):
        ds, tr = legs[name]
        order = g.permutation(N)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tr.run_epoch(ds, order, bs, lr=1e-4, drop_rate=0.2, min_chars=4)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / nsteps * 1e3
    for _ in range(2):
        for name in legs:
            epoch(name)
    ms = {name: [] for name in legs}
    for _ in range(a.epochs):
        for name in legs:
            ms[name].append(round(epoch(name), 4))
    return ms


def summary(xs):
    return dict(ms_per_step=round(float(np.mean(xs)), 4), min=round(float(np.min(xs)), 4), max=round(float(np.max(xs)), 4), epochs=len(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=12404)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--samples', type=int, default=4096)
    ap.add_argument('--epochs', type=int, default=6)
    ap.add_argument('--parent', default=None, help='a built checkout of the parent commit to time the plain loop of')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--loop-only', action='store_true', help='print the ms/step of the timed epochs of the plain loop (a child of --parent)')
    ap.add_argument('--root', default=HERE, help='the checkout whose hual_amd is imported')
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_soft_labels: no GPU - nothing is measured without one')
    if a.loop_only:
        print(json.dumps(loop(a, root, soft=False)['plain']))
        return
    out = dict(n_samples=a.n, iters=a.iters)
    marginals(a, out)
    ms = loop(a, root, soft=True)
    out['loop'] = dict(samples=a.samples, batch=64, banks_not_enabled=summary(ms['plain']), banks_all_weights_1=summary(ms['soft']))
    if a.parent:
        runs = {'this': [], 'parent': []}
        for _ in range(a.reps):                                       # fresh processes, alternating
            for name, r in (('this', HERE), ('parent', os.path.abspath(a.parent))):
                cmd = [sys.executable, os.path.abspath(__file__), '--loop-only', '--root', r, '--samples', str(a.samples), '--epochs', str(a.epochs)]
                res = subprocess.run(cmd, stdout=subprocess.PIPE, check=True, timeout=600)
                runs[name] += json.loads(res.stdout.decode().strip().splitlines()[-1])
        out['loop_vs_parent'] = dict(this=summary(runs['this']), parent=summary(runs['parent']), processes_each=a.reps)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
