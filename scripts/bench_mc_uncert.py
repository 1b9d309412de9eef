#!/usr/bin/env python3
"""Cost of the K-pass uncertainty bank on the bench_al_round set (4096 samples, batch 64, max_vlen 100): infer_trainset with
mc_dropout=0.5 as it always ran (two stochastic passes, their logits fetched) against mc_samples=2 and mc_samples=8 folded into a McBank,
and the fold launch alone.  Device events; medians of --rounds interleaved rounds (one warm-up round first).
    python scripts/bench_mc_uncert.py [--n 4096] [--batch 64] [--max-vlen 100] [--rounds 5]
Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=4096)
    ap.add_argument('--videos', type=int, default=1024)
    ap.add_argument('--vdim', type=int, default=1024)
    ap.add_argument('--max-vlen', type=int, default=100)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--fold-iters', type=int, default=200)
    a = ap.parse_args()
    import torch
    import al_synth
    from hual_amd import al, lib
    from hual_amd.dataset import DeviceDataset
    from hual_amd.model import SeqPAN
    recs, vis, data_gt, data_old = al_synth.make_trainset(a.n, a.videos, a.vdim, a.max_vlen, seed=11, num_words=1000, num_chars=40,
                                                          max_words=20)
    Lm = max(len(r['w_ids']) for r in recs)
    cfg = lib.make_cfg(vdim=a.vdim, max_vlen=max(a.max_vlen, Lm), num_words=1000, num_chars=40)
    wv = np.random.default_rng(777).normal(0, 0.4, size=(998, 300)).astype(np.float32)
    model = SeqPAN(cfg, wv, rng_seed=12345)
    ds = DeviceDataset(recs, vis)
    s0, e0 = al.labels_from_times(data_old, ds.vlen_h)
    ds.set_labels(s0, e0)
    for r, x, y in zip(recs, s0, e0):
        r['s_ind'], r['e_ind'] = int(x), int(y)
    bank = al.McBank.for_dataset(ds)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    legs = {'two_passes_fetched_ms': lambda: al.infer_trainset_sharded(model, ds, a.batch, mc_dropout=0.5),
            'bank_k2_ms': lambda: al.infer_trainset_sharded(model, ds, a.batch, mc_dropout=0.5, mc_samples=2, bank=bank),
            'bank_k8_ms': lambda: al.infer_trainset_sharded(model, ds, a.batch, mc_dropout=0.5, mc_samples=8, bank=bank)}
    times = {k: [] for k in legs}
    for rnd in range(a.rounds + 1):                 # round 0 warms up (module load, workspace sizes, pinned buffers)
        for k, fn in legs.items():
            t = timed(fn)
            if rnd:
                times[k].append(t)
    out = dict(n_samples=a.n, batch=a.batch, max_vlen=a.max_vlen, rounds=a.rounds)
    for k, v in times.items():
        out[k] = round(float(np.median(v)), 2)
        out[k.replace('_ms', '_spread_ms')] = [round(float(min(v)), 2), round(float(max(v)), 2)]
    # the fold launch alone: one batch's logits into 64 rows, back to back
    B, T = a.batch, a.max_vlen
    g = torch.Generator(device='cuda').manual_seed(1)
    s, e = torch.randn(B, T, device='cuda', generator=g), torch.randn(B, T, device='cuda', generator=g)
    v = torch.full((B,), T, dtype=torch.int32, device='cuda')
    rows = bank.rows(np.arange(B))
    for name, k in (('fold_k0_us', 0), ('fold_k1_us', 1), ('fold_k2_us', 2)):
        for _ in range(20):
            bank.fold(rows, v, s, e, k, _checked=True)
        ms = timed(lambda: [bank.fold(rows, v, s, e, k, _checked=True) for _ in range(a.fold_iters)])
        out[name] = round(ms * 1000.0 / a.fold_iters, 2)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
