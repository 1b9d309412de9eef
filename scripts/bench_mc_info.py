#!/usr/bin/env python3
"""What BALD costs over RANGE on the bench_al_round set (4096 samples, batch 64, max_vlen 100): infer_trainset with mc_samples=K folded into
a plain McBank and read as mc_stat='range', against the same pass folded into a McBank(info=True) (hual_al_mc_fold_info: the entropy of
every pass beside the bank) and read as mc_stat='bald', at K = 2 and K = 8; and the two fold launches alone at k = 2.
Device events; medians of --rounds interleaved rounds in one process (one warm-up round first).
    python scripts/bench_mc_info.py [--n 4096] [--batch 64] [--max-vlen 100] [--rounds 5]
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
    banks = {'range': al.McBank.for_dataset(ds), 'bald': al.McBank.for_dataset(ds, info=True)}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def leg(stat, K):
        return lambda: al.infer_trainset_sharded(model, ds, a.batch, mc_dropout=0.5, mc_samples=K, bank=banks[stat], mc_stat=stat)
    legs = {'%s_k%d_ms' % (stat, K): leg(stat, K) for K in (2, 8) for stat in ('range', 'bald')}
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
    for K in (2, 8):
        out['bald_over_range_k%d' % K] = round(out['bald_k%d_ms' % K] / out['range_k%d_ms' % K], 4)
    # the fold launches alone: one batch's logits into 64 rows at k = 2, back to back, the two alternating
    B, T = a.batch, a.max_vlen
    g = torch.Generator(device='cuda').manual_seed(1)
    s, e = torch.randn(B, T, device='cuda', generator=g), torch.randn(B, T, device='cuda', generator=g)
    v = torch.full((B,), T, dtype=torch.int32, device='cuda')
    fold_us = {'fold_k2_us': [], 'fold_info_k2_us': []}
    for rnd in range(a.rounds + 1):
        for name, bank in (('fold_k2_us', banks['range']), ('fold_info_k2_us', banks['bald'])):
            rows = bank.rows(np.arange(B))
            ms = timed(lambda: [bank.fold(rows, v, s, e, 2, _checked=True) for _ in range(a.fold_iters)])
            if rnd:
                fold_us[name].append(ms * 1000.0 / a.fold_iters)
    for name, vals in fold_us.items():
        out[name] = round(float(np.median(vals)), 2)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
