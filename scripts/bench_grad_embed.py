#!/usr/bin/env python3
"""What gradient-embedding acquisition costs.
 1. al.infer_trainset_sharded with and without a GradBank (one hual_al_grad_embed launch per batch) on a synthetic set: N = --n
    samples, batches of --batch, clips of --max-vlen frames (every video has that many, so T is the same in every batch).  Wall clock
    around the whole pass with a synchronisation at its end (host time included), the legs alternating within a round, medians of
    --rounds rounds after a warm-up round.  Also the launch alone and the label-free forward alone on one batch, back to back on the
    device (events around --iters repetitions), and the launch's share of that forward.
 2. hual_kcenter_sample (D^2 sampling from the origin) against hual_kcenter_greedy on the same rows: N(0, 1) float32 [N, 256],
    n_select = N // 2, the same wall clock, alternating legs and medians.
Nothing is gated on the times.
    python scripts/bench_grad_embed.py [--n 4096] [--batch 64] [--max-vlen 128] [--select-n 4096 12403] [--rounds 3]
Prints one JSON line (milliseconds)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=4096)
    ap.add_argument('--videos', type=int, default=1024)
    ap.add_argument('--vdim', type=int, default=1024)
    ap.add_argument('--max-vlen', type=int, default=128)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--select-n', type=int, nargs='+', default=[4096, 12403])
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--iters', type=int, default=50)
    a = ap.parse_args()
    import torch
    import al_synth
    from hual_amd import al, lib
    from hual_amd.dataset import DeviceDataset
    from hual_amd.model import SeqPAN
    if not torch.cuda.is_available():
        raise SystemExit('bench_grad_embed: no GPU - nothing is measured without one')
    dev = torch.device('cuda:0')
    out = dict(n_samples=a.n, batch=a.batch, max_vlen=a.max_vlen, rounds=a.rounds)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def device_ms(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    def report(key, times):
        out[key + '_ms'] = round(float(np.median(times)), 2)
        out[key + '_spread_ms'] = [round(float(min(times)), 2), round(float(max(times)), 2)]

    # ---- 1. the pass over the training set
    recs, vis, data_gt, data_old = al_synth.make_trainset(a.n, a.videos, a.vdim, a.max_vlen, seed=11, num_words=1000, num_chars=40, max_words=20)
    g = np.random.default_rng(5)
    for v in vis:                                                         # every video at the full length: T = max_vlen in every batch
        vis[v] = g.standard_normal((a.max_vlen, a.vdim)).astype(np.float32)
    for r in recs:
        r['v_len'] = a.max_vlen
    Lm = max(len(r['w_ids']) for r in recs)
    cfg = lib.make_cfg(vdim=a.vdim, max_vlen=max(a.max_vlen, Lm), num_words=1000, num_chars=40)
    wv = np.random.default_rng(777).normal(0, 0.4, size=(998, 300)).astype(np.float32)
    model = SeqPAN(cfg, wv, rng_seed=12345)
    ds = DeviceDataset(recs, vis)
    s0, e0 = al.labels_from_times(data_old, ds.vlen_h)
    ds.set_labels(s0, e0)
    for r, x, y in zip(recs, s0, e0):
        r['s_ind'], r['e_ind'] = int(x), int(y)
    bank = al.GradBank.for_dataset(ds)
    legs = {'infer_plain': lambda: al.infer_trainset_sharded(model, ds, a.batch),
            'infer_grad_bank': lambda: al.infer_trainset_sharded(model, ds, a.batch, grad_bank=bank)}
    times = {k: [] for k in legs}
    for rnd in range(a.rounds + 1):                                       # round 0 warms up (module load, workspace, pinned buffers)
        for k, fn in legs.items():
            t = wall(fn)
            if rnd:
                times[k].append(t)
    for k, v in times.items():
        report(k, v)
    out['infer_grad_bank_over_plain'] = round(out['infer_grad_bank_ms'] / out['infer_plain_ms'], 4)
    sel = np.arange(min(a.batch, a.n))
    f = ds.assemble(sel, out=None, labels=False, min_chars=4)
    fwd = lambda: model.forward(f['video'], f['video_seq_len'], f['word_ids'], f['char_ids'])
    o = fwd()
    hyp = torch.stack([o['start_index'], o['end_index']], dim=1).to(torch.int32)
    rows = bank.rows(sel)
    embed = lambda: bank.embed(model, o, f['video_seq_len'], rows, hyp)
    out['forward_one_batch_ms'] = round(device_ms(fwd, a.iters), 4)
    out['grad_embed_one_batch_ms'] = round(device_ms(embed, a.iters), 4)
    out['grad_embed_share_of_forward'] = round(out['grad_embed_one_batch_ms'] / out['forward_one_batch_ms'], 4)
    out['batch_T'] = int(f['video'].shape[1])

    # ---- 2. the sampler against the greedy call
    D = 256
    for N in a.select_n:
        gen = torch.Generator(device='cpu').manual_seed(N + D)
        x = torch.randn(N, D, generator=gen).to(dev)
        n_select = N // 2
        ws = torch.empty(lib.kcenter_workspace_bytes(N), dtype=torch.uint8, device=dev)
        outs = (torch.empty(n_select, dtype=torch.int32, device=dev), torch.empty(n_select, device=dev), torch.empty(N, device=dev),
                torch.empty(N, dtype=torch.int32, device=dev))
        view = lambda k: (outs[0][:k], outs[1][:k], outs[2], outs[3])
        legs = dict(greedy=lambda k=n_select: lib.kcenter_select(x, k, out=view(k), workspace=ws),
                    greedy_origin=lambda k=n_select: lib.kcenter_sample(x, k, sample=False, origin=True, out=view(k), workspace=ws),
                    sample_origin=lambda k=n_select: lib.kcenter_sample(x, k, seed=1, sample=True, origin=True, out=view(k), workspace=ws))
        for fn in legs.values():                                          # warm-up: 64 steps of each
            fn(64)
        torch.cuda.synchronize()
        times = {k: [] for k in legs}
        for _ in range(a.rounds):
            for k, fn in legs.items():
                times[k].append(wall(fn))
        for k, v in times.items():
            report('select_N%d_%s' % (N, k), v)
        out['select_N%d_sample_over_greedy' % N] = round(out['select_N%d_sample_origin_ms' % N] / out['select_N%d_greedy_ms' % N], 3)
        out['select_N%d_sample_us_per_step' % N] = round(1e3 * out['select_N%d_sample_origin_ms' % N] / n_select, 2)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
