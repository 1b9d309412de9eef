"""Cost of model.finetune_word_emb on the GPU box: ms per training step (one replayed step graph: forward, backward, clip +
AdamWeightDecay) at the c2 shape (B=64, T=128, L=20, C=8, vdim 1024), with the word table frozen and trainable, for a Charades-sized
and an ActivityNet-sized synthetic vocabulary.  The four models are timed in interleaved rounds (same box, same clocks); one JSON
line per (rows, flag) with the median over the rounds, then one summary line.

    python scripts/bench_finetune.py [--steps 200] [--rounds 5] [--rows 1500,12000]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import synth_batch  # noqa: E402
from hual_amd import lib  # noqa: E402
from hual_amd.model import SeqPAN  # noqa: E402
from hual_amd.train import Trainer  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--prewarm', type=int, default=200)
    ap.add_argument('--rows', default='1500,12000')
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--T', type=int, default=128)
    ap.add_argument('--L', type=int, default=20)
    ap.add_argument('--C', type=int, default=8)
    ap.add_argument('--vdim', type=int, default=1024)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    runs = []
    for rows in (int(x) for x in a.rows.split(',')):
        num_words = rows + 2
        wv = np.random.default_rng(777).normal(0, 0.4, size=(rows, 300)).astype(np.float32)
        b = synth_batch(a.batch, a.T, a.L, a.C, a.vdim, num_words, 40, 12345)
        for ft in (0, 1):
            cfg = lib.make_cfg(vdim=a.vdim, max_vlen=max(a.T, a.L), num_words=num_words, num_chars=40, finetune_word_emb=ft)
            model = SeqPAN(cfg, wv, device=dev, seed=12345, rng_seed=12345)
            tr = Trainer(model, world=1, use_graph=True)
            tr.set_batch(b['video'], b['lens'], b['word_ids'], b['char_ids'], b['y1'], b['y2'], b['match'], b['inner'])
            runs.append(dict(rows=rows, finetune=ft, floats=int(model.params.numel()), tr=tr, ms=[]))
    for r in runs:                      # capture every step graph and ramp the clocks before anything is timed
        for _ in range(a.prewarm // len(runs) + 10):
            r['tr'].step(lr=1e-4, drop_rate=0.2)
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for r in runs:
            for _ in range(10):
                r['tr'].step(lr=1e-4, drop_rate=0.2)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                r['tr'].step(lr=1e-4, drop_rate=0.2)
            torch.cuda.synchronize()
            r['ms'].append((time.perf_counter() - t0) * 1e3 / a.steps)
    med = {}
    for r in runs:
        ms = float(np.median(r['ms']))
        med[(r['rows'], r['finetune'])] = ms
        print(json.dumps(dict(bench='finetune_word_emb', rows=r['rows'], finetune=r['finetune'], flat_floats=r['floats'], B=a.batch,
                              T=a.T, L=a.L, ms_per_step=round(ms, 4), ms_rounds=[round(x, 4) for x in r['ms']],
                              loss=round(float(r['tr'].last_loss()), 4))))
    print(json.dumps(dict(bench='finetune_word_emb', summary={
        str(rows): dict(frozen_ms=round(med[(rows, 0)], 4), finetune_ms=round(med[(rows, 1)], 4),
                        extra_us=round((med[(rows, 1)] - med[(rows, 0)]) * 1e3, 1))
        for rows in sorted({k[0] for k in med})})))


if __name__ == '__main__':
    main()
