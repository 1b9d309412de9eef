"""Cost of train.ema_decay on the GPU box: ms per training step (one replayed step graph: forward, backward, clip + AdamWeightDecay) at
the c2 shape (B=64, T=128, L=20, C=8, vdim 1024) without and with the averaged weights riding in the optimizer launch, and the device
time of the two optimizer launches alone (the library's own per-launch events).  The two models are timed in interleaved rounds (same
box, same clocks); one JSON line per model with the median over the rounds, then one summary line.

    python scripts/bench_ema.py [--steps 200] [--rounds 5] [--rows 1500]
"""
import argparse
import ctypes
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


def optimizer_us(model, iters):
    """device microseconds per launch of sqnorm_kernel and adamw_kernel (hual_prof_begin / hual_prof_end) over `iters` optimizer calls
    on the model's own buffers, gradient as the last step left it"""
    l = lib.load()
    for _ in range(20):
        model.optimizer_launch(1.0)
    torch.cuda.synchronize()
    lib.check(l.hual_prof_begin())
    for _ in range(iters):
        model.optimizer_launch(1.0)
    torch.cuda.synchronize()
    n = l.hual_prof_end()
    got = {}
    for i in range(n):
        name = ctypes.create_string_buffer(256)
        cnt, us = ctypes.c_int64(), ctypes.c_double()
        lib.check(l.hual_prof_get(i, name, 256, ctypes.byref(cnt), ctypes.byref(us), None, None))
        got[name.value.decode()] = us.value / max(cnt.value, 1)
    return got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--prewarm', type=int, default=200)
    ap.add_argument('--rows', type=int, default=1500)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--T', type=int, default=128)
    ap.add_argument('--L', type=int, default=20)
    ap.add_argument('--C', type=int, default=8)
    ap.add_argument('--vdim', type=int, default=1024)
    ap.add_argument('--decay', type=float, default=0.999)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    num_words = a.rows + 2
    wv = np.random.default_rng(777).normal(0, 0.4, size=(a.rows, 300)).astype(np.float32)
    b = synth_batch(a.batch, a.T, a.L, a.C, a.vdim, num_words, 40, 12345)
    runs = []
    for decay in (0.0, a.decay):
        cfg = lib.make_cfg(vdim=a.vdim, max_vlen=max(a.T, a.L), num_words=num_words, num_chars=40)
        model = SeqPAN(cfg, wv, device=dev, seed=12345, rng_seed=12345, ema_decay=decay)
        tr = Trainer(model, world=1, use_graph=True)
        tr.set_batch(b['video'], b['lens'], b['word_ids'], b['char_ids'], b['y1'], b['y2'], b['match'], b['inner'])
        runs.append(dict(ema=decay, floats=int(model.params.numel()), tr=tr, ms=[]))
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
        opt = optimizer_us(r['tr'].m, a.steps)
        med[r['ema'] > 0] = (ms, opt)
        print(json.dumps(dict(bench='ema', ema_decay=r['ema'], flat_floats=r['floats'], B=a.batch, T=a.T, L=a.L,
                              ms_per_step=round(ms, 4), ms_rounds=[round(x, 4) for x in r['ms']],
                              optimizer_us={k: round(v, 2) for k, v in opt.items()}, loss=round(float(r['tr'].last_loss()), 4))))
    print(json.dumps(dict(bench='ema', summary=dict(
        off_ms=round(med[False][0], 4), on_ms=round(med[True][0], 4), extra_us=round((med[True][0] - med[False][0]) * 1e3, 1),
        adamw_off_us=round(med[False][1].get('adamw_kernel', 0.0), 2), adamw_on_us=round(med[True][1].get('adamw_kernel', 0.0), 2)))))


if __name__ == '__main__':
    main()
