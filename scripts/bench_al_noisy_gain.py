#!/usr/bin/env python3
"""What the noisy label gain costs: hual_al_label_gain_noisy over every frame and over M listed frames per sample, beside
hual_al_label_gain on the same logits with no answers (the nearest equivalent under the hard rule), from the same build on the same
synthetic set - N samples of exactly ld frames (random logits, 3 answers per sample of which a seeded 30 % are flipped, folded into the
rows by one hual_al_noisy_tilt).  Kernel times by the library's own profiling hook (hual_prof_begin / hual_prof_end: the begin / end
timestamps of each dispatch), the mean of --iters launches of each kind after one unprofiled warm-up.
    python scripts/bench_al_noisy_gain.py [--n 256] [--ld 64] [--iters 2] [--cand 8] [--eps 0.1]
Prints one JSON line (microseconds per launch)."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=256)
    ap.add_argument('--ld', type=int, default=64)
    ap.add_argument('--iters', type=int, default=2)
    ap.add_argument('--cand', type=int, default=8)
    ap.add_argument('--eps', type=float, default=0.1)
    a = ap.parse_args()
    import torch
    from hual_amd import al, lib
    if not torch.cuda.is_available():
        raise SystemExit('bench_al_noisy_gain: no GPU - nothing is measured without one')
    l = lib.load()
    g = np.random.default_rng(5)
    N, ld = a.n, a.ld
    lg = (g.standard_normal((2, N, ld)) * 2).astype(np.float32)
    prop = [{'vid': 'v%d' % n, 'v_len': ld, 'prop_logits': [lg[0, n], lg[1, n]], 'prop_logits1': [lg[0, n], lg[1, n]],
             'prop_logits2': [lg[0, n], lg[1, n]]} for n in range(N)]
    aps = []
    for n in range(N):
        s = int(g.integers(0, ld))
        e = int(g.integers(s, ld))
        aps.append([(int(f), bool(s <= f <= e) != bool(g.random() < 0.3)) for f in g.choice(ld, size=3, replace=False)])
    noisy = al.LabelUpdater(prop, aps)
    hard = al.LabelUpdater(prop, [[] for _ in range(N)])
    noisy.query(noise=a.eps)
    cand = (noisy.query_point[:, None] + torch.arange(a.cand, dtype=torch.int32, device=noisy.dev)[None, :] - a.cand // 2).contiguous()
    runs = (('al_label_gain_noisy_all', lambda: noisy.label_gain(frames=False, noise=a.eps)),
            ('al_label_gain_noisy_cand%d' % a.cand, lambda: noisy.label_gain(frames=False, noise=a.eps, cand=cand)),
            ('al_label_gain_all', lambda: hard.label_gain(frames=False)),
            ('al_label_gain_cand%d' % a.cand, lambda: hard.label_gain(frames=False, cand=cand)))
    out = dict(n_samples=N, ld=ld, iters=a.iters, eps=a.eps)
    for name, fn in runs:
        fn()                                                          # (warm-up)
        torch.cuda.synchronize()
        lib.check(l.hual_prof_begin())
        for _ in range(a.iters):
            fn()
        torch.cuda.synchronize()
        assert l.hual_prof_end() == 1
        cnt, us = ctypes.c_int64(), ctypes.c_double()
        lib.check(l.hual_prof_get(0, ctypes.create_string_buffer(256), 256, ctypes.byref(cnt), ctypes.byref(us), None, None))
        assert cnt.value == a.iters
        out[name + '_us'] = round(us.value / cnt.value, 1)
    out['mean_ask_gain_noisy'] = round(float(noisy.ask_gain.clamp(min=0).mean()), 4)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
