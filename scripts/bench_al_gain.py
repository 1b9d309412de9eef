#!/usr/bin/env python3
"""What acquisition by expected label gain costs beside the posterior launches it builds on: hual_al_label_gain over every frame of the
whole set (as update_labels(acquire_by='label_gain') launches it), hual_al_query (over the whole set) and hual_al_mbr_label (over the
selected half) from the same build on the same synthetic set - N samples of ld frames (random logits, v_len in [ld / 2, ld]), with 0
and with 3 truthful active points per sample.  Kernel times by the library's own profiling hook (hual_prof_begin / hual_prof_end: the
begin / end timestamps of each dispatch), the mean of --iters launches of each kind per history after one unprofiled warm-up round.
--cand M also times the launch over M listed frames per sample (the frame of most information and the frames around it).
    python scripts/bench_al_gain.py [--n 12403] [--ld 64] [--iters 5] [--cand 0]
Prints one JSON line (microseconds per launch)."""
import argparse
import ctypes
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=12403)
    ap.add_argument('--ld', type=int, default=64)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--cand', type=int, default=0)
    a = ap.parse_args()
    import torch
    from hual_amd import al, lib
    if not torch.cuda.is_available():
        raise SystemExit('bench_al_gain: no GPU - nothing is measured without one')
    l = lib.load()
    g = np.random.default_rng(5)
    N, ld = a.n, a.ld
    vlen = g.integers(ld // 2, ld + 1, size=N)
    lg = (g.standard_normal((2, N, ld)) * 2).astype(np.float32)
    prop = [{'vid': 'v%d' % n, 'v_len': int(vlen[n]), 'prop_logits': [lg[0, n], lg[1, n]], 'prop_logits1': [lg[0, n], lg[1, n]],
             'prop_logits2': [lg[0, n], lg[1, n]]} for n in range(N)]
    aps3, old = [], np.zeros((N, 2), dtype=np.int32)
    for n in range(N):
        s = int(g.integers(0, vlen[n]))
        e = int(g.integers(s, vlen[n]))
        old[n] = s, e
        aps3.append([(int(f), bool(s <= f <= e)) for f in g.choice(int(vlen[n]), size=3, replace=False)])
    sel = np.sort(g.permutation(N)[:math.ceil(N / 2)])
    out = dict(n_samples=N, n_selected=int(len(sel)), ld=ld, iters=a.iters, cand=a.cand)
    for k, aps in ((0, [[] for _ in range(N)]), (3, aps3)):
        u = al.LabelUpdater(prop, aps)

        def once():
            u.query(frames=False)
            u.mbr_label(sel, old)
            u.label_gain(frames=False)
        once()                                                        # (warm-up)
        torch.cuda.synchronize()
        lib.check(l.hual_prof_begin())
        for _ in range(a.iters):
            once()
        torch.cuda.synchronize()
        for i in range(l.hual_prof_end()):
            name = ctypes.create_string_buffer(256)
            cnt, us = ctypes.c_int64(), ctypes.c_double()
            lib.check(l.hual_prof_get(i, name, 256, ctypes.byref(cnt), ctypes.byref(us), None, None))
            assert cnt.value == a.iters
            out['%s_ap%d_us' % (name.value.decode().replace('_kernel', ''), k)] = round(us.value / cnt.value, 1)
        out['asked_ap%d' % k] = int((u.ask_gain > 0).sum())
        out['mean_ask_gain_ap%d' % k] = round(float(u.ask_gain.clamp(min=0).mean()), 4)
        if a.cand:
            # the frames around the frame of most information, clipped by the kernel itself where they leave the clip
            cand = (u.query_point[:, None] + torch.arange(a.cand, dtype=torch.int32, device=u.dev)[None, :] - a.cand // 2).contiguous()
            u.label_gain(frames=False, cand=cand)                     # (warm-up)
            torch.cuda.synchronize()
            lib.check(l.hual_prof_begin())
            for _ in range(a.iters):
                u.label_gain(frames=False, cand=cand)
            torch.cuda.synchronize()
            assert l.hual_prof_end() == 1
            cnt, us = ctypes.c_int64(), ctypes.c_double()
            lib.check(l.hual_prof_get(0, ctypes.create_string_buffer(256), 256, ctypes.byref(cnt), ctypes.byref(us), None, None))
            out['al_label_gain_cand%d_ap%d_us' % (a.cand, k)] = round(us.value / cnt.value, 1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
