#!/usr/bin/env python3
"""What the minimum-Bayes-risk pseudo-label costs beside the launches of the label update it sits among: hual_al_mbr_label,
hual_al_renew (both over the selected half of the set, as update_labels launches them) and hual_al_query (over the whole set) from the
same build on the same synthetic set - N samples of ld frames (random logits, v_len in [ld / 2, ld]), with 0 and with 3 truthful
active points per sample.  Kernel times by the library's own profiling hook (hual_prof_begin / hual_prof_end: the begin / end
timestamps of each dispatch), --iters launches of each kind per history after one unprofiled warm-up round.
    python scripts/bench_al_label.py [--n 12403] [--ld 64] [--iters 5]
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
    a = ap.parse_args()
    import torch
    from hual_amd import al, lib
    if not torch.cuda.is_available():
        raise SystemExit('bench_al_label: no GPU - nothing is measured without one')
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
    coff = al.get_coff('charades', 1)
    out = dict(n_samples=N, n_selected=int(len(sel)), ld=ld, iters=a.iters)
    for k, aps in ((0, [[] for _ in range(N)]), (3, aps3)):
        u = al.LabelUpdater(prop, aps)
        u.score(coff[6])                                              # sprob / eprob for the renew

        def once():
            u.renew(sel, old, coff)
            u.query(frames=False)
            return u.mbr_label(sel, old)
        once()                                                        # (warm-up)
        torch.cuda.synchronize()
        lib.check(l.hual_prof_begin())
        for _ in range(a.iters):
            lab = once()
        torch.cuda.synchronize()
        for i in range(l.hual_prof_end()):
            name = ctypes.create_string_buffer(256)
            cnt, us = ctypes.c_int64(), ctypes.c_double()
            lib.check(l.hual_prof_get(i, name, 256, ctypes.byref(cnt), ctypes.byref(us), None, None))
            assert cnt.value == a.iters
            out['%s_ap%d_us' % (name.value.decode().replace('_kernel', ''), k)] = round(us.value / cnt.value, 1)
        out['labelled_ap%d' % k] = int((lab[0][sel, 0] >= 0).sum())
        out['mean_conf_ap%d' % k] = round(float(lab[1][sel].mean()), 4)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
