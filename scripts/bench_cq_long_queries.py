"""Context-query attention of long queries: device time of the forward and the backward kernels per padded shape, on this build and on
the paths it replaces.  The library's own profiler (hual_prof_begin / hual_prof_end: device events around every launch) times --iters
calls of hual_cq_attn_fwd + hual_cq_attn_bwd after warm-up; the time of a side is the sum over the context-query kernels it launches
(forward: cq_fwd_* and tri_prep_kernel, backward: cq_bwd_* without cq_bwd_pre_kernel, which every path runs).  Every variant runs in a
child process of its own (HUAL_CQ_NO_WIDE and HUAL_LIB_PATH are read once per process), --rounds interleaved rounds, medians.

    python scripts/bench_cq_long_queries.py [--iters 200] [--rounds 5] [--shapes 16x100x32,16x100x33,...] [--parent-lib path/to/parent.so]
Variants: `wide` (this build), `no_wide` (this build, HUAL_CQ_NO_WIDE=1), `parent` (--parent-lib: a library built from the parent commit).
One JSON line per (shape, variant) with the per-round figures, the median and the spread (max - min over the rounds).
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = '16x100x32,16x100x33,16x100x45,16x100x64,32x128x64'


def _child(shapes, iters):
    import numpy as np
    import torch
    from bench import synth_batch
    from hual_amd import lib
    from hual_amd.model import SeqPAN
    dev = torch.device('cuda:0')
    wv = np.random.default_rng(777).normal(0, 0.4, size=(998, 300)).astype(np.float32)
    l = lib.load()
    res = {}
    for (B, T, L) in shapes:
        cfg = lib.make_cfg(vdim=64, max_vlen=max(T, L), num_words=1000, num_chars=40)
        m = SeqPAN(cfg, wv, device=dev, seed=12345, rng_seed=12345)
        b = synth_batch(B, T, L, 8, 64, 1000, 40, 12345)
        b['lens'][0] = T                                     # (the padded length is the longest clip's)
        bt, keep, _ = m._prep(b['video'], b['lens'], b['word_ids'], b['char_ids'])
        ws = m._workspace(B, T, L, 8)
        opts = m._opts(0.2)
        R = B * (T + L)
        g = torch.Generator().manual_seed(1)
        x, dy = torch.randn(R, 128, generator=g).to(dev), torch.randn(R, 128, generator=g).to(dev)
        feats, dx, grads = torch.empty_like(x), torch.empty_like(x), torch.zeros_like(m.params)
        head = [ctypes.byref(m.cfg), lib.ptr(m.params), ctypes.byref(bt), ctypes.byref(opts)]
        tail = [lib.ptr(ws), ws.numel(), lib.stream_ptr()]

        def call():
            lib.check(l.hual_cq_attn_fwd(*head, lib.ptr(x), lib.ptr(feats), *tail))
            lib.check(l.hual_cq_attn_bwd(*head, lib.ptr(dy), lib.ptr(dx), lib.ptr(grads), *tail))
        for _ in range(20):
            call()
        torch.cuda.synchronize()
        lib.check(l.hual_prof_begin())
        for _ in range(iters):
            call()
        n = l.hual_prof_end()
        fwd = bwd = 0.0
        names = []
        for i in range(n):
            name = ctypes.create_string_buffer(256)
            cnt, us = ctypes.c_int64(), ctypes.c_double()
            lib.check(l.hual_prof_get(i, name, 256, ctypes.byref(cnt), ctypes.byref(us), None, None))
            k = name.value.decode()
            if k.startswith('cq_fwd') or k.startswith('tri_prep'):
                fwd += us.value / iters
                names.append(k)
            elif k.startswith('cq_bwd') and not k.startswith('cq_bwd_pre'):
                bwd += us.value / iters
                names.append(k)
        res['%dx%dx%d' % (B, T, L)] = dict(fwd_us=round(fwd, 2), bwd_us=round(bwd, 2), kernels=sorted(names))
    print('RESULT ' + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--shapes', default=SHAPES)
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--child', action='store_true')
    a = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split('x')) for s in a.shapes.split(',')]
    if a.child:
        return _child(shapes, a.iters)
    variants = [('wide', {}), ('no_wide', {'HUAL_CQ_NO_WIDE': '1'})]
    if a.parent_lib:
        variants.append(('parent', {'HUAL_LIB_PATH': os.path.abspath(a.parent_lib)}))
    runs = {v: [] for v, _ in variants}
    for rnd in range(a.rounds):
        for v, env in variants:                              # interleaved: every round visits every variant
            r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', '--iters', str(a.iters), '--shapes', a.shapes],
                               env=dict(os.environ, **env), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
            line = [x for x in r.stdout.decode().splitlines() if x.startswith('RESULT ')]
            if r.returncode != 0 or not line:
                sys.stderr.write(r.stdout.decode()[-4000:])
                raise SystemExit('variant %s failed (exit status %d): nothing more is started' % (v, r.returncode))
            runs[v].append(json.loads(line[0][7:]))
    for s in a.shapes.split(','):
        for v, _ in variants:
            f, b = [r[s]['fwd_us'] for r in runs[v]], [r[s]['bwd_us'] for r in runs[v]]
            print(json.dumps(dict(shape=s, variant=v, fwd_us=statistics.median(f), bwd_us=statistics.median(b),
                                  fwd_spread=round(max(f) - min(f), 2), bwd_spread=round(max(b) - min(b), 2), fwd_rounds=f, bwd_rounds=b,
                                  kernels=runs[v][0][s]['kernels'])))


if __name__ == '__main__':
    main()
