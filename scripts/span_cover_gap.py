"""How much more a clip's greedy Bayes set covers than its NMS proposals (CPU, the float64 enumeration of tests/span_cover_ref.py, no
GPU): per (T, scale) 64 full-length rows of logits scale * N(0, 1), k = 5, thresholds 3/10, 1/2, 7/10 - the mean coverage of the
greedy set of k spans and of the k proposals of the top-k rule at nms_iou = 0.5 (tests/span_topk_ref.py), and the share of rows whose
two sets differ as sets.  Random logits, not a trained model's: what the difference does to R@k on real data is not known.

    python scripts/span_cover_gap.py [--rows 64] [--k 5] [--cases 33x1,70x1,70x3]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import span_cover_ref as V  # noqa: E402
import span_topk_ref as R  # noqa: E402

THRESHOLDS = [(3, 10), (1, 2), (7, 10)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=64)
    ap.add_argument('--k', type=int, default=5)
    ap.add_argument('--nms-iou', type=float, default=0.5)
    ap.add_argument('--cases', default='33x1,70x1,70x3')
    a = ap.parse_args()
    for case in a.cases.split(','):
        T, scale = (int(x) for x in case.split('x'))
        g = torch.Generator().manual_seed(1000 * 7 + 10 * T + scale)
        s, e = torch.randn(a.rows, T, generator=g) * scale, torch.randn(a.rows, T, generator=g) * scale
        vl = torch.full((a.rows,), T, dtype=torch.int32)
        st, en, _ = R.span_topk_ref(s, e, vl, a.k, nms_iou=a.nms_iou)
        greedy, nms, differ = np.zeros((a.rows, 3)), np.zeros((a.rows, 3)), np.zeros((a.rows, 3), dtype=bool)
        for b, c in enumerate(V.clips(s, e, vl, THRESHOLDS)):
            props = [(int(x), int(y)) for x, y in zip(st[b], en[b])]
            for m in range(3):
                spans, prob, _, _ = c.greedy(m, a.k, 0.0)
                greedy[b, m], nms[b, m] = prob[-1], c.coverage(m, props)[-1]
                differ[b, m] = set(spans) != set(props)
        print(json.dumps(dict(T=T, scale=scale, rows=a.rows, k=a.k, nms_iou=a.nms_iou,
                              greedy_coverage=[round(float(x), 3) for x in greedy.mean(axis=0)],
                              nms_coverage=[round(float(x), 3) for x in nms.mean(axis=0)],
                              sets_differ=[round(float(x), 3) for x in differ.mean(axis=0)],
                              greedy_below_nms_rows=[int(x) for x in (greedy < nms - 1e-12).sum(axis=0)])))


if __name__ == '__main__':
    main()
