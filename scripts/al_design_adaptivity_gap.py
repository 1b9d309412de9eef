#!/usr/bin/env python3
"""What asking a clip's frames at once gives up: the expected information of the greedy design of M frames (hual_al_design's, by the
float64 enumeration of tests/al_design_ref.py) beside the expected information of the adaptive greedy tree of the same depth
(hual_al_session's policy, every answer drawn from the posterior itself), on the rows of the seeded T = 33 case the tests share, with no
answer yet.  CPU only, float64; no device is touched.
    python scripts/al_design_adaptivity_gap.py [--t 33] [--m 3 6]
Prints one JSON line (bits)."""
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
    ap.add_argument('--t', type=int, default=33)
    ap.add_argument('--m', type=int, nargs='+', default=[3, 6])
    a = ap.parse_args()
    import al_design_ref as D
    import al_query_ref as Q
    out = dict(T=a.t, rows=0)
    rows = [D.case_row(a.t, 0, n) for n in range(Q.N_ROWS)]
    rows = [r for r in rows if r.status == Q.LIVE and r.post['query_gain'] > 0]
    out['rows'] = len(rows)
    out['mean_entropy_bits'] = round(float(np.mean([r.H for r in rows])), 4)
    for M in a.m:
        design = np.array([(D.greedy(r, M)['info'] or [0.0])[-1] for r in rows])
        tree = np.array([D.adaptive_tree(r, M) for r in rows])
        gap = tree - design
        out['M%d' % M] = dict(design_bits=round(float(design.mean()), 4), adaptive_bits=round(float(tree.mean()), 4),
                              gap_bits=round(float(gap.mean()), 4), gap_max_bits=round(float(gap.max()), 4),
                              gap_min_bits=round(float(gap.min()), 4), design_share=round(float(design.sum() / tree.sum()), 4))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
