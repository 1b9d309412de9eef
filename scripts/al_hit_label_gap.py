#!/usr/bin/env python3
"""What the span of maximal hit probability is worth beside the minimum-Bayes-risk label, and how often it ties (CPU, the float64
enumerations of tests/al_hit_ref.py and tests/al_label_ref.py, no GPU): on the seeded rows of tests/al_query_ref.case(T) - 16 rows per
T, thresholds 3/10, 1/2, 7/10, candidates and truths restricted to the consistent set A -
  beats:  the (row, threshold) cases in which the max-hit member of A exceeds the MBR label's hit probability by more than 1e-6, the
          mean hit probability gained over those cases and the mean expected tIoU given up;
  ties:   the cases whose runner-up lies within 1e-5 of the best, and how many of those at distance exactly 0.
Random logits, not a trained model's: what the trade does to pseudo-label quality on real data is not known.

    python scripts/al_hit_label_gap.py [--t 33 70] [--answers 0 1 3 6]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import al_hit_ref as HL  # noqa: E402
import al_label_ref as L  # noqa: E402
import al_query_ref as Q  # noqa: E402

THRESHOLDS = HL.THR3
MARGIN, TIE = 1e-6, 1e-5


def rows(T, h):
    """per live row of the case: (the hit probability [|A|, 3] of every member, the expected tIoU [|A|] of every member)"""
    c = Q.case(T)
    for n in range(Q.N_ROWS):
        st = HL.state(c['ps'][n], c['pe'][n], int(c['v'][n]), c['aps'][h][n])
        if st['status'] != HL.LIVE:
            continue
        lst = L.state(c['ps'][n], c['pe'][n], int(c['v'][n]), c['aps'][h][n])
        yield HL.cand_prob(st, np.stack([st['ii'], st['jj']], axis=1), THRESHOLDS), L.all_R(lst)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--t', type=int, nargs='+', default=[33, 70])
    ap.add_argument('--answers', type=int, nargs='+', default=list(Q.HISTORIES))
    a = ap.parse_args()
    for T in a.t + [2]:
        for h in (a.answers if T != 2 else [1]):
            beats, gain, loss = np.zeros(3, dtype=int), np.zeros(3), np.zeros(3)
            ties, exact, cases = 0, 0, 0
            for prob, R in rows(T, h):
                mbr = int(np.argmax(R))
                for m in range(3):
                    best = int(np.argmax(prob[:, m]))
                    cases += 1
                    if prob[best, m] - prob[mbr, m] > MARGIN:
                        beats[m] += 1
                        gain[m] += prob[best, m] - prob[mbr, m]
                        loss[m] += R[mbr] - R[best]
                    if len(prob) > 1:
                        d = prob[best, m] - np.delete(prob[:, m], best).max()
                        ties += d < TIE
                        exact += d == 0
            print(json.dumps(dict(T=T, answers=h, cases=cases, beats_mbr=[int(x) for x in beats],
                                  hit_prob_gained=[round(float(x / b), 3) if b else None for x, b in zip(gain, beats)],
                                  expected_tiou_given_up=[round(float(x / b), 3) if b else None for x, b in zip(loss, beats)],
                                  runner_up_within_1e5=int(ties), at_distance_0=int(exact))))


if __name__ == '__main__':
    main()
