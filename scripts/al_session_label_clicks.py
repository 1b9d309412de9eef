#!/usr/bin/env python3
"""How many questions the stop rule on label reliability saves, and how close its decisions come to their thresholds (CPU, the float64
reference of tests/al_session_label_ref.py, no GPU): on the seeded rows of tests/al_query_ref.case(T) - 16 rows per T, sessions of up
to Q = 6 questions from the start lists with no and with three answers, the rule "stop once the minimum-Bayes-risk label's hit
probability at the threshold is at least p" in front of the budget - per setting
  stopped reliable / at budget, and the questions asked of 16 Q, with the rule and without it;
  near:    the live passes whose hit probability lies within 1e-3 of p;
  margin:  the smallest distance between a label's expected tIoU and its runner-up's.
Random logits, unrelated to the ground truth: what the rule saves on a trained model is not known.

    python scripts/al_session_label_clicks.py [--t 33 70 2] [--q 6] [--all-rules]
Prints one JSON line per setting."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import al_query_ref as Q  # noqa: E402
import al_session_label_ref as SL  # noqa: E402
import al_session_ref as S  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--t', type=int, nargs='+', default=[33, 70, 2])
    ap.add_argument('--q', type=int, default=6)
    ap.add_argument('--all-rules', action='store_true', help='every rule of al_session_label_ref.RULES and the noisy settings, not only 0.9 at 7/10')
    a = ap.parse_args()
    rules = SL.RULES if a.all_rules else SL.RULES[:1]
    settings = SL.SETTINGS if a.all_rules else tuple(s for s in SL.SETTINGS if s[1] == 0.0)
    for T in a.t:
        for start, eps, flipped in settings:
            for stop_hit, stop_m in rules:
                with_rule = SL.sessions(T, start, eps, flipped, a.q, stop_hit, stop_m)
                without = S.sessions(T, start, eps, flipped, a.q)
                live = [p for r in with_rule for p in r['passes'] if p['post']['status'] == Q.LIVE]
                print(json.dumps(dict(
                    T=T, start_answers=start, eps=eps, flipped=flipped, rule='%.2f at %d/%d' % (stop_hit, *SL.THR[stop_m]), slots=Q.N_ROWS * a.q,
                    stopped_reliable=int(sum(r['stop_reason'] == SL.RELIABLE for r in with_rule)),
                    stopped_at_budget=int(sum(r['stop_reason'] == S.BUDGET for r in with_rule)),
                    stopped_otherwise=int(sum(r['stop_reason'] not in (SL.RELIABLE, S.BUDGET) for r in with_rule)),
                    questions_asked=int(sum(r['n_asked'] for r in with_rule)), questions_asked_without_the_rule=int(sum(r['n_asked'] for r in without)),
                    live_passes=len(live), near=int(sum(abs(p['hit'][stop_m] - stop_hit) <= SL.NEAR_HIT for p in live)),
                    smallest_label_margin=float(min([p['label']['margin'] for p in live], default=np.inf)))))


if __name__ == '__main__':
    main()
