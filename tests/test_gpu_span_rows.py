"""GPU: the four span-posterior launches (hual_al_query, hual_al_mbr_label, hual_al_label_gain, hual_al_span_marginals) put every row
of one set in the same class - poisoned, contradictory or live.  They open a row through one definition (csrc/spanpost.h); this pins the
agreement on the edge rows of tests/test_gpu_soft_labels.py::test_edge_rows_in_one_set.  Every comparison is exact."""
import numpy as np
import pytest
import torch

import al_query_ref as Q
from test_gpu_al_query import make_set, pad_logits

pytestmark = pytest.mark.gpu

POISONED, CONTRADICTORY, LIVE = 'poisoned', 'contradictory', 'live'


def test_all_launches_classify_the_edge_rows_alike():
    from hual_amd import lib
    dev = torch.device('cuda:0')
    T, ld, N = 33, 300, 9
    c = Q.case(T)
    s, e = torch.zeros(N, 257), torch.zeros(N, 257)
    s[:, :T], e[:, :T] = c['s'][0], c['e'][0]
    g = torch.Generator().manual_seed(9)
    s[2], e[2] = torch.randn(257, generator=g), torch.randn(257, generator=g)
    vlen = np.array([20, 0, 257, T, 3, 20, 20, 1, 20], dtype=np.int32)
    tlen = np.array([T, T, 257, T, T, T, T, T, 25], dtype=np.int32)      # (row 2: 257 frames, which the host is not told of)
    aps = [[] for _ in range(N)]
    s[0, 5] = float('nan')                                            # 0: a NaN logit below v;  1: v < 1;  2: a row of 257 frames
    aps[3] = [(5, True), (9, True), (7, False)]                       # 3: a negative inside the positive hull
    aps[4] = [(0, False), (2, False), (1, False)]                     # 4: every frame negative
    aps[5] = [(4, True), (25, False), (20, True), (-3, False)]        # 5: active points outside [0, v): ignored
    aps[6] = [(4, True)]                                              # 6: row 5 without them;  7: v == 1: the one span
    aps[8] = [(3, False), (12, False), (9, False)]                    # 8: v < T < ld, negatives only
    e[8, 22] = float('nan')                                           # a NaN logit at t >= v: not read
    want = [POISONED] * 3 + [CONTRADICTORY] * 2 + [LIVE] * 4
    sd, ed = pad_logits(dev, s, ld, 5), pad_logits(dev, e, ld, 6)
    aset, keep = make_set(dev, vlen, tlen, aps, ld)
    host_tlen = np.minimum(tlen, 256)
    agree = lib.al_query(aset, sd, ed, host_tlen, frames=False)[5]
    conf = lib.al_mbr_label(aset, sd, ed, host_tlen)[1]
    value = lib.al_label_gain(aset, sd, ed, host_tlen, frames=False)[3]
    status = lib.al_span_marginals(aset, sd, ed, host_tlen)[2]
    torch.cuda.synchronize()
    agree, conf, value, status = (x.cpu().numpy() for x in (agree, conf, value, status))
    for n in range(N):
        if want[n] == LIVE:
            assert 0 < agree[n] <= 1 and 0 <= conf[n] <= 1 and 0 <= value[n] <= 1 and status[n] == 1, n
            assert value[n:n + 1].view(np.int32) == conf[n:n + 1].view(np.int32), n
        else:
            assert agree[n] == (-1 if want[n] == POISONED else 0) and conf[n] == -1 and value[n] == -1 and status[n] == 0, n
