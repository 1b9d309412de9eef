"""GPU: the three per-clip span launches (hual_span_topk, hual_span_expected_iou, hual_span_hit_prob) put every clip of one batch in the
same class - dead or live.  They open a clip through one definition (csrc/spanclip.h); the per-clip counterpart of
tests/test_gpu_span_rows.py.  Every comparison is exact."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_all_launches_classify_the_edge_clips_alike():
    from hual_amd import lib
    dev = torch.device('cuda:0')
    T, B, k, nan, inf = 33, 8, 3, float('nan'), float('inf')
    g = torch.Generator().manual_seed(11)
    s, e = torch.randn(B, T, generator=g) * 2, torch.randn(B, T, generator=g) * 2
    vlen = [20, 0, 20, 20, 20, 40, 1, 20]
    s[0, 5] = nan                                                     # 0: a NaN logit below v;  1: v < 1
    e[2, 3] = inf                                                     # 2: an infinite logit: the probabilities are NaN, Z with them
    s[3], e[3] = 0.0, 0.0                                             # 3: the start certainly at 10, the end certainly at 2: every
    s[3, 10], e[3, 2] = 2000.0, 2000.0                                #    product of the triangle is exactly 0 (exp(-2000) == 0), Z = 0
    s[4, 25] = nan                                                    # 4: a NaN logit at t >= v: not read;  5: vlen > T reads as T
    v = [min(x, T) for x in vlen]                                     # 6: v == 1, the one span (0, 0);  7: plain
    dead, live = (0, 1, 2, 3), (4, 5, 6, 7)
    st = torch.tensor([[0, 0, -1]] * B, dtype=torch.int64, device=dev)      # hand-made slots, so that a dead clip still offers valid ones
    en = torch.tensor([[0, max(x - 1, 0), -1] for x in v], dtype=torch.int64, device=dev)
    sd, ed, vd = s.to(dev), e.to(dev), torch.tensor(vlen, dtype=torch.int32, device=dev)
    ts, te, tc = (x.cpu() for x in lib.span_topk(sd, ed, vd, k))
    ei, ent = (x.cpu() for x in lib.span_expected_iou(sd, ed, vd, st, en))
    hp, best = lib.span_hit_prob(sd, ed, vd, starts=st, ends=en, best=True)
    hp, (bs, be, bp) = hp.cpu(), (x.cpu() for x in best)
    for b in dead:
        assert (ei[b] == -1).all() and ent[b] == -1 and (hp[b] == -1).all(), b
        assert (bs[b] == -1).all() and (be[b] == -1).all() and (bp[b] == -1).all(), b
        if b != 3:                                                    # (hual_span_topk has no Z rule: spans of score 0 on row 3)
            assert (ts[b] == -1).all() and (te[b] == -1).all() and (tc[b] == -1.0).all(), b
    for b in live:
        assert 0 <= ts[b, 0] <= te[b, 0] < v[b], b
        assert (ei[b, :2] >= 0).all() and (ei[b, :2] <= 1).all() and ei[b, 2] == -1, b
        assert (hp[b, :2] >= 0).all() and (hp[b, :2] <= 1).all() and (hp[b, 2] == -1).all(), b
        assert ent[b] >= 0 and (0 <= bs[b]).all() and (bs[b] <= be[b]).all() and (be[b] < v[b]).all(), b
    assert ent[6] == 0 and (bs[6] == 0).all() and (be[6] == 0).all()
