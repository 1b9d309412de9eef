"""GPU: hual_span_topk (top-k spans after greedy temporal NMS) against the CPU reference of its contract (tests/span_topk_ref.py), its
first slot against hual_span_argmax, graph capture, and Runner.evaluate's R@k on the learnable task of test_gpu_runner.py."""
import numpy as np
import pytest
import torch

import span_topk_ref as R
from span_clip_util import _task, _videos

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def _topk(s, e, vl, k, max_len=0, nms_iou=1.0):
    from hual_amd import lib
    st, en, sc = lib.span_topk(s, e, vl, k, max_len=max_len, nms_iou=nms_iou)
    return st.cpu().numpy(), en.cpu().numpy(), sc.cpu().numpy()


def _assert_same(got, want, what):
    gs, ge, gc = got
    ws, we, wc = want
    bad = np.nonzero((gs != ws).any(1) | (ge != we).any(1) | (gc.view(np.int32) != wc.view(np.int32)).any(1))[0]
    assert len(bad) == 0, (what, len(bad), int(bad[0]), gs[bad[0]], ws[bad[0]], ge[bad[0]], we[bad[0]], gc[bad[0]], wc[bad[0]])


@pytest.mark.parametrize('B', [1, 7, 64])
@pytest.mark.parametrize('T', [1, 2, 63, 64, 65, 128, 256])
def test_topk_matches_the_reference(dev, B, T):
    g = torch.Generator().manual_seed(1000 * B + T)
    s = torch.randn(B, T, generator=g) * 3
    e = torch.randn(B, T, generator=g) * 3
    vl = torch.randint(1, T + 1, (B,), generator=g, dtype=torch.int32)
    vl[0] = T
    if B > 1:
        vl[1] = 1
    if B > 2:
        s[2, :] = 0.5                                             # a plateau: every candidate ties in score
    if B > 3:
        e[3, : T // 2] = e[3, 0]
    sd, ed, vd = s.to(dev), e.to(dev), vl.to(dev)
    for k in (1, 5, 16):
        for nms_iou in (1.0, 0.5, 0.3):
            for max_len in (0, 8):
                got = _topk(sd, ed, vd, k, max_len, nms_iou)
                _assert_same(got, R.span_topk_ref(s, e, vl, k, max_len=max_len, nms_iou=nms_iou), (k, nms_iou, max_len))
                n = np.minimum(vl.numpy().astype(np.int64), T)
                ok = got[0] >= 0
                assert (got[1][ok] < n[:, None].repeat(k, 1)[ok]).all() and (got[0][ok] <= got[1][ok]).all()


def _argmax_hip(dev, s, e, m):
    from hual_amd import lib
    B, T = s.shape
    si = torch.empty(B, dtype=torch.int64, device=dev)
    ei = torch.empty(B, dtype=torch.int64, device=dev)
    lib.check(lib.load().hual_span_argmax(lib.ptr(s), lib.ptr(e), lib.ptr(m), lib.ptr(si), lib.ptr(ei), B, T, lib.stream_ptr()))
    return si.cpu().numpy(), ei.cpu().numpy()


def _top1_vs_argmax(dev, s, e, lens):
    """rows compared, rows where slot 0 and hual_span_argmax agree (the reference's non-product ties excluded)"""
    B, T = s.shape
    m = (torch.arange(T)[None, :] < lens[:, None]).float()
    sd, ed = s.to(dev), e.to(dev)
    si, ei = _argmax_hip(dev, sd, ed, m.to(dev))
    st, en, _ = _topk(sd, ed, lens.to(torch.int32).to(dev), 1, nms_iou=0.5)
    ps, pe, v, _ = R.probabilities(s, e, lens)
    keep = np.array([not R.non_product_tie(ps[b], pe[b], int(v[b])) for b in range(B)])
    same = (st[:, 0] == si) & (en[:, 0] == ei)
    assert same[keep].all(), np.nonzero(keep & ~same)[0]
    return int(keep.sum())


@pytest.mark.parametrize('B,T', [(4, 7), (16, 64), (3, 256), (64, 128)])
def test_top1_is_span_argmax(dev, B, T):
    """the random inputs of test_gpu_kernels.py::test_span_argmax_bit_exact, with its plateau (s[0, :3] equal)"""
    g = torch.Generator().manual_seed(B + T)
    s = torch.randn(B, T, generator=g) * 3
    e = torch.randn(B, T, generator=g) * 3
    s[0, :3] = s[0, 0]
    lens = torch.randint(1, T + 1, (B,), generator=g)
    lens[0] = T
    assert _top1_vs_argmax(dev, s, e, lens) == B                  # no non-product tie on random logits


def test_top1_is_span_argmax_on_near_ties(dev):
    """the near-tie input of test_gpu_kernels.py::test_span_argmax_near_ties_bit_exact: logits a few ulps apart, so different
    products can round to the same float; rows where that decides the maximum are counted out, and there must be few"""
    B, T = 512, 96
    g = torch.Generator().manual_seed(2024)
    base_s = torch.randn(B, 1, generator=g) * 2
    base_e = torch.randn(B, 1, generator=g) * 2
    s = base_s + torch.randint(-3, 4, (B, T), generator=g).float() * 2.0 ** -21
    e = base_e + torch.randint(-3, 4, (B, T), generator=g).float() * 2.0 ** -21
    s[B // 2:, 10:20] = s[B // 2:, 10:11]
    s[B // 2:, 60:70] = s[B // 2:, 10:11]
    e[B // 2:, 30:40] = e[B // 2:, 30:31]
    e[B // 2:, 80:90] = e[B // 2:, 30:31]
    lens = torch.randint(T // 2, T + 1, (B,), generator=g)
    assert _top1_vs_argmax(dev, s, e, lens) >= 0.9 * B


def test_padding_nan_rows_and_lengths(dev):
    T, k = 6, 16
    s = torch.randn(6, T, generator=torch.Generator().manual_seed(5))
    e = torch.randn(6, T, generator=torch.Generator().manual_seed(6))
    s[1, 2] = float('nan')                                        # inside the clip: the whole row is -1
    e[2, 4] = float('nan')                                        # beyond vlen = 3: not read
    s[2, 5] = float('inf')
    vl = torch.tensor([6, 6, 3, 0, 99, -4], dtype=torch.int32)    # 0 / negative: empty clip; 99: read as T
    st, en, sc = _topk(s.to(dev), e.to(dev), vl.to(dev), k, nms_iou=1.0)
    _assert_same((st, en, sc), R.span_topk_ref(s, e, vl, k, nms_iou=1.0), 'padding')
    assert (st[0] >= 0).all() and (st[4] >= 0).all()                 # 21 candidates for 16 slots
    for b in (1, 3, 5):
        assert (st[b] == -1).all() and (en[b] == -1).all() and (sc[b] == -1.0).all()
    assert (st[2, :6] >= 0).all() and (st[2, 6:] == -1).all() and (sc[2, 6:] == -1.0).all()     # 6 candidates for vlen 3
    st, en, sc = _topk(s.to(dev), e.to(dev), vl.to(dev), k, nms_iou=0.3)   # NMS leaves fewer than k
    _assert_same((st, en, sc), R.span_topk_ref(s, e, vl, k, nms_iou=0.3), 'nms padding')
    assert (st[0] == -1).any()


def test_topk_in_a_captured_graph(dev):
    from hual_amd import lib
    B, T, k = 32, 128, 5
    g = torch.Generator().manual_seed(7)
    s = (torch.randn(B, T, generator=g) * 3).to(dev)
    e = (torch.randn(B, T, generator=g) * 3).to(dev)
    vl = torch.randint(1, T + 1, (B,), generator=g, dtype=torch.int32).to(dev)
    out = (torch.empty(B, k, dtype=torch.int64, device=dev), torch.empty(B, k, dtype=torch.int64, device=dev),
           torch.empty(B, k, dtype=torch.float32, device=dev))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        lib.span_topk(s, e, vl, k, nms_iou=0.5, out=out)           # (loads the library and warms up outside the capture)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        lib.span_topk(s, e, vl, k, nms_iou=0.5, out=out)
    for seed in (8, 9):
        g2 = torch.Generator().manual_seed(seed)
        s.copy_(torch.randn(B, T, generator=g2) * 3)
        e.copy_(torch.randn(B, T, generator=g2) * 3)
        for o in out:
            o.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        want = _topk(s, e, vl, k, nms_iou=0.5)
        _assert_same(tuple(o.cpu().numpy() for o in out), want, 'graph replay')


# ------------------------------------------------------------------ whole model: the learnable task of test_gpu_runner.py
def test_runner_evaluate_recall_at_k(tmp_path):
    from hual_amd import data
    from hual_amd.runner import Runner
    vdim = 64
    vis = _videos(24, vdim, 0)
    train = _task(192, vis, 1)
    test = _task(64, vis, 2)
    cfg = dict(task='synth', train=dict(batch_size=32, droprate=0.1, lr=2e-3, epochs=4, clip_norm=1.0),
               model=dict(vdim=vdim, dim=128, num_heads=8, word_dim=300, char_dim=50, max_vlen=32, attn_layer=2),
               loss=dict(match_lambda=1.0, tau=0.3, no_gumbel=True), num_chars=10)
    wv = np.random.default_rng(0).normal(0, 0.4, size=(40, 300)).astype(np.float32)
    lines = []

    class L:
        def info(self, s):
            lines.append(str(s))
    r = Runner(cfg, wv, train, test, vis, ckpt_dir=str(tmp_path / 'ckpt'), logger=L())
    for ep in range(4):
        r.train_epoch(2e-3 * (1.0 - ep / 4))
    t = r.test_epoch()
    res, props = r.evaluate(k=5, nms_iou=0.5, return_proposals=True)
    assert sorted(res) == sorted(['R1@0.3', 'R1@0.5', 'R1@0.7', 'R5@0.3', 'R5@0.5', 'R5@0.7', 'mIoU'])
    assert (res['R1@0.3'], res['R1@0.5'], res['R1@0.7'], res['mIoU']) == t
    for th in ('0.3', '0.5', '0.7'):
        assert res['R5@' + th] >= res['R1@' + th]
    assert any(l.startswith('EVAL') for l in lines)
    assert r.evaluate(k=1, nms_iou=1.0) == {'R1@0.3': t[0], 'R1@0.5': t[1], 'R1@0.7': t[2], 'mIoU': t[3]}
    # per clip: the reference of the contract on the logits of the same forward, converted to seconds like index_to_time
    ds = r.test_set
    assert len(props) == len(ds)
    for lo in range(0, len(ds), r.batch_size):
        sel = np.arange(lo, min(len(ds), lo + r.batch_size))
        f = ds.assemble(sel, labels=False, min_chars=4)
        o = r.model.forward(f['video'], f['video_seq_len'], f['word_ids'], f['char_ids'], drop_rate=0.0)
        st, en, sc = R.span_topk_ref(o['start_logits'].cpu(), o['end_logits'].cpu(), f['video_seq_len'].cpu(), 5, nms_iou=0.5)
        for row, i in enumerate(sel):
            rec = ds.records[i]
            want = [tuple(float(x) for x in data.index_to_time((a, b), rec['v_len'], rec['duration'])) + (float(c),)
                    for a, b, c in zip(st[row], en[row], sc[row]) if a >= 0]
            assert props[i] == want, (i, props[i], want)
            assert len(want) == 5                                   # 20+ frames leave more than five spans after NMS at 0.5
