"""GPU: training on the span posterior.  hual_al_span_marginals (the start / end marginals of the posterior given the answered active
points) against the float64 enumeration of its contract (tests/soft_label_ref.py), its edge rows and the memory it must not touch; the
soft-label blend of hual_assemble_batch_soft / hual_assemble_batch_cursor_soft against its numpy float32 restatement, bit for bit; the
epoch loop's step graphs after the banks and the hard labels change under them; whole-model parity at dense soft labels; and the places
it lands: al.update_labels(soft_out=) and al.run_round(soft_labels=).

The bar (from the contract's arithmetic, include/hual_seqpan.h; not tuned):
  y_start, y_end  1e-6 absolute, the project's bar for float32-stored probabilities (the derivation of the expected-tIoU bar):
                  float32 probabilities shared bit for bit with the reference, float64 sums of non-negative terms, one final rounding to
                  float32 of a value <= 1 (6e-8).
Everything about the assembly is exact."""
import copy

import numpy as np
import pytest
import torch

import al_query_ref as Q
import al_synth
import parity_util as pu
import soft_label_ref as S
from test_gpu_al_query import _pads_intact, _round_set, _sentinel, make_set, pad_logits

pytestmark = pytest.mark.gpu

BAR = 1e-6
FILL = 777.0


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def run_marginals(dev, s, e, vlen, tlen, aps, host_tlen=None):
    """one launch into sentinel-filled outputs -> (y_start, y_end, status) numpy, after checking the memory around and beyond them"""
    from hual_amd import lib
    N, ld = s.shape
    aset, keep = make_set(dev, vlen, tlen, aps, ld)
    bufs = [_sentinel((N, ld), torch.float32, dev, FILL), _sentinel((N, ld), torch.float32, dev, FILL), _sentinel((N,), torch.int32, dev, 777)]
    out = tuple(b[0] for b in bufs)
    got = lib.al_span_marginals(aset, s, e, np.asarray(tlen if host_tlen is None else host_tlen), out=out)
    assert all(a is b for a, b in zip(got, out))
    torch.cuda.synchronize()
    for b, fill in zip(bufs, (FILL, FILL, 777)):
        assert _pads_intact(b[1], b[2], fill)
    ys, ye, st = (o.cpu().numpy() for o in out)
    assert not (st == 777).any()
    beyond = np.arange(ld)[None, :] >= np.asarray(tlen)[:, None]
    for y in (ys, ye):
        assert (y[beyond] == FILL).all() and not (y[~beyond] == FILL).any()      # columns [tlen, ld) keep their fill
    return ys, ye, st


def _worst(ys, ye, ref, v, T):
    """max |y - ref| of one live row, after the exact checks: 0 at [v, T)"""
    assert (ys[v:T] == 0).all() and (ye[v:T] == 0).all()
    return max(float(np.abs(ys[:v].astype(np.float64) - ref['y_start']).max()), float(np.abs(ye[:v].astype(np.float64) - ref['y_end']).max()))


# ---------------------------------------------------------------------------------------------------------------- 1. the marginals
@pytest.mark.parametrize('h', Q.HISTORIES)
@pytest.mark.parametrize('T', Q.TS)
def test_marginals_against_the_float64_reference(dev, T, h):
    c = S.case(T)
    ld = T + 7
    s, e = pad_logits(dev, c['s'], ld, 1), pad_logits(dev, c['e'], ld, 2)
    ys, ye, st = run_marginals(dev, s, e, c['vlen'].numpy(), [T] * Q.N_ROWS, c['aps'][h])
    assert (st == 1).all()
    d = 0.0
    for n in range(Q.N_ROWS):
        ref, v = c['mref'][h][n], int(c['v'][n])
        assert ref['status'] == S.LIVE
        d = max(d, _worst(ys[n], ye[n], ref, v, T))
        assert abs(float(ys[n, :v].astype(np.float64).sum()) - 1.0) <= 1e-5 and abs(float(ye[n, :v].astype(np.float64).sum()) - 1.0) <= 1e-5
        for f, is_pos in c['aps'][h][n]:                                # what the answers rule out is exactly 0
            if not is_pos:
                assert ys[n, f] == 0 and ye[n, f] == 0
    print('T=%d ld=%d answers=%d: max |y - ref| = %.3e (bar %.0e)' % (T, ld, h, d, BAR))
    assert d <= BAR


def test_marginals_of_a_mixed_set(dev):
    """rows of 70 and of 256 frames in one set of ld = 300: columns [T, ld) keep the sentinel (run_marginals), [v, T) are 0"""
    ld = 300
    a, b = S.case(70), S.case(256)
    N = 2 * Q.N_ROWS
    s, e = torch.zeros(N, 256), torch.zeros(N, 256)
    s[0::2, :70], e[0::2, :70], s[1::2], e[1::2] = a['s'], a['e'], b['s'], b['e']
    tlen = np.array([70, 256] * Q.N_ROWS)
    vlen, aps, ref = np.zeros(N, dtype=np.int32), [None] * N, [None] * N
    for n in range(Q.N_ROWS):
        for k, (c, h) in enumerate(((a, 3), (b, 6))):
            vlen[2 * n + k], aps[2 * n + k], ref[2 * n + k] = int(c['vlen'][n]), c['aps'][h][n], c['mref'][h][n]
    ys, ye, st = run_marginals(dev, pad_logits(dev, s, ld, 3), pad_logits(dev, e, ld, 4), vlen, tlen, aps)
    assert (st == 1).all()
    d = max(_worst(ys[n], ye[n], ref[n], int(vlen[n]), int(tlen[n])) for n in range(N))
    print('mixed set, ld = 300: max |y - ref| = %.3e (bar %.0e)' % (d, BAR))
    assert d <= BAR


def test_edge_rows_in_one_set(dev):
    from hual_amd import lib
    T, ld = 33, 300
    c = Q.case(T)
    N = 9
    s, e = torch.zeros(N, 257), torch.zeros(N, 257)
    s[:, :T], e[:, :T] = c['s'][0], c['e'][0]
    g = torch.Generator().manual_seed(9)
    s[2], e[2] = torch.randn(257, generator=g), torch.randn(257, generator=g)
    vlen = np.array([20, 0, 257, T, 3, 20, 20, 1, 20], dtype=np.int32)
    tlen = np.array([T, T, 257, T, T, T, T, T, 25], dtype=np.int32)
    aps = [[] for _ in range(N)]
    s[0, 5] = float('nan')                                            # 0: a NaN logit below v: poisoned
    #                                                                   1: v < 1: poisoned;  2: a row of 257 frames: poisoned
    aps[3] = [(5, True), (9, True), (7, False)]                       # 3: a negative inside the positive hull: contradictory
    aps[4] = [(0, False), (2, False), (1, False)]                     # 4: every frame negative: contradictory
    aps[5] = [(4, True), (25, False), (20, True), (-3, False)]        # 5: active points outside [0, v): ignored
    aps[6] = [(4, True)]                                              # 6: row 5 without them
    #                                                                   7: v == 1: the one span;  8: v < T < ld, negatives only
    aps[8] = [(3, False), (12, False), (9, False)]
    e[8, 22] = float('nan')                                           # a NaN logit at t >= v: not read
    sd, ed = pad_logits(dev, s, ld, 5), pad_logits(dev, e, ld, 6)
    ys, ye, st = run_marginals(dev, sd, ed, vlen, tlen, aps, host_tlen=np.minimum(tlen, 256))      # (the host is not told of row 2)
    assert st.tolist() == [0, 0, 0, 0, 0, 1, 1, 1, 1]
    ref = S.set_ref(s, e, vlen, tlen, aps)                            # (row 2: the 256-frame limit is the kernel's, not the definition's)
    assert [x['status'] for n, x in enumerate(ref) if n != 2] == [S.POISONED] * 2 + [S.CONTRADICTORY] * 2 + [S.LIVE] * 4
    for n in range(N):
        Tn = int(tlen[n])
        if st[n] == 0:
            assert not ys[n, :Tn].any() and not ye[n, :Tn].any(), n      # zeros in [0, min(T, ld))
        else:
            assert _worst(ys[n], ye[n], ref[n], ref[n]['v'], Tn) <= BAR, n
    assert (ys[5].view(np.int32) == ys[6].view(np.int32)).all() and (ye[5].view(np.int32) == ye[6].view(np.int32)).all()
    assert ys[5, 5:T].max() == 0 and ye[5, :4].max() == 0             # row 5: the positive at 4 alone counts
    assert ys[7, 0] == 1.0 and ye[7, 0] == 1.0
    for f in (3, 9, 12):
        assert ys[8, f] == 0 and ye[8, f] == 0
    # a collapsed posterior: one-hot rows
    ys, ye, st = run_marginals(dev, sd[:1].nan_to_num(0.0).contiguous(), ed[:1].contiguous(), [20], [T], [[(11, False), (12, True), (13, False)]])
    assert st[0] == 1 and ys[0, 12] == 1.0 and ye[0, 12] == 1.0 and ys[0, :T].sum() == 1.0 and ye[0, :T].sum() == 1.0
    # a row longer than 256 frames the host knows of: the binding refuses the set before the launch
    aset, keep = make_set(dev, [300, 20], [300, 20], [[], []], 300)
    z = torch.zeros(2, 300, device=dev)
    with pytest.raises(lib.HualError, match='256'):
        lib.al_span_marginals(aset, z, z, np.array([300, 20]))


def test_marginals_in_a_captured_graph(dev):
    from hual_amd import lib
    c = S.case(33)
    s, e = pad_logits(dev, c['s'], 33, 1), pad_logits(dev, c['e'], 33, 2)
    aset, keep = make_set(dev, c['vlen'].numpy(), [33] * Q.N_ROWS, c['aps'][3], 33)
    eager = lib.al_span_marginals(aset, s, e, [33] * Q.N_ROWS)
    out = (torch.zeros(Q.N_ROWS, 33, device=dev), torch.zeros(Q.N_ROWS, 33, device=dev), torch.zeros(Q.N_ROWS, dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        lib.al_span_marginals(aset, s, e, [33] * Q.N_ROWS, out=out)
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, out):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------- 2. the assembly
LENS = (1, 2, 7, 33, 64)
WEIGHTS = (0.0, 0.25, 1.0, 0.5, 0.0)


def _five_sample_set(dev):
    from hual_amd.dataset import DeviceDataset
    g = np.random.default_rng(11)
    V = 16
    recs, vis = [], {}
    for i, n in enumerate(LENS):
        vis['v%d' % i] = g.standard_normal((n, V)).astype(np.float32)
        a = int(g.integers(0, n))
        nw = int(g.integers(1, 7))
        recs.append(dict(vid='v%d' % i, w_ids=[int(x) for x in g.integers(1, 99, size=nw)],
                         c_ids=[[int(x) for x in g.integers(1, 30, size=int(g.integers(1, 9)))] for _ in range(nw)],
                         s_ind=a, e_ind=int(g.integers(a, n))))
    b1, b2 = g.random((5, 70), dtype=np.float32), g.random((5, 70), dtype=np.float32)      # wider than the banks: the leading columns are taken
    w = np.array(WEIGHTS, dtype=np.float32)
    b1[w == 0], b2[w == 0] = np.nan, np.nan                           # the rows of the unweighted samples must not be read
    return recs, vis, b1, b2, w


FEEDS = ('video', 'video_seq_len', 'word_ids', 'char_ids', 'y1', 'y2', 'match_labels', 'inner_labels')


def _bits(t):
    a = t.cpu().numpy()
    return a.view(np.int32) if a.dtype == np.float32 else a


def _check_assembled(out, plain, recs, sel, b1, b2, w):
    """`out` against the numpy blend; its unweighted rows, its frames beyond the clips and every other feed against the plain assembly"""
    lens = np.array([LENS[i] for i in sel])
    T = int(lens.max())
    y1, y2, match, inner = S.soft_labels_ref([recs[i]['s_ind'] for i in sel], [recs[i]['e_ind'] for i in sel], lens, T, b1[sel], b2[sel], w[sel])
    assert (_bits(out['y1']) == y1.view(np.int32)).all() and (_bits(out['y2']) == y2.view(np.int32)).all()
    np.testing.assert_array_equal(out['match_labels'].cpu().numpy(), match)
    np.testing.assert_array_equal(out['inner_labels'].cpu().numpy(), inner)
    for k in FEEDS:
        if k not in ('y1', 'y2'):
            assert (_bits(out[k]) == _bits(plain[k])).all(), k
    beyond = np.arange(T)[None, :] >= lens[:, None]
    for k in ('y1', 'y2'):
        o, p = _bits(out[k]), _bits(plain[k])
        assert (o[w[sel] == 0] == p[w[sel] == 0]).all() and (o[beyond] == p[beyond]).all(), k
    assert np.isfinite(out['y1'].cpu().numpy()).all() and np.isfinite(out['y2'].cpu().numpy()).all()
    moved = (_bits(out['y1']) != _bits(plain['y1'])).any(axis=1)
    assert (moved == ((w[sel] != 0) & (lens > 0))).all()               # every weighted row did move


def test_soft_assembly_is_the_numpy_blend_bit_for_bit(dev):
    from hual_amd.dataset import DeviceDataset
    recs, vis, b1, b2, w = _five_sample_set(dev)
    hard = DeviceDataset(recs, vis)                                   # banks never enabled: today's launches
    ds = DeviceDataset(recs, vis)
    assert ds.soft is None and ds.soft_address() == 0
    sels = ([0, 1, 2, 3, 4], [4, 2], [1, 0], [3, 2, 0])
    before = [{k: v.clone() for k, v in ds.assemble(sel, min_chars=4).items()} for sel in sels]
    ds.enable_soft_labels()
    addr = (ds.soft_y1.data_ptr(), ds.soft_y2.data_ptr(), ds.soft_w.data_ptr())
    assert ds.soft_address() == addr[0] and tuple(ds.soft_y1.shape) == (5, 64) and not ds.soft_w.any()
    for sel, want in zip(sels, before):                               # enabled, all weights 0: the plain assembly bit for bit
        got = ds.assemble(sel, min_chars=4)
        for k in FEEDS:
            assert (_bits(got[k]) == _bits(want[k])).all(), k
    ds.set_soft_labels(torch.from_numpy(b1).to(dev), b2, w)          # device and host sources
    assert (ds.soft_y1.data_ptr(), ds.soft_y2.data_ptr(), ds.soft_w.data_ptr()) == addr
    b1c, b2c = b1[:, :64], b2[:, :64]
    for sel in sels:
        sel = np.asarray(sel)
        plain = hard.assemble(sel, min_chars=4)
        _check_assembled(ds.assemble(sel, min_chars=4), plain, recs, sel, b1c, b2c, w)
        # with a carry
        src, dst = torch.arange(6, dtype=torch.int64, device=dev), torch.zeros(6, dtype=torch.int64, device=dev)
        _check_assembled(ds.assemble(sel, min_chars=4, carry=(src, dst)), plain, recs, sel, b1c, b2c, w)
        assert torch.equal(src, dst)
        # through the cursor variant: the batch sits behind two other ids
        B, (T, L, C) = len(sel), ds.batch_shape(sel)
        C = max(C, 4)
        bufs = ds.feed_buffers(B, min_chars=4)
        views = ds.feed_views(B, T, L, C, bufs)
        ids = torch.from_numpy(np.concatenate([[4, 0], sel]).astype(np.int32)).to(dev)
        cursor = torch.tensor([2, 0], dtype=torch.int64, device=dev)
        ds.enqueue_assemble_cursor(views, ids, cursor)
        _check_assembled(views, plain, recs, sel, b1c, b2c, w)
        hv = hard.feed_views(B, T, L, C, hard.feed_buffers(B, min_chars=4))
        hard.enqueue_assemble_cursor(hv, ids, cursor)
        for k in FEEDS:
            assert (_bits(hv[k]) == _bits(plain[k])).all(), k
    # test batches carry no labels, banks or not
    assert 'y1' not in ds.assemble([0, 3], labels=False)
    # clear: back to the plain labels, the banks where they were
    ds.clear_soft_labels()
    got = ds.assemble(sels[0], min_chars=4)
    assert (_bits(got['y1']) == _bits(before[0]['y1'])).all() and ds.soft_y1.data_ptr() == addr[0]
    # the weights are validated on the host
    for bad in ([0, 0, 0, 0, 1.5], [0, -0.1, 0, 0, 0], [0, 0, float('nan'), 0, 0], [0, 0, 0, 0]):
        with pytest.raises(ValueError, match='w must hold'):
            ds.set_soft_labels(b1, b2, np.array(bad, dtype=np.float32))
    with pytest.raises(ValueError, match='y1 / y2'):
        ds.set_soft_labels(b1[:, :40], b2, w)


# ---------------------------------------------------------------------------------------------------------------- 3. the trainer
def test_a_reused_trainer_sees_new_soft_and_hard_labels():
    """the step graphs hold the assembly launch with its pointer arguments: banks enabled after a shape was captured re-capture, and
    new bank values / new hard labels written in place reach a replayed step.  Feeds are compared, not trajectories."""
    from hual_amd import al, lib
    from hual_amd.dataset import DeviceDataset
    from hual_amd.model import SeqPAN
    from hual_amd.train import Trainer
    N, bs, vdim, max_vlen = 8, 4, 64, 24
    recs, vis, data_gt, data_old = al_synth.make_trainset(N, 16, vdim, max_vlen, seed=5)
    cfg = lib.make_cfg(vdim=vdim, max_vlen=max_vlen, num_words=200, num_chars=30)
    wv = np.random.default_rng(1).normal(0, 0.4, size=(198, 300)).astype(np.float32)
    ds = DeviceDataset(recs, vis)
    s0, e0 = al.labels_from_times(data_gt, ds.vlen_h)
    ds.set_labels(s0, e0)
    ind_addr = (ds.s_ind.data_ptr(), ds.e_ind.data_ptr())
    tr = Trainer(SeqPAN(cfg, wv), world=1, use_graph=True)
    order = np.random.default_rng(0).permutation(N).astype(np.int32)
    shapes = len({ds.batch_shape(order[lo:lo + bs]) for lo in range(0, N, bs)})
    g = np.random.default_rng(3)

    def epoch():
        tr.run_epoch(ds, order, bs, lr=1e-4, drop_rate=0.2, min_chars=4)
        torch.cuda.synchronize()
        return dict(tr.stats)

    def banks():
        y = g.random((2, N, max_vlen + 3), dtype=np.float32)
        return y[0] / y[0].sum(1, keepdims=True), y[1] / y[1].sum(1, keepdims=True), g.choice(np.array([0.0, 0.5, 1.0], dtype=np.float32), N)

    def last_feeds_are(s_ind, e_ind, b1, b2, w):
        sel = order[N - bs:]
        lens = ds.vlen_h[sel]
        y1, y2, match, _ = S.soft_labels_ref(s_ind[sel], e_ind[sel], lens, int(lens.max()), b1[sel], b2[sel], w[sel])
        assert (_bits(tr.y1) == y1.view(np.int32)).all() and (_bits(tr.y2) == y2.view(np.int32)).all()
        np.testing.assert_array_equal(tr.match.cpu().numpy(), match)
    zero = np.zeros((N, max_vlen), dtype=np.float32), np.zeros((N, max_vlen), dtype=np.float32), np.zeros(N, dtype=np.float32)
    epoch()
    st = epoch()                                                      # banks not enabled: eager, then captured
    assert (st['eager'], st['captured']) == (shapes, shapes)
    last_feeds_are(s0, e0, *zero)
    b1, b2, w = banks()
    w[order[-1]] = 0.5
    ds.set_soft_labels(b1, b2, w)                                     # enabling the banks: another key, never the old launch
    epoch()
    last_feeds_are(s0, e0, b1, b2, w)
    st = epoch()
    assert (st['eager'], st['captured']) == (2 * shapes, 2 * shapes)
    last_feeds_are(s0, e0, b1, b2, w)
    # other values and other indices, in place; the same trainer replays
    b1, b2, w = banks()
    w[order[-1]] = 1.0
    bank_addr = ds.soft_address()
    ds.set_soft_labels(torch.from_numpy(b1).cuda(), torch.from_numpy(b2).cuda(), w)
    s1 = np.array([int(g.integers(0, n)) for n in ds.vlen_h], dtype=np.int32)
    e1 = np.array([int(g.integers(a, n)) for a, n in zip(s1, ds.vlen_h)], dtype=np.int32)
    assert (s1 != s0).any()
    ds.set_labels(s1, e1)
    assert (ds.s_ind.data_ptr(), ds.e_ind.data_ptr()) == ind_addr and ds.soft_address() == bank_addr
    replayed = st['replayed']
    st = epoch()
    assert st['replayed'] == replayed + N // bs and st['captured'] == 2 * shapes
    last_feeds_are(s1, e1, b1, b2, w)


# ---------------------------------------------------------------------------------------------------------------- 4. the model
def test_whole_model_parity_at_dense_soft_labels():
    """y1 / y2 dense rows that sum to 1 over each clip: every tap, loss and gradient passes the usual gates, spans exact"""
    cfg, p, wv, b, labels = pu.make_case(B=3, T=20, L=6, C=5, seed=3, max_vlen=32)
    g = np.random.default_rng(17)
    lens = b['lens'].numpy()
    dense = []
    for _ in range(2):
        y = g.random((3, 20)).astype(np.float32) * (np.arange(20)[None, :] < lens[:, None])
        dense.append(torch.tensor((y / y.sum(1, keepdims=True)).astype(np.float32)))
    assert all(int((d > 0).sum()) == int(lens.sum()) for d in dense)
    rows, idx_equal, o, h, m = pu.compare(cfg, p, wv, b, (dense[0], dense[1], labels[2], labels[3]), drop_rate=0.2)
    pu.assert_rows(rows, ('tap', 'out', 'loss', 'grad', 'gl2'), pu.TOL)
    assert idx_equal
    hard, _, _, _, _ = pu.compare(cfg, p, wv, b, labels, drop_rate=0.2, with_grads=False)
    loc = {r[1]: r[3] for r in rows if r[0] == 'loss'}['loc_loss'], {r[1]: r[3] for r in hard if r[0] == 'loss'}['loc_loss']
    assert abs(loc[0] - loc[1]) > 1e-2, loc                           # the dense rows are another loss than the hard labels'


# ---------------------------------------------------------------------------------------------------------------- 5. update and round
def _aps_of(data):
    return [[(f, True) for f in r[4]['pos_idx']] + [(f, False) for f in r[4]['neg_idx']] for r in data]


def test_update_labels_hands_out_the_marginals(dev):
    from hual_amd import al
    Sx = _round_set()
    N, prop, coff = Sx['N'], Sx['prop'], al.get_coff('charades', 1)
    # earlier rounds' answers, made by hand and truthful: every third sample was told its ground-truth centre frame is inside the span;
    # sample 1 carries a point beyond its clip, which answers nothing
    vl = [int(p['v_len']) for p in prop]
    new1 = copy.deepcopy(Sx['data_old'])
    early = np.arange(N) % 3 == 0
    for i, r in enumerate(new1):
        a, e = (al._round_half_even_index(t, Sx['data_gt'][i][1], vl[i]) for t in Sx['data_gt'][i][2])
        r.append({'pos_idx': [(a + e) // 2] if early[i] else [], 'neg_idx': [1000] if i == 1 else []})
    for kw in (dict(), dict(observe_by='info_gain', renew_by='posterior')):
        new0, d0 = al.update_labels(copy.deepcopy(new1), Sx['data_gt'], prop, al.get_coff('charades', 2), return_debug=True, **kw)
        soft = {}
        new2, d2 = al.update_labels(copy.deepcopy(new1), Sx['data_gt'], prop, al.get_coff('charades', 2), return_debug=True, soft_out=soft, **kw)
        assert new2 == new0 and sorted(d2) == sorted(d0)              # nothing else about the call changes
        for k in d0:
            if k != 'updater':
                np.testing.assert_array_equal(d2[k], d0[k], err_msg=k)
        assert sorted(soft) == ['answered', 'live', 'y1', 'y2']
        up = d2['updater']
        aps = _aps_of(new2)                                           # the post-answer active points
        ref = S.set_ref(up._s0.cpu(), up._e0.cpu(), up.vlen_h, up.tlen_h, aps)
        y1, y2 = soft['y1'].cpu().numpy(), soft['y2'].cpu().numpy()
        assert y1.shape == y2.shape == (N, up.ld) and soft['y1'].is_cuda and soft['live'].dtype == bool and soft['answered'].dtype == bool
        d = 0.0
        for n in range(N):
            assert soft['live'][n] == (ref[n]['status'] == S.LIVE)
            assert soft['answered'][n] == any(0 <= f < int(up.vlen_h[n]) for f, _ in aps[n])
            if soft['live'][n]:
                d = max(d, _worst(y1[n], y2[n], ref[n], ref[n]['v'], int(up.tlen_h[n])))
        print('update_labels(soft_out=, %s): max |bank - ref| = %.3e (bar %.0e)' % (kw, d, BAR))
        assert d <= BAR
        insel = np.zeros(N, dtype=bool)
        insel[d2['order'][:(N + 1) // 2]] = True
        assert soft['live'].all()
        np.testing.assert_array_equal(soft['answered'], insel | early)   # this round's answers and the earlier rounds' on unselected samples
        print('answered: %d of %d, %d of them unselected' % (soft['answered'].sum(), N, (early & ~insel).sum()))
        assert not soft['answered'][1] or insel[1]


def test_a_round_on_soft_labels():
    from hual_amd import al, lib
    from hual_amd.dataset import DeviceDataset
    from hual_amd.model import SeqPAN
    N, vdim, max_vlen = 24, 64, 24
    recs, vis, data_gt, data_old = al_synth.make_trainset(N, 8, vdim, max_vlen, seed=3)
    cfg = lib.make_cfg(vdim=vdim, max_vlen=max_vlen, num_words=200, num_chars=30)
    wv = np.random.default_rng(1).normal(0, 0.4, size=(198, 300)).astype(np.float32)
    model = SeqPAN(cfg, wv)
    ds = DeviceDataset(recs, vis)
    s0, e0 = al.labels_from_times(data_old, ds.vlen_h)
    ds.set_labels(s0, e0)
    for r, a, b in zip(recs, s0, e0):
        r['s_ind'], r['e_ind'] = int(a), int(b)

    def batches():
        for lo in range(0, N, 8):
            sel = np.arange(lo, min(N, lo + 8))
            f = ds.assemble(sel, labels=False, min_chars=4)
            yield [recs[i] for i in sel], f['video'], f['video_seq_len'], f['word_ids'], f['char_ids']
    prop, _ = al.infer_trainset(model, batches(), mc_dropout=0.5)
    soft = {}
    al.update_labels(copy.deepcopy(data_old), data_gt, prop, al.get_coff('charades', 1), soft_out=soft)
    want = soft['live'] & soft['answered']
    assert 0 < want.sum() < N
    new1, prop1, m1 = al.run_round(model, ds, copy.deepcopy(data_old), data_gt, prop, 'charades', 1, epochs=1, batch_size=8, lr=1e-3,
                                   drop_rate=0.2, soft_labels=0.5)
    assert len(prop1) == N and m1['train_steps'] == 3 and 0.0 <= m1['miou'] <= 100.0
    assert m1['soft_rows'] == int(want.sum())
    w = ds.soft_w.cpu().numpy()
    assert (w[want] == 0.5).all() and (w[~want] == 0.0).all()
    assert torch.equal(ds.soft_y1, soft['y1'][:, :ds.soft_y1.shape[1]]) and torch.equal(ds.soft_y2, soft['y2'][:, :ds.soft_y2.shape[1]])
    assert torch.isfinite(model.params).all()
    # the default: no weights left behind, no metric
    new2, prop2, m2 = al.run_round(model, ds, copy.deepcopy(new1), data_gt, prop1, 'charades', 2, epochs=1, batch_size=8, lr=1e-3,
                                   drop_rate=0.2)
    assert 'soft_rows' not in m2 and not ds.soft_w.any()
