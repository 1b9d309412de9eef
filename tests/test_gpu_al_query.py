"""GPU: hual_al_query (span posterior given the answered active points, the frame of most expected information gain) against the
float64 brute-force reference of its contract (tests/al_query_ref.py), its edge rows, the memory it must not touch, its agreement with
hual_span_expected_iou and hual_span_argmax, graph capture, and the three places it lands: LabelUpdater.query,
al.update_labels(observe_by='info_gain') and al.run_round(observe_by=).

The bars (from the contract's arithmetic, include/hual_seqpan.h; not tuned):
  incl, agree   1e-6 absolute: the derivation of the expected-tIoU bar - the float32 roundings of p_s and p_e (2^-24 relative
                each, carried through sums of non-negative terms), float64 sums and one final rounding to float32 of a value <= 1: under
                3e-7; the bar is about three times that.
  gain          5e-5 bits: a 1e-6 error of q through h2's slope log2((1 - q) / q) <= 20 bits per unit wherever h2(q) exceeds the bar
                itself, plus the 2e-5 float32 bar of h2_bits (tests/test_gpu_mc_info.py).
  post_entropy  5e-5 bits: the span-entropy bar of hual_span_expected_iou (tests/test_gpu_span_conf.py).
query_point is the first argmax of the kernel's own gain row, exactly; against the reference it has to be a frame whose reference gain
is within 1e-4 bits (twice the bar) of the reference's maximum - plateaus of the gain are common on spiky distributions."""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch

import al_query_ref as Q
import al_synth
import span_topk_ref as R
from span_clip_util import _pads_intact, _sentinel

pytestmark = pytest.mark.gpu

INCL_BAR, AGREE_BAR, GAIN_BAR, ENT_BAR = 1e-6, 1e-6, 5e-5, 5e-5
FILL = 777.0


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def make_set(dev, vlen, tlen, aps, ld):
    """a hual_al_set over device tensors (kept alive beside it): (set, tensors)"""
    from hual_amd import lib
    N = len(vlen)
    off = np.zeros(N + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(a) for a in aps])
    idx = np.array([f for a in aps for f, _ in a] + [0], dtype=np.int32)
    pos = np.array([1 if p else 0 for a in aps for _, p in a] + [0], dtype=np.int8)
    keep = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (np.asarray(vlen, dtype=np.int32), np.asarray(tlen, dtype=np.int32),
                                                                        off, idx, pos)]
    return lib.hual_al_set(N, ld, *[lib._addr(t) for t in keep]), keep


def pad_logits(dev, x, ld, seed):
    """[N, T] -> device [N, ld]; the columns beyond T hold finite noise the kernel must not read"""
    N, T = x.shape
    out = torch.randn(N, ld, generator=torch.Generator().manual_seed(seed)) * 50
    out[:, :T] = x
    return out.contiguous().to(dev)


def run_query(dev, s, e, vlen, tlen, aps, frames=True):
    """one launch into sentinel-filled outputs -> dict of numpy arrays, after checking the memory around and beyond them"""
    from hual_amd import lib
    N, ld = s.shape
    aset, keep = make_set(dev, vlen, tlen, aps, ld)
    bufs = [_sentinel((N, ld), torch.float32, dev, FILL) if frames else None, _sentinel((N, ld), torch.float32, dev, FILL) if frames else None,
            _sentinel((N,), torch.int32, dev, 777), _sentinel((N,), torch.float32, dev, FILL), _sentinel((N,), torch.float32, dev, FILL),
            _sentinel((N,), torch.float32, dev, FILL)]
    out = tuple(b[0] if b is not None else None for b in bufs)
    got = lib.al_query(aset, s, e, np.asarray(tlen), frames=frames, out=out)
    assert all(a is b for a, b in zip(got, out))
    torch.cuda.synchronize()
    for b, fill in zip(bufs, (FILL, FILL, 777, FILL, FILL, FILL)):
        if b is not None:
            assert _pads_intact(b[1], b[2], fill)
    names = ('incl', 'gain', 'query_point', 'query_gain', 'post_entropy', 'agree')
    r = {k: (o.cpu().numpy() if o is not None else None) for k, o in zip(names, out)}
    for k in names[2:]:
        assert not (r[k] == 777).any(), k                             # every [N] slot was written
    if frames:
        beyond = np.arange(ld)[None, :] >= np.asarray(tlen)[:, None]
        for k in ('incl', 'gain'):
            assert (r[k][beyond] == FILL).all() and not (r[k][~beyond] == FILL).any(), k      # columns [tlen, ld) keep their fill
    return r


_GOT = {}


def got(dev, T, extra, h):
    """the device results of the shared case (al_query_ref.case) of length T with ld = T + extra after h answers: computed once"""
    if (T, extra, h) not in _GOT:
        c = Q.case(T)
        ld = T + extra
        s, e = pad_logits(dev, c['s'], ld, 1), pad_logits(dev, c['e'], ld, 2)
        _GOT[(T, extra, h)] = (run_query(dev, s, e, c['vlen'].numpy(), [T] * Q.N_ROWS, c['aps'][h]), s, e)
    return _GOT[(T, extra, h)]


# ---------------------------------------------------------------------------------------------------------------- 1. values
@pytest.mark.parametrize('h', Q.HISTORIES)
@pytest.mark.parametrize('extra', [0, 7])
@pytest.mark.parametrize('T', Q.TS)
def test_values_against_the_float64_reference(dev, T, extra, h):
    c = Q.case(T)
    r, _, _ = got(dev, T, extra, h)
    d = dict(incl=0.0, gain=0.0, ent=0.0, agree=0.0, qp=0.0)
    for n in range(Q.N_ROWS):
        ref, v = c['ref'][h][n], int(c['v'][n])
        assert ref['status'] == Q.LIVE
        assert (r['incl'][n, v:T] == 0).all() and (r['gain'][n, v:T] == 0).all()      # 0 at t >= v
        q, g = r['incl'][n, :v], r['gain'][n, :v]
        assert q.min() >= 0.0 and q.max() <= 1.0
        d['incl'] = max(d['incl'], float(np.abs(q.astype(np.float64) - ref['incl']).max()))
        d['gain'] = max(d['gain'], float(np.abs(g.astype(np.float64) - ref['gain']).max()))
        d['ent'] = max(d['ent'], abs(float(r['post_entropy'][n]) - ref['post_entropy']))
        d['agree'] = max(d['agree'], abs(float(r['agree'][n]) - ref['agree']))
        # the query: the first maximal frame of the kernel's own gain row, exactly - and a maximal frame of the reference up to twice the bar
        qp = int(r['query_point'][n])
        assert qp == int(np.argmax(g)) and r['query_gain'][n].view(np.int32) == g[qp].view(np.int32)
        d['qp'] = max(d['qp'], float(ref['gain'].max() - ref['gain'][qp]))
        for f, is_pos in c['aps'][h][n]:                              # what the answers fix is exact
            assert q[f] == (1.0 if is_pos else 0.0)
    print('T=%d ld=%d answers=%d: max |incl - ref| = %.3e (bar %.0e), |agree - ref| = %.3e (bar %.0e), |gain - ref| = %.3e bits (bar %.0e), '
          '|post_entropy - ref| = %.3e bits (bar %.0e), reference gain lost at query_point = %.3e bits (bar %.0e)'
          % (T, T + extra, h, d['incl'], INCL_BAR, d['agree'], AGREE_BAR, d['gain'], GAIN_BAR, d['ent'], ENT_BAR, d['qp'], 2 * GAIN_BAR))
    assert d['incl'] <= INCL_BAR
    assert d['agree'] <= AGREE_BAR
    assert d['gain'] <= GAIN_BAR
    assert d['ent'] <= ENT_BAR
    assert d['qp'] <= 2 * GAIN_BAR
    if extra:                                                         # the row stride changes nothing
        r0, _, _ = got(dev, T, 0, h)
        for k in ('query_point', 'query_gain', 'post_entropy', 'agree'):
            assert (r[k].view(np.int32) == r0[k].view(np.int32)).all(), k
        assert (r['incl'][:, :T].view(np.int32) == r0['incl'].view(np.int32)).all()


# ---------------------------------------------------------------------------------------------------------------- 2. edge rows
def test_edge_rows_and_untouched_memory(dev):
    from hual_amd import lib
    T, ld = 33, 40
    c = Q.case(T)
    s, e = c['s'].clone(), c['e'].clone()
    vlen = np.full(Q.N_ROWS, T, dtype=np.int32)
    tlen = np.full(Q.N_ROWS, T, dtype=np.int32)
    aps = [[] for _ in range(Q.N_ROWS)]
    vlen[0] = 1                                                       # v = 1: collapsed
    vlen[1], tlen[1] = 20, 25                                         # v < T < ld: columns [20, 25) zero, [25, 40) untouched
    s[2, 3] = float('nan')                                            # a NaN logit below v: poisoned
    vlen[3] = 20
    e[3, 30] = float('nan')                                           # a NaN logit at t >= v: not read
    aps[4] = [(5, True), (9, True), (7, False)]                       # a negative inside the positive hull: contradictory
    vlen[5] = 20
    aps[5] = [(4, True), (25, False), (20, True), (-3, False)]        # active points outside [0, v): ignored
    vlen[6] = 3
    aps[6] = [(0, False), (2, False), (1, False)]                     # every gap emptied: contradictory
    aps[7] = [(11, False), (12, True), (13, False)]                   # one consistent span: collapsed, not an error
    vlen[8] = 0                                                       # an empty clip: poisoned
    vlen[9] = T + 9                                                   # read as T
    vlen[10] = 20
    s[10, :], e[10, :] = -200.0, -200.0                               # the start certainly last, the end certainly first: every weight
    s[10, 19], e[10, 0] = 200.0, 200.0                                # with i <= j is exactly 0, Z = 0: poisoned
    s[11, 5] = float('inf')                                           # probabilities NaN, Z with them: poisoned
    aps[12] = [(3, False), (20, False), (9, False)]                   # negatives only: three gaps
    aps[13] = [(15, True), (2, False), (30, False), (6, False), (18, True)]
    sd, ed = pad_logits(dev, s, ld, 3), pad_logits(dev, e, ld, 4)
    ref = Q.set_ref(s, e, vlen, tlen, aps)
    status = [x['status'] for x in ref]
    assert [n for n in range(Q.N_ROWS) if status[n] == Q.POISONED] == [2, 8, 10, 11]
    assert [n for n in range(Q.N_ROWS) if status[n] == Q.CONTRADICTORY] == [4, 6]
    r = run_query(dev, sd, ed, vlen, tlen, aps)
    for n in range(Q.N_ROWS):
        x, T_n = ref[n], int(tlen[n])
        if x['status'] != Q.LIVE:
            assert r['query_point'][n] == -1 and r['query_gain'][n] == -1.0 and r['post_entropy'][n] == -1.0
            assert r['agree'][n] == (0.0 if x['status'] == Q.CONTRADICTORY else -1.0)
            assert (r['incl'][n, :T_n] == 0).all() and (r['gain'][n, :T_n] == 0).all()
            continue
        v = len(x['incl'])
        assert (r['incl'][n, v:T_n] == 0).all() and (r['gain'][n, v:T_n] == 0).all()
        assert np.abs(r['incl'][n, :v] - x['incl']).max() <= INCL_BAR and np.abs(r['gain'][n, :v] - x['gain']).max() <= GAIN_BAR
        assert abs(r['agree'][n] - x['agree']) <= AGREE_BAR and abs(r['post_entropy'][n] - x['post_entropy']) <= ENT_BAR
        qp = int(r['query_point'][n])
        assert qp == int(np.argmax(r['gain'][n, :v])) and x['gain'].max() - x['gain'][qp] <= 2 * GAIN_BAR
    for n in (0, 7):                                                  # collapsed: nothing to ask, the first frame, zero entropy
        assert r['query_point'][n] == 0 and r['query_gain'][n] == 0.0 and (r['gain'][n, :tlen[n]] == 0).all()
        assert r['post_entropy'][n] <= ENT_BAR and r['agree'][n] > 0
    assert r['agree'][0] == 1.0 and r['agree'][9] == 1.0 and len(ref[9]['incl']) == T and len(ref[1]['incl']) == 20
    assert 0.0 < r['agree'][13] < 1.0 and r['query_gain'][12] > 0 and r['query_gain'][13] > 0
    # incl = gain = NULL writes only the [N] outputs, and the same ones
    r2 = run_query(dev, sd, ed, vlen, tlen, aps, frames=False)
    assert r2['incl'] is None and r2['gain'] is None
    for k in ('query_point', 'query_gain', 'post_entropy', 'agree'):
        assert (r2[k].view(np.int32) == r[k].view(np.int32)).all(), k
    # a row longer than 256 frames: the binding refuses the set before the launch
    aset, keep = make_set(dev, [300, 20], [300, 20], [[], []], 300)
    z = torch.zeros(2, 300, device=dev)
    with pytest.raises(lib.HualError, match='256'):
        lib.al_query(aset, z, z, np.array([300, 20]))


# ---------------------------------------------------------------------------------------------------------------- 3. the other launches
def _argmax_hip(dev, s, e, m):
    from hual_amd import lib
    B, T = s.shape
    si = torch.empty(B, dtype=torch.int64, device=dev)
    ei = torch.empty(B, dtype=torch.int64, device=dev)
    lib.check(lib.load().hual_span_argmax(lib.ptr(s), lib.ptr(e), lib.ptr(m), lib.ptr(si), lib.ptr(ei), B, T, lib.stream_ptr()))
    return si.cpu().numpy(), ei.cpu().numpy()


@pytest.mark.parametrize('T', Q.TS)
def test_no_answers_agrees_with_the_span_launches(dev, T):
    """with no active point the posterior is the span distribution itself: agree = 1 and the entropy hual_span_expected_iou returns; and
    the probabilities are hual_span_argmax's - the reference that reproduces this kernel to 1e-6 from span_topk_ref.probabilities has
    its heaviest span where hual_span_argmax puts it, wherever its two heaviest weights are further apart than float32 rounds"""
    from hual_amd import lib
    c = Q.case(T)
    r, sd, ed = got(dev, T, 0, 0)
    vd = c['vlen'].to(dev)
    assert (r['agree'] == 1.0).all()
    z = torch.zeros(Q.N_ROWS, 1, dtype=torch.int64, device=dev)
    _, ent = lib.span_expected_iou(sd, ed, vd, z, z.clone())
    d = float(np.abs(r['post_entropy'].astype(np.float64) - ent.cpu().numpy().astype(np.float64)).max())
    print('T=%d: max |post_entropy - span_entropy of hual_span_expected_iou| = %.3e bits (bar %.0e)' % (T, d, ENT_BAR))
    assert d <= ENT_BAR
    mask = (torch.arange(T)[None, :] < c['vlen'][:, None]).float().to(dev)
    si, ei = _argmax_hip(dev, sd, ed, mask)
    compared = 0
    for n in range(Q.N_ROWS):
        v = int(c['v'][n])
        W, _ = Q.weights(c['ps'][n], c['pe'][n], v)
        top = np.sort(W[np.triu(np.ones((v, v), dtype=bool))])[::-1]
        if len(top) > 1 and top[0] - top[1] <= 2.0 ** -22 * top[0]:      # the float32 products of the two may tie or swap
            continue
        i, j = np.unravel_index(int(np.argmax(W)), W.shape)
        assert (int(si[n]), int(ei[n])) == (int(i), int(j)), n
        compared += 1
    assert compared >= Q.N_ROWS // 2


# ---------------------------------------------------------------------------------------------------------------- 4. capture
def test_query_in_a_captured_graph(dev):
    from hual_amd import lib
    T, h = 70, 3
    c = Q.case(T)
    want, sd, ed = got(dev, T, 7, h)
    ld = T + 7
    aset, keep = make_set(dev, c['vlen'].numpy(), [T] * Q.N_ROWS, c['aps'][h], ld)
    tl = np.full(Q.N_ROWS, T)

    def outs():
        return (torch.full((Q.N_ROWS, ld), FILL, device=dev), torch.full((Q.N_ROWS, ld), FILL, device=dev),
                torch.full((Q.N_ROWS,), 777, dtype=torch.int32, device=dev), torch.full((Q.N_ROWS,), FILL, device=dev),
                torch.full((Q.N_ROWS,), FILL, device=dev), torch.full((Q.N_ROWS,), FILL, device=dev))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        lib.al_query(aset, sd, ed, tl, out=outs())                    # (warm-up)
    torch.cuda.current_stream().wait_stream(side)
    out = outs()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        lib.al_query(aset, sd, ed, tl, out=out)
    for _ in range(2):
        for o in out:
            o.fill_(5)
        out[0][:, T:] = FILL
        out[1][:, T:] = FILL
        graph.replay()
        torch.cuda.synchronize()
        for o, k in zip(out, ('incl', 'gain', 'query_point', 'query_gain', 'post_entropy', 'agree')):
            assert (o.cpu().numpy().view(np.int32) == want[k].view(np.int32)).all(), k


# ---------------------------------------------------------------------------------------------------------------- 5. the label update
@functools.lru_cache(maxsize=None)
def _round_set():
    """the set of tests/test_gpu_al_round.py (al_synth.make_trainset, 40 samples) with the records of one inference pass"""
    from hual_amd import al, lib
    from hual_amd.dataset import DeviceDataset
    from hual_amd.model import SeqPAN
    N, vdim, max_vlen = 40, 64, 24
    recs, vis, data_gt, data_old = al_synth.make_trainset(N, 12, vdim, max_vlen, seed=3)
    cfg = lib.make_cfg(vdim=vdim, max_vlen=max_vlen, num_words=200, num_chars=30)
    wv = np.random.default_rng(1).normal(0, 0.4, size=(198, 300)).astype(np.float32)
    model = SeqPAN(cfg, wv)
    ds = DeviceDataset(recs, vis)
    s0, e0 = al.labels_from_times(data_old, ds.vlen_h)
    ds.set_labels(s0, e0)
    for r, a, b in zip(recs, s0, e0):
        r['s_ind'], r['e_ind'] = int(a), int(b)

    def batches():
        for lo in range(0, N, 16):
            sel = np.arange(lo, min(N, lo + 16))
            f = ds.assemble(sel, labels=False, min_chars=4)
            yield [recs[i] for i in sel], f['video'], f['video_seq_len'], f['word_ids'], f['char_ids']
    prop, _ = al.infer_trainset(model, batches(), mc_dropout=0.5)
    return dict(N=N, recs=recs, data_gt=data_gt, data_old=data_old, model=model, ds=ds, prop=prop)


def _prof(fn):
    """{kernel name: launches} of the library launches fn() makes"""
    from hual_amd import lib
    l = lib.load()
    lib.check(l.hual_prof_begin())
    out = fn()
    torch.cuda.synchronize()
    n = l.hual_prof_end()
    launches = {}
    for i in range(n):
        name = ctypes.create_string_buffer(256)
        cnt = ctypes.c_int64()
        lib.check(l.hual_prof_get(i, name, 256, ctypes.byref(cnt), None, None, None))
        launches[name.value.decode()] = int(cnt.value)
    return out, launches


def _answers(new, old):
    """per sample the active points `new` holds beyond `old`: (frame, is_pos)"""
    out = []
    for a, b in zip(new, old):
        had = b[4] if len(b) > 4 else {'pos_idx': [], 'neg_idx': []}
        out.append([(f, True) for f in a[4]['pos_idx'][len(had['pos_idx']):]] + [(f, False) for f in a[4]['neg_idx'][len(had['neg_idx']):]])
    return out


def test_update_labels_by_info_gain(dev):
    from hual_amd import al
    from test_gpu_mc_uncert import _bank_of_records
    S = _round_set()
    N, prop, coff = S['N'], S['prop'], al.get_coff('charades', 1)
    (new0, d0), k0 = _prof(lambda: al.update_labels(copy.deepcopy(S['data_old']), S['data_gt'], prop, coff, return_debug=True))
    (new0b, d0b), k0b = _prof(lambda: al.update_labels(copy.deepcopy(S['data_old']), S['data_gt'], prop, coff, return_debug=True,
                                                       observe_by='uncert_frame'))
    # the default: the launches, keys and results of before
    assert k0 == k0b and sum(k0.values()) == 2 and not any('al_query' in k for k in k0), k0
    assert sorted(d0) == sorted(['order', 'uncert_video', 'observe', 'uncert_frame', 'sprob', 'eprob', 'new_idx', 'gt_idx', 'old_idx', 'updater'])
    assert new0 == new0b and all(np.array_equal(d0[k], d0b[k]) for k in d0 if k != 'updater')
    # round 1 by information gain, then round 2 on its answers
    (new1, d1), k1 = _prof(lambda: al.update_labels(copy.deepcopy(S['data_old']), S['data_gt'], prop, coff, return_debug=True,
                                                    observe_by='info_gain'))
    assert sum(k1.values()) == 3 and sum(v for k, v in k1.items() if 'al_query' in k) == 1, k1
    assert sorted(d1) == sorted(list(d0) + ['query_point', 'query_gain', 'post_entropy', 'agree', 'observe_used'])
    new2, d2 = al.update_labels(copy.deepcopy(new1), S['data_gt'], prop, al.get_coff('charades', 2), return_debug=True, observe_by='info_gain')
    moved = 0
    for prev, new, d in ((S['data_old'], new1, d1), (new1, new2, d2)):
        for key in ('order', 'uncert_video', 'observe'):              # ranking and the reference's own frame are untouched
            if d is d1:
                np.testing.assert_array_equal(d[key], d0[key])
        want = np.where(d['query_gain'] > 0, d['query_point'], d['observe'])
        np.testing.assert_array_equal(d['observe_used'], want)
        sel = set(int(i) for i in d['order'][:(N + 1) // 2])
        ans = _answers(new, prev)
        for i in range(N):
            if i in sel:
                p = int(want[i])
                assert ans[i] == [(p, bool(d['gt_idx'][i, 0] <= p <= d['gt_idx'][i, 1]))], i
            else:
                assert ans[i] == []
        assert (d['query_gain'] > 0).sum() > N // 2 and (d['agree'] > 0).all() and (d['post_entropy'] >= 0).all()
        moved += int((want != d['observe']).sum())
    assert moved > 0                                                  # another question, not a relabelling of the reference's
    assert (d1['agree'] == 1.0).all() and (d2['agree'][sorted(sel)] <= 1.0).all() and (d2['agree'] < 1.0).any()
    # round 2 asks about the posterior its first answers left: the reference of the device logits, with those answers
    up = d2['updater']
    aps = [[(f, True) for f in r[4]['pos_idx']] + [(f, False) for f in r[4]['neg_idx']] for r in new1]
    ref = Q.set_ref(up._s0.cpu(), up._e0.cpu(), up.vlen_h, up.tlen_h, aps)
    for i in range(N):
        assert ref[i]['status'] == Q.LIVE
        assert abs(float(d2['agree'][i]) - ref[i]['agree']) <= AGREE_BAR and abs(float(d2['post_entropy'][i]) - ref[i]['post_entropy']) <= ENT_BAR
        assert ref[i]['gain'].max() - ref[i]['gain'][int(d2['query_point'][i])] <= 2 * GAIN_BAR
        assert np.abs(up.incl[i, :len(ref[i]['incl'])].cpu().numpy() - ref[i]['incl']).max() <= INCL_BAR
    # from a bank of the same passes: the same frames, the same labels
    bank = _bank_of_records(prop)
    new3, d3 = al.update_labels(copy.deepcopy(new1), S['data_gt'], prop, al.get_coff('charades', 2), return_debug=True, bank=bank,
                                observe_by='info_gain')
    for key in ('query_point', 'query_gain', 'post_entropy', 'agree', 'observe_used', 'observe', 'order'):
        np.testing.assert_array_equal(d3[key], d2[key])
    assert new3 == new2


def test_two_rounds_by_info_gain():
    from hual_amd import al
    S = _round_set()
    model, ds, N = S['model'], S['ds'], S['N']
    new1, prop1, m1 = al.run_round(model, ds, copy.deepcopy(S['data_old']), S['data_gt'], S['prop'], 'charades', 1, epochs=1, batch_size=16,
                                   lr=1e-3, drop_rate=0.2, observe_by='info_gain')
    new2, prop2, m2 = al.run_round(model, ds, copy.deepcopy(new1), S['data_gt'], prop1, 'charades', 2, epochs=1, batch_size=16, lr=1e-3,
                                   drop_rate=0.2, observe_by='info_gain')
    assert len(prop2) == N and m2['train_steps'] == 3 and 0.0 <= m2['miou'] <= 100.0
    first = _answers(new1, S['data_old'])
    second = _answers(new2, new1)
    assert sum(len(a) for a in first) == (N + 1) // 2 == sum(len(a) for a in second)
    assert first != second                                            # the second round's active points differ from the first's
