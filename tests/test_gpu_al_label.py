"""GPU: hual_al_mbr_label (the pseudo-label by minimum Bayes risk under the answered-point posterior) against the float64 enumeration
of its contract (tests/al_label_ref.py), its edge rows, the memory it must not touch, its agreement with hual_span_expected_iou and
hual_span_topk, graph capture, and the places it lands: LabelUpdater.mbr_label, al.update_labels(renew_by='posterior') and
al.run_round(renew_by=).

The bars (from the contract's arithmetic, include/hual_seqpan.h; not tuned):
  conf, old_conf  1e-6 absolute: the derivation of the expected-tIoU bar - float32 probabilities shared bit for bit with the
                  reference, float64 sums of non-negative terms, one final rounding to float32 of a value <= 1 (6e-8).
  new_idx         exact wherever the reference enumerates all of A: its margin between the best and the second-best span exceeds 1e-5
                  on every such row (tests/test_al_label.py), ten times the bar on R.  Where A is too large to enumerate (T = 256) the
                  chosen span has to be a member of A whose reference R is within 2e-6 (the bar on either side) of every probe's."""
import copy

import numpy as np
import pytest
import torch

import al_label_ref as L
import al_query_ref as Q
from test_gpu_al_query import _pads_intact, _prof, _round_set, _sentinel, make_set, pad_logits

pytestmark = pytest.mark.gpu

CONF_BAR = 1e-6
FILL, IFILL = 777.0, 777


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def run_label(dev, s, e, vlen, tlen, aps, old=None, sel=None, host_tlen=None):
    """one launch into sentinel-filled outputs -> dict of numpy arrays (old_conf None without old), after checking the memory around
    them.  sel: sample ids (any order) or None = all; host_tlen: what the binding is told where it is to differ from the device's"""
    from hual_amd import lib
    N, ld = s.shape
    aset, keep = make_set(dev, vlen, tlen, aps, ld)
    bufs = [_sentinel((N, 2), torch.int32, dev, IFILL), _sentinel((N,), torch.float32, dev, FILL),
            _sentinel((N,), torch.float32, dev, FILL) if old is not None else None]
    out = tuple(b[0] if b is not None else None for b in bufs)
    sel_d = torch.from_numpy(np.asarray(sel, dtype=np.int32)).to(dev) if sel is not None else None
    old_d = torch.from_numpy(np.ascontiguousarray(old, dtype=np.int32)).to(dev) if old is not None else None
    got = lib.al_mbr_label(aset, s, e, np.asarray(tlen if host_tlen is None else host_tlen), sel=sel_d, old_idx=old_d, out=out)
    assert all(a is b for a, b in zip(got, out))
    torch.cuda.synchronize()
    for b, fill in zip(bufs, (IFILL, FILL, FILL)):
        if b is not None:
            assert _pads_intact(b[1], b[2], fill)
    r = {k: (o.cpu().numpy() if o is not None else None) for k, o in zip(('new_idx', 'conf', 'old_conf'), out)}
    written = np.zeros(N, dtype=bool)
    written[np.arange(N) if sel is None else np.asarray(sel)] = True
    for k, fill in (('new_idx', IFILL), ('conf', FILL), ('old_conf', FILL)):      # only the selected rows are written, and all of them
        if r[k] is not None:
            assert (r[k][~written] == fill).all() and not (r[k][written] == fill).any(), k
    return r


_GOT = {}


def got(dev, T, extra, h):
    """the device results of the shared case (al_label_ref.case) of length T with ld = T + extra after h answers: computed once"""
    if (T, extra, h) not in _GOT:
        c = L.case(T)
        ld = T + extra
        s, e = pad_logits(dev, c['s'], ld, 1), pad_logits(dev, c['e'], ld, 2)
        _GOT[(T, extra, h)] = (run_label(dev, s, e, c['vlen'].numpy(), [T] * Q.N_ROWS, c['aps'][h], old=c['old'][h]), s, e)
    return _GOT[(T, extra, h)]


def check_rows(c, r, h):
    """every row of the shared case against the reference -> (max |conf - ref|, max |old_conf - ref|, rows compared by index)"""
    d_conf = d_old = 0.0
    by_index = 0
    for n in range(Q.N_ROWS):
        ref = c['lref'][h][n]
        st = ref['st']
        got_span = (int(r['new_idx'][n, 0]), int(r['new_idx'][n, 1]))
        assert 0.0 <= r['conf'][n] <= 1.0
        d_old = max(d_old, abs(float(r['old_conf'][n]) - c['old_conf'][h][n]))
        if ref['full']:
            assert got_span == ref['label'], (h, n, got_span, ref['label'], float(r['conf'][n]), ref['conf'])
            d_conf = max(d_conf, abs(float(r['conf'][n]) - ref['conf']))
            by_index += 1
            continue
        # A too large to enumerate pairs: a member of A, its value the reference's, and no probe better than it
        assert L.is_member(st, *got_span), (h, n, got_span)
        mine = L.span_R(st, *got_span)
        d_conf = max(d_conf, abs(float(r['conf'][n]) - mine))
        pa, pe_ = L.probes(st, got_span, 9100 + 16 * h + n)
        assert len(pa) > 257
        worst = float(L.expected_iou(st, pa, pe_).max() - mine)
        assert worst <= 2 * CONF_BAR, (h, n, got_span, worst)
    return d_conf, d_old, by_index


# ---------------------------------------------------------------------------------------------------------------- 1. values
@pytest.mark.parametrize('h', Q.HISTORIES)
@pytest.mark.parametrize('extra', [0, 7])
@pytest.mark.parametrize('T', [2, 33, 70])
def test_values_against_the_float64_reference(dev, T, extra, h):
    c = L.case(T)
    r, _, _ = got(dev, T, extra, h)
    d_conf, d_old, by_index = check_rows(c, r, h)
    print('T=%d ld=%d answers=%d: %d rows equal by index; max |conf - ref| = %.3e, max |old_conf - ref| = %.3e (bar %.0e)'
          % (T, T + extra, h, by_index, d_conf, d_old, CONF_BAR))
    assert by_index == Q.N_ROWS
    assert d_conf <= CONF_BAR
    assert d_old <= CONF_BAR
    if extra:                                                         # the row stride changes no bit
        r0, _, _ = got(dev, T, 0, h)
        for k in ('new_idx', 'conf', 'old_conf'):
            assert (r[k].view(np.int32) == r0[k].view(np.int32)).all(), k


# ---------------------------------------------------------------------------------------------------------------- 2. T = 256
@pytest.mark.parametrize('h', Q.HISTORIES)
def test_values_at_256_frames(dev, h):
    c = L.case(256)
    r, _, _ = got(dev, 256, 0, h)
    d_conf, d_old, by_index = check_rows(c, r, h)
    print('T=256 answers=%d: %d rows equal by index, %d by probes; max |conf - ref| = %.3e, max |old_conf - ref| = %.3e (bar %.0e)'
          % (h, by_index, Q.N_ROWS - by_index, d_conf, d_old, CONF_BAR))
    assert by_index == sum(x['full'] for x in c['lref'][h])
    assert d_conf <= CONF_BAR
    assert d_old <= CONF_BAR


# ---------------------------------------------------------------------------------------------------------------- 3. edge rows
def test_edge_rows_and_untouched_memory(dev):
    from hual_amd import lib
    T, ld = 33, 40
    c = Q.case(T)
    s, e = c['s'].clone(), c['e'].clone()
    vlen = np.full(Q.N_ROWS, T, dtype=np.int32)
    tlen = np.full(Q.N_ROWS, T, dtype=np.int32)
    aps = [[] for _ in range(Q.N_ROWS)]
    old = np.tile(np.array([[2, 10]]), (Q.N_ROWS, 1))
    vlen[0], old[0] = 1, (0, 0)                                       # v = 1: the one span
    vlen[1], tlen[1] = 20, 25                                         # v < T < ld
    s[2, 3] = float('nan')                                            # a NaN logit below v: poisoned
    vlen[3] = 20
    e[3, 30] = float('nan')                                           # a NaN logit at t >= v: not read
    aps[4] = [(5, True), (9, True), (7, False)]                       # a negative inside the positive hull: contradictory
    vlen[5] = 20
    aps[5] = [(4, True), (25, False), (20, True), (-3, False)]        # active points outside [0, v): ignored
    vlen[6], old[6] = 3, (0, 2)
    aps[6] = [(0, False), (2, False), (1, False)]                     # every frame negative: contradictory
    aps[7] = [(11, False), (12, True), (13, False)]                   # one consistent span: collapsed, not an error
    vlen[8] = 0                                                       # an empty clip: poisoned
    vlen[9], old[9] = T + 9, (-1, 5)                                  # read as T; an old span that starts before the clip
    vlen[10] = 20
    s[10, :], e[10, :] = -200.0, -200.0                               # every weight with i <= j is exactly 0, Z = 0: poisoned
    s[10, 19], e[10, 0] = 200.0, 200.0
    s[11, 5] = float('inf')                                           # an Inf logit: probabilities NaN, Z with them: poisoned
    aps[12] = [(3, False), (20, False), (9, False)]                   # negatives only: three gaps
    aps[13] = [(15, True), (2, False), (30, False), (6, False), (18, True)]
    old[14] = (5, 3)                                                  # an old span with a > e
    vlen[15], old[15] = 20, (4, 20)                                   # an old span that ends beyond v
    sd, ed = pad_logits(dev, s, ld, 3), pad_logits(dev, e, ld, 4)
    ref = L.set_ref(s, e, vlen, tlen, aps)
    status = [x['status'] for x in ref]
    assert [n for n in range(Q.N_ROWS) if status[n] == L.POISONED] == [2, 8, 10, 11]
    assert [n for n in range(Q.N_ROWS) if status[n] == L.CONTRADICTORY] == [4, 6]
    r = run_label(dev, sd, ed, vlen, tlen, aps, old=old)              # sel NULL: every row written (run_label checks)
    for n in range(Q.N_ROWS):
        x = ref[n]
        if x['status'] != L.LIVE:
            assert tuple(r['new_idx'][n]) == (-1, -1) and r['conf'][n] == -1.0 and r['old_conf'][n] == -1.0, n
            continue
        assert x['full'] and x['margin'] > 1e-5
        assert tuple(int(t) for t in r['new_idx'][n]) == x['label'], (n, r['new_idx'][n], x['label'])
        assert abs(float(r['conf'][n]) - x['conf']) <= CONF_BAR, n
        v = x['st']['v']
        if L.old_valid(old[n], v):
            assert abs(float(r['old_conf'][n]) - L.span_R(x['st'], *old[n])) <= CONF_BAR, n
        else:
            assert r['old_conf'][n] == -1.0, n
    assert [n for n in range(Q.N_ROWS) if status[n] == L.LIVE and r['old_conf'][n] == -1.0] == [9, 14, 15]
    assert tuple(r['new_idx'][0]) == (0, 0) and r['conf'][0] == 1.0 and r['old_conf'][0] == 1.0
    assert tuple(r['new_idx'][7]) == (12, 12) and r['conf'][7] == 1.0 and r['old_conf'][7] == 0.0      # (2, 10) misses the one span
    assert ref[9]['st']['v'] == T and ref[1]['st']['v'] == 20
    lab = r['new_idx']
    assert lab[5, 0] <= 4 and lab[5, 1] >= 4 and lab[5, 1] < 20      # row 5: the positive at 4 alone counts
    assert lab[13, 0] > 6 and lab[13, 0] <= 15 and 18 <= lab[13, 1] < 30
    assert not any(lab[12, 0] <= f <= lab[12, 1] for f in (3, 9, 20))
    # a strict subset in shuffled order writes the selected rows only (run_label checks the others' fill), and the same bits
    sel = [13, 2, 7, 0, 12, 4, 9]
    r2 = run_label(dev, sd, ed, vlen, tlen, aps, old=old, sel=sel)
    for k in ('new_idx', 'conf', 'old_conf'):
        assert (r2[k][sel].view(np.int32) == r[k][sel].view(np.int32)).all(), k
    # old_idx = old_conf = NULL: the same labels and values
    r3 = run_label(dev, sd, ed, vlen, tlen, aps)
    assert r3['old_conf'] is None
    for k in ('new_idx', 'conf'):
        assert (r3[k].view(np.int32) == r[k].view(np.int32)).all(), k
    # a row of 300 frames the host was not told about: poisoned on the device, its neighbours untouched by it
    ld2 = 304
    s2, e2 = pad_logits(dev, c['s'][:3], ld2, 5), pad_logits(dev, c['e'][:3], ld2, 6)
    r4 = run_label(dev, s2, e2, [T, T, T], [T, 300, T], [[], [], []], old=old[:3], host_tlen=[T, T, T])
    assert tuple(r4['new_idx'][1]) == (-1, -1) and r4['conf'][1] == -1.0 and r4['old_conf'][1] == -1.0
    r5 = run_label(dev, s2, e2, [T, T, T], [T, T, T], [[], [], []], old=old[:3])
    for k in ('new_idx', 'conf', 'old_conf'):
        assert (r4[k][[0, 2]].view(np.int32) == r5[k][[0, 2]].view(np.int32)).all(), k
    assert r5['new_idx'][1, 0] >= 0
    # a row longer than 256 frames the host knows of: the binding refuses the set before the launch
    aset, keep = make_set(dev, [300, 20], [300, 20], [[], []], 300)
    z = torch.zeros(2, 300, device=dev)
    with pytest.raises(lib.HualError, match='256'):
        lib.al_mbr_label(aset, z, z, np.array([300, 20]))


# ---------------------------------------------------------------------------------------------------------------- 4. the span launches
@pytest.mark.parametrize('T', Q.TS)
def test_no_answers_agrees_with_the_span_launches(dev, T):
    """with no active point the posterior is the span distribution itself: the label's conf is what hual_span_expected_iou says of that
    span, and none of the 16 proposals of hual_span_topk has a larger expected tIoU"""
    from hual_amd import lib
    c = L.case(T)
    r, sd, ed = got(dev, T, 0, 0)
    vd = c['vlen'].to(dev)
    lab = torch.from_numpy(r['new_idx'].astype(np.int64)).to(dev)
    assert (r['new_idx'] >= 0).all()
    mine, _ = lib.span_expected_iou(sd, ed, vd, lab[:, :1].contiguous(), lab[:, 1:].contiguous())
    d = float(np.abs(mine.cpu().numpy()[:, 0].astype(np.float64) - r['conf'].astype(np.float64)).max())
    st, en, _ = lib.span_topk(sd, ed, vd, 16)
    prop, _ = lib.span_expected_iou(sd, ed, vd, st, en)
    prop = prop.cpu().numpy().astype(np.float64)                      # (-1.0 in the slots no proposal fills)
    over = float((prop - r['conf'].astype(np.float64)[:, None]).max())
    print('T=%d: max |conf - expected_iou of the label| = %.3e (bar %.0e); best proposal of 16 exceeds the label by %.3e (bar %.0e)'
          % (T, d, CONF_BAR, over, 2 * CONF_BAR))
    assert d <= CONF_BAR
    assert over <= 2 * CONF_BAR


# ---------------------------------------------------------------------------------------------------------------- 5. capture
def test_label_in_a_captured_graph(dev):
    from hual_amd import lib
    T, h = 70, 3
    c = L.case(T)
    want, sd, ed = got(dev, T, 7, h)
    ld = T + 7
    aset, keep = make_set(dev, c['vlen'].numpy(), [T] * Q.N_ROWS, c['aps'][h], ld)
    tl = np.full(Q.N_ROWS, T)
    old_d = torch.from_numpy(c['old'][h].astype(np.int32)).to(dev)

    def outs():
        return (torch.full((Q.N_ROWS, 2), IFILL, dtype=torch.int32, device=dev), torch.full((Q.N_ROWS,), FILL, device=dev),
                torch.full((Q.N_ROWS,), FILL, device=dev))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        lib.al_mbr_label(aset, sd, ed, tl, old_idx=old_d, out=outs())      # (warm-up)
    torch.cuda.current_stream().wait_stream(side)
    out = outs()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        lib.al_mbr_label(aset, sd, ed, tl, old_idx=old_d, out=out)
    for _ in range(2):
        for o in out:
            o.fill_(5)
        graph.replay()
        torch.cuda.synchronize()
        for o, k in zip(out, ('new_idx', 'conf', 'old_conf')):
            assert (o.cpu().numpy().view(np.int32) == want[k].view(np.int32)).all(), k


# ---------------------------------------------------------------------------------------------------------------- 6. the label update
def _time_of(idx, vl, dur):
    """index_to_time as update_labels writes it (update_label.py:50-57)"""
    return [round(int(t) / (vl - 1) * dur, 2) for t in idx]


def test_update_labels_by_posterior(dev):
    from hual_amd import al
    S = _round_set()
    N, prop, coff = S['N'], S['prop'], al.get_coff('charades', 1)
    (new0, d0), k0 = _prof(lambda: al.update_labels(copy.deepcopy(S['data_old']), S['data_gt'], prop, coff, return_debug=True))
    (new0b, d0b), k0b = _prof(lambda: al.update_labels(copy.deepcopy(S['data_old']), S['data_gt'], prop, coff, return_debug=True,
                                                       renew_by='heuristic'))
    # the default: the launches, keys and results of before
    assert k0 == k0b and sum(k0.values()) == 2 and not any('al_mbr_label' in k for k in k0), k0
    assert sorted(d0) == sorted(['order', 'uncert_video', 'observe', 'uncert_frame', 'sprob', 'eprob', 'new_idx', 'gt_idx', 'old_idx', 'updater'])
    assert new0 == new0b and all(np.array_equal(d0[k], d0b[k]) for k in d0 if k != 'updater')
    # by the posterior: one launch instead of the renew, every selected sample live
    (new1, d1), k1 = _prof(lambda: al.update_labels(copy.deepcopy(S['data_old']), S['data_gt'], prop, coff, return_debug=True,
                                                    renew_by='posterior'))
    assert sum(k1.values()) == 2 and sum(v for k, v in k1.items() if 'al_mbr_label' in k) == 1 and not any('al_renew' in k for k in k1), k1
    assert sorted(d1) == sorted(list(d0) + ['label_conf', 'old_conf', 'renewed_by_posterior'])
    for key in ('order', 'uncert_video', 'observe', 'gt_idx', 'old_idx'):      # ranking, selection and the question are untouched
        np.testing.assert_array_equal(d1[key], d0[key])
    sel = d1['order'][:(N + 1) // 2]
    insel = np.zeros(N, dtype=bool)
    insel[sel] = True
    np.testing.assert_array_equal(d1['renewed_by_posterior'], insel)
    up = d1['updater']
    lab, conf, oconf = up.mbr_label(sel, d1['old_idx'])              # the kernel's label on the updater's set: this round's answers included
    np.testing.assert_array_equal(lab[sel], d1['new_idx'][sel])
    assert (conf[sel].view(np.int32) == d1['label_conf'][sel].view(np.int32)).all()
    assert (oconf[sel].view(np.int32) == d1['old_conf'][sel].view(np.int32)).all()
    aps = [[(f, True) for f in r[4]['pos_idx']] + [(f, False) for f in r[4]['neg_idx']] for r in new1]
    ref = L.set_ref(up._s0.cpu(), up._e0.cpu(), up.vlen_h, up.tlen_h, aps)
    moved = compared = 0
    for i in range(N):
        if not insel[i]:
            assert new1[i][2] == S['data_old'][i][2] and new1[i][4] == {'pos_idx': [], 'neg_idx': []}      # unselected: span kept
            continue
        assert len(aps[i]) == 1 and ref[i]['status'] == L.LIVE
        vl, dur = int(up.vlen_h[i]), new1[i][1]
        assert new1[i][2] == _time_of(lab[i], vl, dur), i           # the unchanged index -> time line on the kernel's label
        a, e = int(lab[i, 0]), int(lab[i, 1])
        f, is_pos = aps[i][0]
        assert (a <= f <= e) == is_pos                                # the label obeys this round's answer
        assert abs(float(conf[i]) - L.span_R(ref[i]['st'], a, e)) <= CONF_BAR
        assert conf[i] >= oconf[i] - 2 * CONF_BAR or not L.is_member(ref[i]['st'], *d1['old_idx'][i])
        if ref[i]['margin'] > 1e-5:
            assert (a, e) == ref[i]['label'], i
            compared += 1
        moved += new1[i][2] != new0[i][2]
    assert compared >= len(sel) // 2 and moved > 0                    # another label than the heuristic's
    # contradictory answers made by hand: the heuristic's span for those rows, the posterior's for the others
    data_c = copy.deepcopy(S['data_old'])
    hand = [i for i in range(N) if i % 2 == 0 and int(up.vlen_h[i]) >= 10]
    for i, r in enumerate(data_c):
        r.append({'pos_idx': [2, 8], 'neg_idx': [5]} if i in hand else {'pos_idx': [], 'neg_idx': []})
    (new_h, d_h), k_h = _prof(lambda: al.update_labels(copy.deepcopy(data_c), S['data_gt'], prop, coff, return_debug=True))
    (new_p, d_p), k_p = _prof(lambda: al.update_labels(copy.deepcopy(data_c), S['data_gt'], prop, coff, return_debug=True,
                                                       renew_by='posterior'))
    np.testing.assert_array_equal(d_p['order'], d_h['order'])
    sel_c = d_p['order'][:(N + 1) // 2]
    dead = [int(i) for i in sel_c if i in hand]
    assert dead and len(dead) < len(sel_c), (dead, sel_c)
    assert sum(k_p.values()) == 3 and sum(v for k, v in k_p.items() if 'al_mbr_label' in k) == 1 and \
        sum(v for k, v in k_p.items() if 'al_renew' in k) == 1, k_p
    for i in sel_c:
        if int(i) in dead:
            assert not d_p['renewed_by_posterior'][i] and d_p['label_conf'][i] == -1.0 and d_p['old_conf'][i] == -1.0
            np.testing.assert_array_equal(d_p['new_idx'][i], d_h['new_idx'][i])
            assert new_p[i][2] == new_h[i][2]
        else:
            assert d_p['renewed_by_posterior'][i] and d_p['new_idx'][i, 0] >= 0 and 0.0 <= d_p['label_conf'][i] <= 1.0
            assert new_p[i][2] == _time_of(d_p['new_idx'][i], int(up.vlen_h[i]), new_p[i][1])
    assert not d_p['renewed_by_posterior'][~np.isin(np.arange(N), sel_c)].any()


def test_a_round_by_posterior(monkeypatch):
    from hual_amd import al
    S = _round_set.__wrapped__()                                      # a set of its own: the round trains the model and relabels the dataset
    model, ds, N = S['model'], S['ds'], S['N']
    seen = {}
    plain = al.update_labels

    def observed(*args, **kw):
        out, seen['launches'] = _prof(lambda: plain(*args, **kw))
        seen['renew_by'] = kw.get('renew_by')
        return out
    monkeypatch.setattr(al, 'update_labels', observed)
    new1, prop1, m1 = al.run_round(model, ds, copy.deepcopy(S['data_old']), S['data_gt'], S['prop'], 'charades', 1, epochs=1, batch_size=16,
                                   lr=1e-3, drop_rate=0.2, renew_by='posterior')
    assert seen['renew_by'] == 'posterior' and sum(v for k, v in seen['launches'].items() if 'al_mbr_label' in k) == 1, seen
    assert len(prop1) == N and m1['train_steps'] == 3 and 0.0 <= m1['miou'] <= 100.0
    assert sum(r[2] != o[2] for r, o in zip(new1, S['data_old'])) > 0
