"""GPU: hual_al_label_gain (per frame, the tIoU the minimum-Bayes-risk pseudo-label is expected to gain from the frame's answer under
the answered-point posterior) against the float64 enumeration of its contract (tests/al_gain_ref.py), its agreement with
hual_al_mbr_label and hual_al_query, candidate lists, its edge rows, the memory it must not touch, graph capture, and the places it
lands: LabelUpdater.label_gain, al.update_labels(acquire_by='label_gain') and al.run_round(acquire_by=).

The bars (from the contract's arithmetic, include/hual_seqpan.h; not tuned):
  gain, ask_gain, value  1e-6 absolute, the CONF_BAR of hual_al_mbr_label, and the same arithmetic: float32 probabilities shared bit for
                         bit with the reference, float64 sums of non-negative terms, a difference of three values <= 1, one final
                         rounding to float32 of a value <= 1 (6e-8).
  ask_point              exact on every state whose reference margin between the best and the second-best frame exceeds 1e-5, ten times
                         the bar on a gain (tests/test_al_gain.py counts them); on the other states with a gain to be had the kernel's
                         frame has a reference gain within 2e-6 (the bar on either side) of the best.

Measured on an MI355X: max |gain - ref| 1.5e-8, |ask_gain - ref| 1.5e-8, |value - ref| 3.0e-8."""
import copy

import numpy as np
import pytest
import torch

import al_gain_ref as G
import al_label_ref as L
import al_query_ref as Q
from test_al_gain import BY_INDEX
from test_gpu_al_label import _time_of, run_label
from test_gpu_al_query import _pads_intact, _prof, _round_set, _sentinel, make_set, pad_logits, run_query

pytestmark = pytest.mark.gpu

GAIN_BAR = 1e-6
FILL, IFILL = 777.0, 777
NAMES = ('gain', 'ask_point', 'ask_gain', 'value')


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def run_gain(dev, s, e, vlen, tlen, aps, sel=None, cand=None, frames=True, host_tlen=None):
    """one launch into sentinel-filled outputs -> dict of numpy arrays (gain None with frames=False), after checking the memory around
    and beyond them.  sel: sample ids (any order) or None = all; cand: int [N, M] or None = every frame; host_tlen: what the binding is
    told where it is to differ from the device's"""
    from hual_amd import lib
    N, ld = s.shape
    aset, keep = make_set(dev, vlen, tlen, aps, ld)
    bufs = [_sentinel((N, ld), torch.float32, dev, FILL) if frames else None, _sentinel((N,), torch.int32, dev, IFILL),
            _sentinel((N,), torch.float32, dev, FILL), _sentinel((N,), torch.float32, dev, FILL)]
    out = tuple(b[0] if b is not None else None for b in bufs)
    sel_d = torch.from_numpy(np.asarray(sel, dtype=np.int32)).to(dev) if sel is not None else None
    cand_d = torch.from_numpy(np.ascontiguousarray(cand, dtype=np.int32)).to(dev) if cand is not None else None
    got = lib.al_label_gain(aset, s, e, np.asarray(tlen if host_tlen is None else host_tlen), sel=sel_d, cand=cand_d, frames=frames, out=out)
    assert all(a is b for a, b in zip(got, out))
    torch.cuda.synchronize()
    for b, fill in zip(bufs, (FILL, IFILL, FILL, FILL)):
        if b is not None:
            assert _pads_intact(b[1], b[2], fill)
    r = {k: (o.cpu().numpy() if o is not None else None) for k, o in zip(NAMES, out)}
    written = np.zeros(N, dtype=bool)
    written[np.arange(N) if sel is None else np.asarray(sel)] = True
    for k, fill in zip(NAMES[1:], (IFILL, FILL, FILL)):               # only the selected rows are written, and all of them
        assert (r[k][~written] == fill).all() and not (r[k][written] == fill).any(), k
    if frames:                                                        # of a selected row the columns [0, tlen), nothing else
        inside = written[:, None] & (np.arange(ld)[None, :] < np.minimum(np.asarray(tlen), ld)[:, None])
        assert (r['gain'][~inside] == FILL).all() and not (r['gain'][inside] == FILL).any()
    return r


_GOT = {}


def got(dev, T, extra, h):
    """the device results of the shared case (al_gain_ref.case) of length T with ld = T + extra after h answers, over every frame of the
    rows al_gain_ref.ROWS[T] (a strict subset goes through sel): computed once"""
    if (T, extra, h) not in _GOT:
        c = G.case(T)
        ld = T + extra
        s, e = pad_logits(dev, c['s'], ld, 1), pad_logits(dev, c['e'], ld, 2)
        sel = None if len(G.ROWS[T]) == Q.N_ROWS else list(G.ROWS[T])
        _GOT[(T, extra, h)] = (run_gain(dev, s, e, c['vlen'].numpy(), [T] * Q.N_ROWS, c['aps'][h], sel=sel), s, e)
    return _GOT[(T, extra, h)]


def check_row(r, n, ref, T_n):
    """row n of a launch over the frames ref['frames'] against its reference -> (|gain - ref|, |ask_gain - ref|, |value - ref|, was the
    frame compared by index)"""
    if ref['status'] != G.LIVE:
        assert r['ask_point'][n] == -1 and r['ask_gain'][n] == -1.0 and r['value'][n] == -1.0 and (r['gain'][n, :T_n] == 0).all(), n
        return 0.0, 0.0, 0.0, False
    v = len(ref['gain'])
    g = r['gain'][n, :v]
    assert (r['gain'][n, v:T_n] == 0).all() and g.min() >= 0.0 and g.max() <= 1.0
    assert (g[[t for t in range(v) if t not in ref['frames']]] == 0).all()
    d = (float(np.abs(g.astype(np.float64) - ref['gain']).max()), abs(float(r['ask_gain'][n]) - ref['ask_gain']),
         abs(float(r['value'][n]) - ref['value']))
    ap = int(r['ask_point'][n])
    if not ref['frames']:
        assert ap == -1 and r['ask_gain'][n] == 0.0
        return d + (False,)
    # the kernel's frame is an evaluated one, its ask_gain that frame's gain and the row's largest (rounding to float32 is monotonic)
    assert ap in ref['frames'] and r['ask_gain'][n] == g[ap] == g.max(), (n, ap)
    if G.by_index(ref):
        assert ap == ref['ask_point'], (n, ap, ref['ask_point'], ref['margin'])
    elif ref['ask_gain'] > 1e-9:                                      # a runner-up within ten bars: any frame within the bar on either side
        assert ref['ask_gain'] - ref['gain'][ap] <= 2 * GAIN_BAR, (n, ap, ref['ask_point'])
    else:
        assert r['ask_gain'][n] <= GAIN_BAR, n
    return d + (G.by_index(ref),)


# ---------------------------------------------------------------------------------------------------------------- 1. values
@pytest.mark.parametrize('h', Q.HISTORIES)
@pytest.mark.parametrize('extra', [0, 7])
@pytest.mark.parametrize('T', sorted(G.ROWS))
def test_values_against_the_float64_reference(dev, T, extra, h):
    c = G.case(T)
    r, _, _ = got(dev, T, extra, h)
    d = np.zeros(3)
    by_index = 0
    for n in G.ROWS[T]:
        *dn, exact = check_row(r, n, c['gref'][h][n], T)
        d = np.maximum(d, dn)
        by_index += exact
    print('T=%d ld=%d answers=%d: %d of %d rows equal by index; max |gain - ref| = %.3e, |ask_gain - ref| = %.3e, |value - ref| = %.3e '
          '(bar %.0e)' % (T, T + extra, h, by_index, len(G.ROWS[T]), d[0], d[1], d[2], GAIN_BAR))
    assert by_index == BY_INDEX[T][Q.HISTORIES.index(h)]
    assert (d <= GAIN_BAR).all()
    if extra:                                                         # the row stride changes no bit
        r0, _, _ = got(dev, T, 0, h)
        rows = list(G.ROWS[T])
        for k in NAMES[1:]:
            assert (r[k][rows].view(np.int32) == r0[k][rows].view(np.int32)).all(), k
        assert (r['gain'][rows, :T].view(np.int32) == r0['gain'][rows].view(np.int32)).all()


# ---------------------------------------------------------------------------------------------------------------- 2. the other launches
@pytest.mark.parametrize('h', Q.HISTORIES)
@pytest.mark.parametrize('T', sorted(G.ROWS))
def test_agrees_with_the_label_and_the_query(dev, T, h):
    """value is the conf of hual_al_mbr_label on the same set, bit for bit; and a frame whose answer hual_al_query calls certain (incl
    exactly 0 or 1) has gain exactly 0"""
    c = G.case(T)
    r, sd, ed = got(dev, T, 0, h)
    rows = list(G.ROWS[T])
    lab = run_label(dev, sd, ed, c['vlen'].numpy(), [T] * Q.N_ROWS, c['aps'][h], sel=None if len(rows) == Q.N_ROWS else rows)
    assert (r['value'][rows].view(np.int32) == lab['conf'][rows].view(np.int32)).all()
    q = run_query(dev, sd, ed, c['vlen'].numpy(), [T] * Q.N_ROWS, c['aps'][h])
    certain = (q['incl'][rows] == 0) | (q['incl'][rows] == 1)
    assert (certain.any() or h == 0) and (r['gain'][rows][certain] == 0).all()      # (full clips without an answer hold no certain frame)
    assert (r['gain'][rows][~certain] > 0).any() or T == 2


# ---------------------------------------------------------------------------------------------------------------- 3. candidate lists
def test_candidate_list_is_the_all_frames_launch_at_its_frames(dev):
    T, h = 33, 3
    c = G.case(T)
    full, sd, ed = got(dev, T, 0, h)
    v = c['v']
    cand = np.array([[(3 * n + 1) % int(v[n]), -1, int(v[n]) + n % 3, (7 * n + 5) % int(v[n])] for n in range(Q.N_ROWS)])
    r = run_gain(dev, sd, ed, c['vlen'].numpy(), [T] * Q.N_ROWS, c['aps'][h], cand=cand)
    for n in range(Q.N_ROWS):
        listed = [int(cand[n, 0]), int(cand[n, 3])]
        want = np.zeros(T, dtype=np.float32)
        want[listed] = full['gain'][n, listed]
        assert (r['gain'][n].view(np.int32) == want.view(np.int32)).all(), n      # the same bits at the listed frames, 0 elsewhere
        first = listed[int(np.argmax(want[listed]))]                  # the first listed frame of maximal gain
        assert r['ask_point'][n] == first and r['ask_gain'][n] == want[first], n
    assert (r['value'].view(np.int32) == full['value'].view(np.int32)).all()
    # no listed frame inside the clip: nothing evaluated
    none = run_gain(dev, sd, ed, c['vlen'].numpy(), [T] * Q.N_ROWS, c['aps'][h], cand=np.tile(np.array([[-1, T]]), (Q.N_ROWS, 1)))
    assert (none['ask_point'] == -1).all() and (none['ask_gain'] == 0).all() and (none['gain'] == 0).all()
    assert (none['value'].view(np.int32) == full['value'].view(np.int32)).all()


def test_candidates_at_256_frames(dev):
    """T = 256 after 6 answers, four candidates per row: the frame of most information (the reference's own), its two neighbours and
    the middle of the clip.  Against the enumeration where al_label_ref enumerates the row in full; elsewhere the gain's range."""
    T, h = 256, 6
    c = L.case(T)
    sd, ed = pad_logits(dev, c['s'], T, 1), pad_logits(dev, c['e'], T, 2)
    cand = np.array([[c['ref'][h][n]['query_point'] + k for k in (-1, 0, 1)] + [int(c['v'][n]) // 2] for n in range(Q.N_ROWS)])
    r = run_gain(dev, sd, ed, c['vlen'].numpy(), [T] * Q.N_ROWS, c['aps'][h], cand=cand)
    lab = run_label(dev, sd, ed, c['vlen'].numpy(), [T] * Q.N_ROWS, c['aps'][h])
    assert (r['value'].view(np.int32) == lab['conf'].view(np.int32)).all()
    d = np.zeros(3)
    full = 0
    for n in range(Q.N_ROWS):
        if c['lref'][h][n]['full']:
            ref = G.gain_ref(c['ps'][n], c['pe'][n], int(c['v'][n]), c['aps'][h][n], frames=cand[n])
            d = np.maximum(d, check_row(r, n, ref, T)[:3])
            full += 1
        else:
            assert r['gain'][n].min() >= 0.0 and r['gain'][n].max() <= 1.0 - r['value'][n] + GAIN_BAR
    print('T=256 answers=%d: %d rows against the enumeration; max |gain - ref| = %.3e, |ask_gain - ref| = %.3e, |value - ref| = %.3e '
          '(bar %.0e)' % (h, full, d[0], d[1], d[2], GAIN_BAR))
    assert full >= Q.N_ROWS // 2 and (r['ask_gain'] > 0).sum() >= Q.N_ROWS // 2
    assert (d <= GAIN_BAR).all()


# ---------------------------------------------------------------------------------------------------------------- 4. edge rows
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
    aps[6] = [(0, False), (2, False), (1, False)]                     # every frame negative: contradictory
    aps[7] = [(11, False), (12, True), (13, False)]                   # one consistent span: collapsed, not an error
    vlen[8] = 0                                                       # an empty clip: poisoned
    vlen[9] = T + 9                                                   # read as T
    vlen[10] = 20
    s[10, :], e[10, :] = -200.0, -200.0                               # every weight with i <= j is exactly 0, Z = 0: poisoned
    s[10, 19], e[10, 0] = 200.0, 200.0
    s[11, 5] = float('inf')                                           # an Inf logit: probabilities NaN, Z with them: poisoned
    aps[12] = [(3, False), (20, False), (9, False)]                   # negatives only: three gaps
    aps[13] = [(15, True), (2, False), (30, False), (6, False), (18, True)]
    sd, ed = pad_logits(dev, s, ld, 3), pad_logits(dev, e, ld, 4)
    ref = G.set_ref(s, e, vlen, tlen, aps)
    status = [x['status'] for x in ref]
    assert [n for n in range(Q.N_ROWS) if status[n] == G.POISONED] == [2, 8, 10, 11]
    assert [n for n in range(Q.N_ROWS) if status[n] == G.CONTRADICTORY] == [4, 6]
    r = run_gain(dev, sd, ed, vlen, tlen, aps)                        # sel NULL: every row written (run_gain checks)
    d = np.zeros(3)
    for n in range(Q.N_ROWS):
        d = np.maximum(d, check_row(r, n, ref[n], int(tlen[n]))[:3])
    assert (d <= GAIN_BAR).all(), d
    for n in (0, 7):                                                  # collapsed: nothing to gain, the first frame, a label worth 1
        assert r['ask_point'][n] == 0 and r['ask_gain'][n] == 0.0 and r['value'][n] == 1.0 and (r['gain'][n, :tlen[n]] == 0).all()
    assert len(ref[9]['gain']) == T and len(ref[1]['gain']) == 20
    g = r['gain']
    assert (g[5, 4] == 0) and r['ask_gain'][5] > 0                    # row 5: the positive at 4 alone counts, and is certain
    assert (g[12, [3, 9, 20]] == 0).all() and r['ask_gain'][12] > 0   # an answered negative is certain; the gaps are not
    assert (g[13, :7] == 0).all() and (g[13, 15:19] == 0).all() and (g[13, 30:T] == 0).all() and r['ask_gain'][13] > 0
    # a strict subset in shuffled order writes the selected rows only (run_gain checks the others' fill), and the same bits
    sel = [13, 2, 7, 0, 12, 4, 9]
    r2 = run_gain(dev, sd, ed, vlen, tlen, aps, sel=sel)
    for k in NAMES[1:]:
        assert (r2[k][sel].view(np.int32) == r[k][sel].view(np.int32)).all(), k
    for n in sel:
        assert (r2['gain'][n, :tlen[n]].view(np.int32) == r['gain'][n, :tlen[n]].view(np.int32)).all(), n
    # gain = NULL writes only the [N] outputs, and the same ones
    r3 = run_gain(dev, sd, ed, vlen, tlen, aps, frames=False)
    assert r3['gain'] is None
    for k in NAMES[1:]:
        assert (r3[k].view(np.int32) == r[k].view(np.int32)).all(), k
    # a row of 300 frames the host was not told about: poisoned on the device, its neighbours untouched by it
    ld2 = 304
    s2, e2 = pad_logits(dev, c['s'][:3], ld2, 5), pad_logits(dev, c['e'][:3], ld2, 6)
    r4 = run_gain(dev, s2, e2, [T, T, T], [T, 300, T], [[], [], []], host_tlen=[T, T, T])
    assert r4['ask_point'][1] == -1 and r4['ask_gain'][1] == -1.0 and r4['value'][1] == -1.0 and (r4['gain'][1, :300] == 0).all()
    r5 = run_gain(dev, s2, e2, [T, T, T], [T, T, T], [[], [], []])
    for k in NAMES:
        assert (r4[k][[0, 2]].view(np.int32) == r5[k][[0, 2]].view(np.int32)).all(), k
    assert r5['ask_point'][1] >= 0
    # a row longer than 256 frames the host knows of: the binding refuses the set before the launch
    aset, keep = make_set(dev, [300, 20], [300, 20], [[], []], 300)
    z = torch.zeros(2, 300, device=dev)
    with pytest.raises(lib.HualError, match='256'):
        lib.al_label_gain(aset, z, z, np.array([300, 20]))


# ---------------------------------------------------------------------------------------------------------------- 5. capture
def test_gain_in_a_captured_graph(dev):
    from hual_amd import lib
    T, h = 33, 3
    c = G.case(T)
    want, sd, ed = got(dev, T, 7, h)
    ld = T + 7
    aset, keep = make_set(dev, c['vlen'].numpy(), [T] * Q.N_ROWS, c['aps'][h], ld)
    tl = np.full(Q.N_ROWS, T)

    def outs():
        return (torch.full((Q.N_ROWS, ld), FILL, device=dev), torch.full((Q.N_ROWS,), IFILL, dtype=torch.int32, device=dev),
                torch.full((Q.N_ROWS,), FILL, device=dev), torch.full((Q.N_ROWS,), FILL, device=dev))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        lib.al_label_gain(aset, sd, ed, tl, out=outs())               # (warm-up)
    torch.cuda.current_stream().wait_stream(side)
    out = outs()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        lib.al_label_gain(aset, sd, ed, tl, out=out)
    for _ in range(2):
        for o in out:
            o.fill_(5)
        out[0][:, T:] = FILL
        graph.replay()
        torch.cuda.synchronize()
        for o, k in zip(out, NAMES):
            assert (o.cpu().numpy().view(np.int32) == want[k].view(np.int32)).all(), k


# ---------------------------------------------------------------------------------------------------------------- 6. the label update
def test_update_labels_by_label_gain(dev):
    from hual_amd import al
    S = _round_set()
    N, prop, coff = S['N'], S['prop'], al.get_coff('charades', 1)
    (new0, d0), k0 = _prof(lambda: al.update_labels(copy.deepcopy(S['data_old']), S['data_gt'], prop, coff, return_debug=True))
    (new0b, d0b), k0b = _prof(lambda: al.update_labels(copy.deepcopy(S['data_old']), S['data_gt'], prop, coff, return_debug=True,
                                                       acquire_by=None))
    # the default: the launches, keys and results of before
    assert k0 == k0b and sum(k0.values()) == 2 and not any('al_label_gain' in k for k in k0), k0
    assert sorted(d0) == sorted(['order', 'uncert_video', 'observe', 'uncert_frame', 'sprob', 'eprob', 'new_idx', 'gt_idx', 'old_idx', 'updater'])
    assert new0 == new0b and all(np.array_equal(d0[k], d0b[k]) for k in d0 if k != 'updater')
    # by label gain: score, the gain, renew
    (new1, d1), k1 = _prof(lambda: al.update_labels(copy.deepcopy(S['data_old']), S['data_gt'], prop, coff, return_debug=True,
                                                    acquire_by='label_gain'))
    assert sum(k1.values()) == 3 and sum(v for k, v in k1.items() if 'al_label_gain' in k) == 1 and \
        sum(v for k, v in k1.items() if 'al_renew' in k) == 1 and sum(v for k, v in k1.items() if 'al_score' in k) == 1, k1
    assert sorted(d1) == sorted(list(d0) + ['ask_point', 'ask_gain', 'label_value', 'observe_used'])
    for key in ('uncert_video', 'observe', 'gt_idx', 'old_idx'):      # the score and the reference's own frame are untouched
        np.testing.assert_array_equal(d1[key], d0[key])
    np.testing.assert_array_equal(d1['order'], np.argsort(-d1['ask_gain'], kind='stable'))      # largest gain first, ties in sample order
    assert (np.diff(d1['ask_gain'][d1['order']]) <= 0).all()
    sel = d1['order'][:(N + 1) // 2]
    want = np.where(d1['ask_gain'] > 0, d1['ask_point'], d1['observe'])
    np.testing.assert_array_equal(d1['observe_used'], want)
    insel = np.zeros(N, dtype=bool)
    insel[sel] = True
    for i in range(N):                                                # the selected half, each asked once at its frame, answered truthfully
        if insel[i]:
            p = int(want[i])
            is_pos = bool(d1['gt_idx'][i, 0] <= p <= d1['gt_idx'][i, 1])
            assert new1[i][4] == {'pos_idx': [p] if is_pos else [], 'neg_idx': [] if is_pos else [p]}, i
        else:
            assert new1[i][4] == {'pos_idx': [], 'neg_idx': []} and new1[i][2] == S['data_old'][i][2], i
    assert (d1['ask_gain'][sel] > 0).all() and d1['ask_gain'][sel].min() >= d1['ask_gain'][~insel].max()
    assert ((d1['label_value'] > 0) & (d1['label_value'] <= 1)).all() and (d1['ask_gain'] <= 1 - d1['label_value'] + GAIN_BAR).all()
    # the kernel's numbers on the updater's logits, with no answer yet, are the reference's
    up = d1['updater']
    ref = G.set_ref(up._s0.cpu(), up._e0.cpu(), up.vlen_h, up.tlen_h, [[] for _ in range(N)])
    gain = up.gain.cpu().numpy()
    for i in range(N):
        assert ref[i]['status'] == G.LIVE
        assert np.abs(gain[i, :len(ref[i]['gain'])] - ref[i]['gain']).max() <= GAIN_BAR and abs(d1['ask_gain'][i] - ref[i]['ask_gain']) <= GAIN_BAR
        assert abs(d1['label_value'][i] - ref[i]['value']) <= GAIN_BAR
        assert ref[i]['ask_gain'] - ref[i]['gain'][int(d1['ask_point'][i])] <= 2 * GAIN_BAR
    # another question than the frame of most information
    new2, d2 = al.update_labels(copy.deepcopy(S['data_old']), S['data_gt'], prop, coff, return_debug=True, observe_by='info_gain')
    assert (want != d2['observe_used']).any()
    # with the posterior's label: the MBR launch in the renew's place, on the same questions
    (new3, d3), k3 = _prof(lambda: al.update_labels(copy.deepcopy(S['data_old']), S['data_gt'], prop, coff, return_debug=True,
                                                    acquire_by='label_gain', renew_by='posterior'))
    assert sum(k3.values()) == 3 and sum(v for k, v in k3.items() if 'al_label_gain' in k) == 1 and \
        sum(v for k, v in k3.items() if 'al_mbr_label' in k) == 1 and not any('al_renew' in k for k in k3), k3
    for key in ('order', 'ask_point', 'ask_gain', 'label_value', 'observe_used'):
        np.testing.assert_array_equal(d3[key], d1[key])
    assert [r[4] for r in new3] == [r[4] for r in new1] and d3['renewed_by_posterior'][sel].all()
    for i in sel:
        assert new3[i][2] == _time_of(d3['new_idx'][i], int(up.vlen_h[i]), new3[i][1])


def test_a_round_by_label_gain(monkeypatch):
    from hual_amd import al
    S = _round_set.__wrapped__()                                      # a set of its own: the round trains the model and relabels the dataset
    model, ds, N = S['model'], S['ds'], S['N']
    seen = {}
    plain = al.update_labels

    def observed(*args, **kw):
        out, seen['launches'] = _prof(lambda: plain(*args, **kw))
        seen['acquire_by'] = kw.get('acquire_by')
        return out
    monkeypatch.setattr(al, 'update_labels', observed)
    new1, prop1, m1 = al.run_round(model, ds, copy.deepcopy(S['data_old']), S['data_gt'], S['prop'], 'charades', 1, epochs=1, batch_size=16,
                                   lr=1e-3, drop_rate=0.2, acquire_by='label_gain')
    assert seen['acquire_by'] == 'label_gain' and sum(v for k, v in seen['launches'].items() if 'al_label_gain' in k) == 1, seen
    assert len(prop1) == N and m1['train_steps'] == 3 and 0.0 <= m1['miou'] <= 100.0
    assert sum(len(r[4]['pos_idx']) + len(r[4]['neg_idx']) for r in new1) == (N + 1) // 2
    assert sum(r[2] != o[2] for r, o in zip(new1, S['data_old'])) > 0
