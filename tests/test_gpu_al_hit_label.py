"""GPU: hual_al_hit_label (label reliability: the hit probability of pseudo-labels under the answered-point posterior, and per IoU
threshold the member of the consistent set that maximises it) against the float64 enumeration of its contract (tests/al_hit_ref.py),
its edge rows, the memory it must not touch, its agreement with hual_span_hit_prob, determinism and graph capture, the noisy
annotator's rows, and the places it lands: LabelUpdater.hit_label and al.update_labels(rank_by='label_miss' / renew_by='hit_prob').

The bars (from the contract's arithmetic, include/hual_seqpan.h; not tuned):
  cand_hit, best_prob  1e-6 absolute, the project's bar for float64-accumulated probabilities stored as float32: float32 probabilities
                       shared bit for bit with the reference, float64 sums of non-negative terms, prefix differences off by a few
                       2^-53, one final rounding to float32 of a value <= 1 (6e-8).
  the pick             its REFERENCE hit probability within 2e-6 (the bar on either side) of the reference's best - by full
                       enumeration where A holds at most 2,500 spans, else against a field: the picks, the mode, the MBR label and
                       200 random members of A.  Its identity only where the reference's runner-up lies >= 1e-5 below (histories 0
                       and 1 at T in {33, 70}): once answers shrink A exact ties are the rule, and the regret bar covers them.
  hual_span_hit_prob   on rows without active points the spans are equal and the probabilities within one float32 ulp (2^-24): the
                       masses are the same doubles, the divisors two float64 sums of the same terms in different orders."""
import copy

import numpy as np
import pytest
import torch

import al_hit_ref as HL
import al_query_ref as Q
import al_synth
import span_topk_ref as R
from span_clip_util import _pads_intact, _sentinel
from test_gpu_al_query import _prof, make_set, pad_logits

pytestmark = pytest.mark.gpu

BAR, REGRET, GAP, ULP = 1e-6, 2e-6, 1e-5, 2.0 ** -24
FILL, IFILL = 777.0, 777
THR3 = HL.THR3


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def run_hit(dev, s, e, vlen, tlen, aps, thr, cand=None, best=True, sel=None, host_tlen=None):
    """one launch into sentinel-filled outputs -> dict of numpy arrays (None for a part not asked for), after checking the memory
    around them and that exactly the rows of the selected samples inside [0, N) were written"""
    from hual_amd import lib
    N, ld = s.shape
    M = len(thr)
    aset, keep = make_set(dev, vlen, tlen, aps, ld)
    k = 0 if cand is None else int(np.asarray(cand).shape[1])
    bufs = [_sentinel((N, k, M), torch.float32, dev, FILL) if k else None, _sentinel((N, M, 2), torch.int32, dev, IFILL) if best else None,
            _sentinel((N, M), torch.float32, dev, FILL) if best else None]
    out = (bufs[0][0] if k else None, (bufs[1][0], bufs[2][0]) if best else None)
    sel_d = torch.from_numpy(np.asarray(sel, dtype=np.int32)).to(dev) if sel is not None else None
    cand_d = torch.from_numpy(np.ascontiguousarray(cand, dtype=np.int32)).to(dev) if k else None
    got = lib.al_hit_label(aset, s, e, np.asarray(tlen if host_tlen is None else host_tlen), thresholds=thr, sel=sel_d, cand=cand_d, best=best,
                           out=out)
    assert got[0] is out[0] and (got[1] is None) == (not best)
    torch.cuda.synchronize()
    for b, fill in zip(bufs, (FILL, IFILL, FILL)):
        if b is not None:
            assert _pads_intact(b[1], b[2], fill)
    r = dict(cand_hit=out[0].cpu().numpy() if k else None, best_idx=out[1][0].cpu().numpy() if best else None,
             best_prob=out[1][1].cpu().numpy() if best else None)
    written = np.zeros(N, dtype=bool)
    ids = np.arange(N) if sel is None else np.asarray(sel)
    written[ids[(ids >= 0) & (ids < N)]] = True
    for key, fill in (('cand_hit', FILL), ('best_idx', IFILL), ('best_prob', FILL)):      # only the selected rows are written, and all of them
        if r[key] is not None:
            assert (r[key][~written] == fill).all() and not (r[key][written] == fill).any(), key
    return r


def same_bits(a, b):
    return a.shape == b.shape and bool((np.ascontiguousarray(a).view(np.int32) == np.ascontiguousarray(b).view(np.int32)).all())


_CASE = {}


def case(dev, T, h):
    """the shared case al_query_ref.case(T) after h answers on the device (ld = T + 5), its candidates - per row the MBR label
    (hual_al_mbr_label's own), the mode, a random member of A, a random span of the clip (row 0: a slot that is no span) - and the
    launch with k = 4, M = 3 and the search: computed once"""
    if (T, h) not in _CASE:
        from hual_amd import lib
        c = Q.case(T)
        ld = T + 5
        sd, ed = pad_logits(dev, c['s'], ld, 11), pad_logits(dev, c['e'], ld, 12)
        vlen, tlen, aps = c['vlen'].numpy(), [T] * Q.N_ROWS, c['aps'][h]
        aset, keep = make_set(dev, vlen, tlen, aps, ld)
        mbr = lib.al_mbr_label(aset, sd, ed, np.asarray(tlen))[0].cpu().numpy()
        sts = HL.states(T, h)
        cand = np.zeros((Q.N_ROWS, 4, 2), dtype=np.int64)
        for n, st in enumerate(sts):
            cand[n, 0], cand[n, 1] = mbr[n], HL.mode(st)
            cand[n, 2] = HL.random_spans(st, 1, 7000 + 16 * h + n, inside=True)[0]
            cand[n, 3] = HL.random_spans(st, 1, 8000 + 16 * h + n, inside=False)[0]
        cand[0, 3] = (0, int(c['v'][0]))                              # ends beyond the clip: no span
        _CASE[(T, h)] = dict(sd=sd, ed=ed, vlen=vlen, tlen=tlen, aps=aps, cand=cand, sts=sts,
                             got=run_hit(dev, sd, ed, vlen, tlen, aps, THR3, cand=cand))
    return _CASE[(T, h)]


def check_values(sts, cand, r, thr, seed, full=None):
    """every row against the reference -> (max |cand_hit - ref|, max |best_prob - ref of the pick|, max regret of a pick, the picks'
    reference values [N, M])"""
    d_cand = d_best = regret = 0.0
    mine_all = np.zeros((len(sts), len(thr)))
    for n, st in enumerate(sts):
        assert st['status'] == HL.LIVE
        if cand is not None:
            want = HL.cand_prob(st, cand[n], thr)
            flag = want[:, 0] < 0
            assert (r['cand_hit'][n][flag] == -1.0).all() and (r['cand_hit'][n][~flag] >= 0).all() and (r['cand_hit'][n] <= 1).all(), n
            d_cand = max(d_cand, float(np.abs(r['cand_hit'][n].astype(np.float64) - want)[~flag].max(initial=0.0)))
        if r['best_idx'] is None:
            continue
        picks = r['best_idx'][n].astype(np.int64)
        assert all(HL.is_member(st, int(a), int(b)) for a, b in picks), (n, picks)
        mine = np.diag(HL.cand_prob(st, picks, thr))                  # the pick of threshold m at threshold m
        mine_all[n] = mine
        d_best = max(d_best, float(np.abs(r['best_prob'][n].astype(np.float64) - mine).max()))
        if full is not None and full[n] is not None:
            top = full[n]['top']
        else:                                                         # A too large to enumerate pairs: a field of members
            field = np.concatenate([picks, np.array([HL.mode(st)]), cand[n][[HL.is_member(st, int(a), int(b)) for a, b in cand[n]]]
                                    if cand is not None else np.zeros((0, 2), dtype=np.int64), HL.random_spans(st, 200, seed + n, inside=True)])
            top = HL.cand_prob(st, field, thr).max(axis=0)
        regret = max(regret, float((top - mine).max()))
    return d_cand, d_best, regret, mine_all


# ---------------------------------------------------------------------------------------------------------------- 1. values and picks
@pytest.mark.parametrize('h', Q.HISTORIES)
@pytest.mark.parametrize('T', Q.TS)
def test_values_and_picks_against_the_float64_reference(dev, T, h):
    c = case(dev, T, h)
    r, sts = c['got'], c['sts']
    full = HL.full_best(T, h)
    d_cand, d_best, regret, _ = check_values(sts, c['cand'], r, THR3, 9000 + 16 * h, full=full)
    by_enum = sum(f is not None for f in full)
    print('T=%d answers=%d: max |cand_hit - ref| = %.3e, max |best_prob - ref| = %.3e (bar %.0e); max regret of a pick = %.3e (bar %.0e), '
          '%d rows by full enumeration, %d against a field' % (T, h, d_cand, d_best, BAR, regret, REGRET, by_enum, Q.N_ROWS - by_enum))
    assert d_cand <= BAR and d_best <= BAR
    assert regret <= REGRET
    if T <= 70:
        assert by_enum == Q.N_ROWS
    if T in (33, 70) and h in (0, 1):                                 # the identity of the pick, where the reference's runner-up is clear
        close = 0
        for n in range(Q.N_ROWS):
            for m in range(3):
                if full[n]['gap'][m] < GAP:
                    close += 1
                    continue
                q = full[n]['best'][m]
                assert tuple(r['best_idx'][n, m]) == (sts[n]['ii'][q], sts[n]['jj'][q]), (n, m)
        print('  identity: %d of 48 (row, threshold) cases left out as closer than %.0e' % (close, GAP))
        assert close <= 0.05 * 48
    # k = 1 and k = 0: the same bits as the columns of the launch with k = 4; a candidates-only launch too
    a = (c['sd'], c['ed'], c['vlen'], c['tlen'], c['aps'], THR3)
    r1 = run_hit(dev, *a, cand=c['cand'][:, :1])
    r0 = run_hit(dev, *a)
    rc = run_hit(dev, *a, cand=c['cand'], best=False)
    assert r0['cand_hit'] is None and rc['best_idx'] is None and rc['best_prob'] is None
    assert same_bits(r1['cand_hit'], r['cand_hit'][:, :1]) and same_bits(rc['cand_hit'], r['cand_hit'])
    for x in (r1, r0):
        assert same_bits(x['best_idx'], r['best_idx']) and same_bits(x['best_prob'], r['best_prob'])


# ---------------------------------------------------------------------------------------------------------------- 2. other thresholds
@pytest.mark.parametrize('h', [0, 3])
def test_one_threshold_and_four(dev, h):
    T = 70
    c = case(dev, T, h)
    a = (c['sd'], c['ed'], c['vlen'], c['tlen'], c['aps'])
    r = run_hit(dev, *a, [(1, 1)], cand=c['cand'])
    d_cand, d_best, regret, _ = check_values(c['sts'], c['cand'], r, [(1, 1)], 0, full=HL.full_best(T, h, ((1, 1),)))
    for n, st in enumerate(c['sts']):                                 # at 1 / 1 a span hits itself only: the heaviest member, w / Z_A
        q = int(np.argmax(st['w']))
        assert abs(float(r['best_prob'][n, 0]) - st['w'][q] / st['ZA']) <= BAR
    r4 = run_hit(dev, *a, [(1, 1024), (3, 10), 0.5, 0.7], cand=c['cand'])
    thr4 = [(1, 1024)] + THR3
    d4 = check_values(c['sts'], c['cand'], r4, thr4, 0, full=HL.full_best(T, h, tuple(thr4)))
    print('T=70 answers=%d: 1/1 alone: %.3e / %.3e / regret %.3e; four thresholds with 1/1024: %.3e / %.3e / regret %.3e'
          % ((h, d_cand, d_best, regret) + d4[:3]))
    assert max(d_cand, d_best, d4[0], d4[1]) <= BAR and max(regret, d4[2]) <= REGRET
    assert same_bits(r4['cand_hit'][:, :, 1:], c['got']['cand_hit'])  # a column does not depend on its neighbours
    assert same_bits(r4['best_idx'][:, 1:], c['got']['best_idx']) and same_bits(r4['best_prob'][:, 1:], c['got']['best_prob'])
    assert (np.diff(r4['cand_hit'].astype(np.float64), axis=2) <= 1e-7).all()


# ---------------------------------------------------------------------------------------------------------------- 3. hual_span_hit_prob
@pytest.mark.parametrize('T', Q.TS)
def test_no_answers_agrees_with_span_hit_prob(dev, T):
    from hual_amd import lib
    c = Q.case(T)
    k = case(dev, T, 0)
    sd, ed, vd = c['s'].contiguous().to(dev), c['e'].contiguous().to(dev), c['vlen'].to(dev)
    r = run_hit(dev, sd, ed, k['vlen'], k['tlen'], k['aps'], THR3, cand=k['cand'])
    assert same_bits(r['cand_hit'], k['got']['cand_hit']) and same_bits(r['best_idx'], k['got']['best_idx'])      # the row stride changes no bit
    st = torch.from_numpy(k['cand'][:, :, 0].copy()).to(dev)
    en = torch.from_numpy(k['cand'][:, :, 1].copy()).to(dev)
    hp, (bs, be, bp) = lib.span_hit_prob(sd, ed, vd, THR3, starts=st, ends=en, best=True)
    torch.cuda.synchronize()
    assert (r['best_idx'][:, :, 0] == bs.cpu().numpy()).all() and (r['best_idx'][:, :, 1] == be.cpu().numpy()).all()
    d_best = float(np.abs(r['best_prob'].astype(np.float64) - bp.cpu().numpy().astype(np.float64)).max())
    d_cand = float(np.abs(r['cand_hit'].astype(np.float64) - hp.cpu().numpy().astype(np.float64)).max())
    print('T=%d: max |best_prob - span_hit_prob| = %.3e, max |cand_hit - span_hit_prob| = %.3e (one float32 ulp: %.3e)' % (T, d_best, d_cand, ULP))
    assert d_best <= ULP and d_cand <= ULP


# ---------------------------------------------------------------------------------------------------------------- 4. edge rows
def test_edge_rows_are_classified_as_by_the_label_launch(dev):
    """the nine edge rows of tests/test_gpu_span_rows.py: each in the class hual_al_mbr_label puts it in, with the contract's flags"""
    from hual_amd import lib
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
    want = [HL.POISONED] * 3 + [HL.CONTRADICTORY] * 2 + [HL.LIVE] * 4
    sd, ed = pad_logits(dev, s, ld, 5), pad_logits(dev, e, ld, 6)
    host_tlen = np.minimum(tlen, 256)
    aset, keep = make_set(dev, vlen, tlen, aps, ld)
    conf = lib.al_mbr_label(aset, sd, ed, host_tlen)[1].cpu().numpy()
    ref = HL.set_ref(s, e, vlen, tlen, aps)
    assert [x['status'] for x in ref] == want
    cand = np.tile(np.array([[[2, 10], [0, 0], [4, 19], [-1, 3]]]), (N, 1, 1))
    r = run_hit(dev, sd, ed, vlen, tlen, aps, THR3, cand=cand, host_tlen=host_tlen)
    for n in range(N):
        assert (conf[n] == -1.0) == (want[n] != HL.LIVE), n
        if want[n] != HL.LIVE:
            assert (r['cand_hit'][n] == -1.0).all() and (r['best_prob'][n] == -1.0).all() and (r['best_idx'][n] == -1).all(), n
            continue
        wantp = HL.cand_prob(ref[n], cand[n], THR3)
        assert np.abs(r['cand_hit'][n].astype(np.float64) - wantp).max() <= BAR, n
        assert (r['cand_hit'][n, 3] == -1.0).all()
        b = HL.best_ref(ref[n], THR3)
        mine = np.diag(HL.cand_prob(ref[n], r['best_idx'][n], THR3))
        assert np.abs(r['best_prob'][n].astype(np.float64) - mine).max() <= BAR and (b['top'] - mine).max() <= REGRET, n
    assert same_bits(r['cand_hit'][5], r['cand_hit'][6]) and same_bits(r['best_idx'][5], r['best_idx'][6])      # ignored points change no bit
    assert (r['best_idx'][7] == 0).all() and (r['best_prob'][7] == 1.0).all() and (r['cand_hit'][7, 1] == 1.0).all()      # v == 1
    assert (r['cand_hit'][7, 0] == -1.0).all()                        # (2, 10) is no span of a clip of one frame
    # a collapsed posterior is not an error: the best span is that span, with probability 1
    aps2 = [[(11, False), (12, True), (13, False)], []]
    r2 = run_hit(dev, sd[3:5].contiguous(), ed[3:5].contiguous(), [T, T], [T, T], aps2, THR3, cand=np.array([[[12, 12], [11, 13]]] * 2), sel=[0])
    assert (r2['best_idx'][0] == 12).all() and (r2['best_prob'][0] == 1.0).all()
    assert (r2['cand_hit'][0, 0] == 1.0).all() and list(r2['cand_hit'][0, 1]) == [1.0, 0.0, 0.0]      # IoU 1/3 with the one truth
    # a row longer than 256 frames the host knows of: the binding refuses the set before the launch
    aset, keep = make_set(dev, [300, 20], [300, 20], [[], []], 300)
    z = torch.zeros(2, 300, device=dev)
    with pytest.raises(lib.HualError, match='256'):
        lib.al_hit_label(aset, z, z, np.array([300, 20]))


# ---------------------------------------------------------------------------------------------------------------- 5. untouched memory
def test_only_the_selected_rows_are_written(dev):
    T, h = 33, 3
    c = case(dev, T, h)
    a = (c['sd'], c['ed'], c['vlen'], c['tlen'], c['aps'], THR3)
    sel = [13, 2, 7, 0, 12, 4, 9]
    r = run_hit(dev, *a, cand=c['cand'], sel=sel)                      # (run_hit checks the others' fill and the memory around)
    for key in ('cand_hit', 'best_idx', 'best_prob'):
        assert same_bits(r[key][sel], c['got'][key][sel]), key
    # ids outside [0, N) write nothing, anywhere
    r = run_hit(dev, *a, cand=c['cand'], sel=[5, -1, Q.N_ROWS, 11, 2 ** 30, -2 ** 31])
    for key in ('cand_hit', 'best_idx', 'best_prob'):
        assert same_bits(r[key][[5, 11]], c['got'][key][[5, 11]]), key
    r = run_hit(dev, *a, cand=c['cand'][:, :2], best=False, sel=[Q.N_ROWS + 3, 8])
    assert same_bits(r['cand_hit'][8], c['got']['cand_hit'][8, :2])


# ---------------------------------------------------------------------------------------------------------------- 6. determinism
def test_second_launch_and_graph_replay_return_equal_bits(dev):
    from hual_amd import lib
    T, h = 70, 1
    c = case(dev, T, h)
    want = c['got']
    again = run_hit(dev, c['sd'], c['ed'], c['vlen'], c['tlen'], c['aps'], THR3, cand=c['cand'])
    for key in ('cand_hit', 'best_idx', 'best_prob'):
        assert same_bits(again[key], want[key]), key
    aset, keep = make_set(dev, c['vlen'], c['tlen'], c['aps'], T + 5)
    tl = np.asarray(c['tlen'])
    cand_d = torch.from_numpy(c['cand'].astype(np.int32)).to(dev)

    def outs():
        return (torch.full((Q.N_ROWS, 4, 3), FILL, device=dev),
                (torch.full((Q.N_ROWS, 3, 2), IFILL, dtype=torch.int32, device=dev), torch.full((Q.N_ROWS, 3), FILL, device=dev)))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        lib.al_hit_label(aset, c['sd'], c['ed'], tl, cand=cand_d, out=outs())      # (warm-up)
    torch.cuda.current_stream().wait_stream(side)
    out = outs()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        lib.al_hit_label(aset, c['sd'], c['ed'], tl, cand=cand_d, out=out)
    for _ in range(2):
        for o in (out[0],) + out[1]:
            o.fill_(5)
        graph.replay()
        torch.cuda.synchronize()
        for o, key in zip((out[0],) + out[1], ('cand_hit', 'best_idx', 'best_prob')):
            assert same_bits(o.cpu().numpy(), want[key]), key


# ---------------------------------------------------------------------------------------------------------------- 7. the noisy annotator
def _records(s, e, vlen):
    return [{'vid': 'v%d' % n, 'v_len': int(vlen[n]), 'prop_logits': (s[n], e[n]), 'prop_logits1': (s[n], e[n]), 'prop_logits2': (s[n], e[n])}
            for n in range(len(vlen))]


def test_noise_is_the_reference_on_the_tilted_rows(dev):
    """noise=0.1 on rows with 30 % flipped answers: the set without answers and the tilted rows - A is the whole triangle, and no row
    is contradictory"""
    from hual_amd import al
    T = 33
    c = Q.case(T)
    rng = np.random.default_rng(77)
    aps = [[(f, bool(p) != bool(rng.random() < 0.3)) for f, p in a] for a in c['aps'][6]]
    assert sum(p != q for a, b in zip(aps, c['aps'][6]) for (_, p), (_, q) in zip(a, b)) > 5
    up = al.LabelUpdater(_records(c['s'].numpy(), c['e'].numpy(), c['vlen'].numpy()), aps, device=dev)
    sts0 = HL.states(T, 0)
    cand = np.zeros((Q.N_ROWS, 2, 2), dtype=np.int64)
    for n, st in enumerate(sts0):
        cand[n, 0], cand[n, 1] = HL.mode(st), HL.random_spans(st, 1, 600 + n, inside=False)[0]
    up.hit_label(cand=cand, noise=0.1)
    torch.cuda.synchronize()
    assert up.tilt_eps == pytest.approx(0.1)
    ps, pe, v, _ = R.probabilities(up.s_t.cpu(), up.e_t.cpu(), c['vlen'])
    sts = [HL.state(ps[n], pe[n], int(v[n]), []) for n in range(Q.N_ROWS)]
    r = dict(cand_hit=up.cand_hit.cpu().numpy(), best_idx=up.hit_best_idx.cpu().numpy(), best_prob=up.hit_best_prob.cpu().numpy())
    d_cand, d_best, regret, _ = check_values(sts, cand, r, THR3, 0, full=[HL.best_ref(st, THR3) for st in sts])
    print('noise 0.1, 30 %% flipped: max |cand_hit - ref| = %.3e, max |best_prob - ref| = %.3e (bar %.0e); max regret = %.3e (bar %.0e)'
          % (d_cand, d_best, BAR, regret, REGRET))
    assert d_cand <= BAR and d_best <= BAR and regret <= REGRET
    # without noise the same answers are hard constraints: some rows are contradictory, and say so
    up.hit_label(cand=cand)
    hard = HL.set_ref(c['s'], c['e'], c['vlen'].numpy(), [T] * Q.N_ROWS, aps)
    dead = np.array([x['status'] != HL.LIVE for x in hard])
    assert dead.any() and ((up.hit_best_prob.cpu().numpy()[:, 0] == -1.0) == dead).all()
    up.set_ensemble(up._s0[None].contiguous(), up._e0[None].contiguous())
    with pytest.raises(Exception, match='no ensemble form'):
        up.hit_label(cand=cand)


# ---------------------------------------------------------------------------------------------------------------- 8. the round
PARENT_KEYS = ['order', 'uncert_video', 'observe', 'uncert_frame', 'sprob', 'eprob', 'new_idx', 'gt_idx', 'old_idx', 'updater']


def _round_inputs():
    """al_synth.make_trainset(N = 24) with random logits as records, and truthful answers of earlier rounds on every other sample"""
    from hual_amd import al
    N = 24
    recs, vis, data_gt, data_old = al_synth.make_trainset(N, 8, 16, 40, seed=31)
    g = torch.Generator().manual_seed(31)
    rng = np.random.default_rng(31)
    s = [(torch.randn(r['v_len'], generator=g) * 2).numpy() for r in recs]
    e = [(torch.randn(r['v_len'], generator=g) * 2).numpy() for r in recs]
    prop = _records(s, e, [r['v_len'] for r in recs])
    for p, r in zip(prop, recs):
        p['vid'] = r['vid']
    for i, (old, gt, r) in enumerate(zip(data_old, data_gt, recs)):
        pts = {'pos_idx': [], 'neg_idx': []}
        if i % 2 == 0:
            a, b = (al._round_half_even_index(t, gt[1], r['v_len']) for t in gt[2])
            f = int(rng.integers(0, r['v_len']))
            pts['pos_idx' if a <= f <= b else 'neg_idx'].append(f)
        old.append(pts)
    return N, prop, data_gt, data_old


def _aps_of(data):
    return [[(f, True) for f in r[4]['pos_idx']] + [(f, False) for f in r[4]['neg_idx']] for r in data]


def _round_states(up, aps):
    return HL.set_ref(up._s0.cpu(), up._e0.cpu(), up.vlen_h, up.tlen_h, aps)


def test_round_ranks_by_label_miss(dev):
    from hual_amd import al
    N, prop, data_gt, data_old = _round_inputs()
    coff = al.get_coff('charades', 1)
    (new0, d0), k0 = _prof(lambda: al.update_labels(copy.deepcopy(data_old), data_gt, prop, coff, return_debug=True))
    (new1, d1), k1 = _prof(lambda: al.update_labels(copy.deepcopy(data_old), data_gt, prop, coff, return_debug=True, rank_by='label_miss',
                                                    hit_iou=0.5))
    assert sum(k1.values()) == sum(k0.values()) + 1 and sum(v for k, v in k1.items() if 'al_hit_label' in k) == 1, k1
    assert sorted(d1) == sorted(PARENT_KEYS + ['label_miss', 'old_hit'])
    np.testing.assert_array_equal(d1['old_idx'], d0['old_idx'])
    sts = _round_states(d1['updater'], _aps_of(data_old))            # on the answers of the earlier rounds
    want = np.stack([HL.cand_prob(st, [d1['old_idx'][n]], THR3)[0] for n, st in enumerate(sts)])
    assert d1['old_hit'].shape == (N, 3) and d1['label_miss'].dtype == np.float32
    assert np.abs(d1['old_hit'].astype(np.float64) - want).max() <= BAR
    miss = np.where(want[:, 1] < 0, -1.0, 1.0 - want[:, 1])
    d = float(np.abs(d1['label_miss'].astype(np.float64) - miss).max())
    print('label_miss at 0.5: max |label_miss - ref| = %.3e (bar %.0e); range %.3f .. %.3f' % (d, BAR, d1['label_miss'].min(), d1['label_miss'].max()))
    assert d <= BAR
    np.testing.assert_array_equal(d1['order'], np.argsort(-d1['label_miss'], kind='stable'))
    assert not np.array_equal(d1['order'], d0['order'])
    sel = d1['order'][:(N + 1) // 2]
    assert sorted(i for i in range(N) if len(_aps_of(new1)[i]) > len(_aps_of(data_old)[i])) == sorted(sel.tolist())      # the same half is asked


def test_round_renews_by_hit_probability(dev):
    from hual_amd import al
    N, prop, data_gt, data_old = _round_inputs()
    hand = [i for i in range(N) if i % 4 == 1]                        # contradictory answers made by hand: no label from the posterior
    for i in hand:
        data_old[i][4] = {'pos_idx': [2, 8], 'neg_idx': [5]}
    coff = al.get_coff('charades', 1)
    (new_h, d_h), k_h = _prof(lambda: al.update_labels(copy.deepcopy(data_old), data_gt, prop, coff, return_debug=True))
    (new_p, d_p), k_p = _prof(lambda: al.update_labels(copy.deepcopy(data_old), data_gt, prop, coff, return_debug=True, renew_by='posterior'))
    (new1, d1), k1 = _prof(lambda: al.update_labels(copy.deepcopy(data_old), data_gt, prop, coff, return_debug=True, renew_by='hit_prob'))
    assert sum(k1.values()) == sum(k_p.values()) + 1 and sum(v for k, v in k1.items() if 'al_hit_label' in k) == 1, k1
    assert sorted(d1) == sorted(list(d_p) + ['old_hit', 'label_hit', 'hit_best_idx', 'hit_best_prob', 'renewed_by_hit'])
    for key in ('order', 'old_idx', 'label_conf', 'old_conf', 'renewed_by_posterior'):
        np.testing.assert_array_equal(d1[key], d_p[key])
    sel = d1['order'][:(N + 1) // 2]
    insel = np.zeros(N, dtype=bool)
    insel[sel] = True
    dead = [int(i) for i in sel if i in hand]
    assert dead and len(dead) < len(sel)
    c = 2                                                             # hit_iou = 0.7, the default
    mbr = d_p['new_idx']                                              # the MBR label, with the reference's renew where there is none
    move = d1['renewed_by_posterior'] & (d1['hit_best_prob'][:, c].astype(np.float64) - d1['label_hit'][:, c].astype(np.float64) > 1e-6)
    np.testing.assert_array_equal(d1['renewed_by_hit'], move)
    assert not move[~insel].any() and not move[dead].any()
    np.testing.assert_array_equal(d1['new_idx'], np.where(move[:, None], d1['hit_best_idx'][:, c], mbr))
    for i in dead:                                                    # rows without a label: the reference's renew
        np.testing.assert_array_equal(d1['new_idx'][i], d_h['new_idx'][i])
        assert (d1['label_hit'][i] == -1.0).all() and (d1['hit_best_prob'][i] == -1.0).all() and new1[i][2] == new_h[i][2]
    assert (d1['label_hit'][~insel] == -1.0).all() and (d1['hit_best_idx'][~insel] == -1).all()
    # the values against the reference, on this round's answers
    sts = _round_states(d1['updater'], _aps_of(new1))
    worst = 0.0
    for i in sel:
        if int(i) in dead:
            continue
        want = HL.cand_prob(sts[i], [d1['old_idx'][i], mbr[i]], THR3)
        worst = max(worst, float(np.abs(np.stack([d1['old_hit'][i], d1['label_hit'][i]]).astype(np.float64) - want).max()))
        b = HL.best_ref(sts[i], THR3)
        mine = np.diag(HL.cand_prob(sts[i], d1['hit_best_idx'][i], THR3))
        assert (b['top'] - mine).max() <= REGRET and np.abs(d1['hit_best_prob'][i].astype(np.float64) - mine).max() <= BAR, i
        vl, dur = int(d1['updater'].vlen_h[i]), new1[i][1]
        assert new1[i][2] == [round(int(t) / (vl - 1) * dur, 2) for t in d1['new_idx'][i]]
    print('renew by hit probability at 0.7: %d of %d selected labels moved off the MBR label; max |old_hit, label_hit - ref| = %.3e (bar %.0e)'
          % (int(move.sum()), len(sel), worst, BAR))
    assert worst <= BAR
    # both switches on: the ranking's label_miss, the renew's old_hit
    new2, d2 = al.update_labels(copy.deepcopy(data_old), data_gt, prop, coff, return_debug=True, rank_by='label_miss', renew_by='hit_prob',
                                hit_iou=0.3)
    assert 'label_miss' in d2 and (d2['old_hit'][~np.isin(np.arange(N), d2['order'][:(N + 1) // 2])] == -1.0).all()


def test_round_with_both_switches_off_is_the_parents(dev):
    from hual_amd import al
    N, prop, data_gt, data_old = _round_inputs()
    coff = al.get_coff('charades', 1)
    for extra in ({}, dict(renew_by='posterior'), dict(observe_by='info_gain')):
        (new0, d0), k0 = _prof(lambda: al.update_labels(copy.deepcopy(data_old), data_gt, prop, coff, return_debug=True, **extra))
        (new1, d1), k1 = _prof(lambda: al.update_labels(copy.deepcopy(data_old), data_gt, prop, coff, return_debug=True, rank_by='uncert_video',
                                                        hit_iou=0.3, **dict(dict(renew_by='heuristic'), **extra)))
        assert k0 == k1 and not any('al_hit_label' in k for k in k0), (k0, k1)
        assert new0 == new1 and list(d0) == list(d1)
        assert all(np.array_equal(d0[k], d1[k]) for k in d0 if k != 'updater')
        if not extra:
            assert sorted(d0) == sorted(PARENT_KEYS) and sum(k0.values()) == 2
