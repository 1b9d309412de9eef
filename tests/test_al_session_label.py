"""CPU: the float64 reference of hual_al_session_label (tests/al_session_label_ref.py) against al_session_ref with the rule off, its
own rules (every stop reason, a reliable stop only ever comes earlier, the final slot), the share of passes too close to a threshold
or a tie for the GPU test to compare, the argument checks of the entry point and of the binding that come before any HIP call, and
the rules of al.check_round / al.update_labels(stop_hit=) that come before any device is touched."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import al_query_ref as Q
import al_session_label_ref as SL
import al_session_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRANSCRIPT = ('asked', 'answer', 'q_asked', 'gain', 'entropy', 'n_asked', 'stop_reason', 'aps')


# ---------------------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize('T', [2, 33, 70])
def test_with_the_rule_off_the_reference_is_the_session_reference(T):
    for start, eps, flipped in SL.SETTINGS:
        for stop_entropy, min_gain in ((-1.0, 0.0), (S.STOP_ENTROPY, S.MIN_GAIN)):
            got = SL.sessions(T, start, eps, flipped, 6, -1.0, 0, stop_entropy, min_gain)
            want = S.sessions(T, start, eps, flipped, 6, stop_entropy, min_gain)
            for g, w in zip(got, want):
                for k in TRANSCRIPT:
                    assert g[k] == w[k], (start, eps, flipped, k)
                assert SL.RELIABLE != g['stop_reason']
                assert len(g['label']) == len(g['label_conf']) == len(g['label_hit']) == g['n_asked'] + 1


def test_every_stop_reason_is_reached():
    seen = set()
    c = Q.case(33)
    stop_hit, stop_m = SL.RULES[0]
    for T in (2, 33, 70):
        for start in S.STARTS:
            for eps, flipped in ((0.0, False), (0.0, True), (0.05, True)):
                for x in SL.sessions(T, start, eps, flipped, 6, stop_hit, stop_m) + SL.sessions(T, start, eps, flipped, 6, stop_hit, stop_m, 1.0, 0.0):
                    seen.add(x['stop_reason'])
                    if x['stop_reason'] == SL.RELIABLE:               # the pass that stopped it holds the label that is reliable
                        assert x['label_hit'][-1][stop_m] >= stop_hit and all(h[stop_m] < stop_hit for h in x['label_hit'][:-1])
                        assert x['label'][-1][0] >= 0 and 0.0 <= x['label_conf'][-1] <= 1.0
                    if x['stop_reason'] == S.CONTRADICTORY:
                        assert x['label'][-1] == (-1, -1) and x['label_conf'][-1] == -1.0 and (x['label_hit'][-1] == -1.0).all()
    # the gain's rule behind the new one: a best gain of at most 0.9 bits stops a session whose label is not yet reliable
    slow = [x for x in SL.sessions(33, 0, 0.0, False, 6, stop_hit, stop_m, -1.0, 0.9) if x['stop_reason'] == S.GAIN]
    assert slow and all(x['label_hit'][-1][stop_m] < stop_hit and x['posts'][-1]['query_gain'] <= 0.9 for x in slow)
    seen.add(S.GAIN)
    assert {S.BUDGET, S.ENTROPY, S.GAIN, S.CONTRADICTORY, SL.RELIABLE} <= seen
    s, e = c['s'][0].numpy(), c['e'][0].numpy()
    dead = SL.session(s, e, 33, [], c['gt'][0], 6, stop_hit=stop_hit, stop_m=stop_m, nan_logit=True)
    assert dead['stop_reason'] == S.POISONED and dead['label'] == [(-1, -1)]
    full = [(0, False)] * 60
    over = SL.session(s, e, 33, full, c['gt'][0], 6, stop_hit=stop_hit, stop_m=stop_m)
    assert over['stop_reason'] == S.OVERFLOW and over['label'] == []
    # one frame: the label is that frame, it certainly hits, and the rule comes before the gain's
    assert int(c['v'][8]) == 1
    one = SL.sessions(33, 0, 0.0, False, 6, stop_hit, stop_m)[8]
    assert one['stop_reason'] == SL.RELIABLE and one['label'] == [(0, 0)] and one['label_conf'] == [1.0] and (one['label_hit'][0] == 1.0).all()
    assert SL.sessions(33, 0, 0.0, False, 6)[8]['stop_reason'] == S.GAIN


@pytest.mark.parametrize('T', [2, 33, 70])
def test_a_reliable_stop_only_comes_earlier(T):
    """the rule reads, it does not steer: a session under it is a prefix of the same session without it"""
    fewer = 0
    for start, eps, flipped in SL.SETTINGS:
        for stop_hit, stop_m in SL.RULES:
            for x, y in zip(SL.sessions(T, start, eps, flipped, 6, stop_hit, stop_m), SL.sessions(T, start, eps, flipped, 6)):
                assert x['n_asked'] <= y['n_asked']
                assert x['asked'] == y['asked'][:x['n_asked']] and x['answer'] == y['answer'][:x['n_asked']]
                assert x['label'] == y['label'][:x['n_asked'] + 1]
                if x['stop_reason'] != SL.RELIABLE:
                    assert (x['n_asked'], x['stop_reason']) == (y['n_asked'], y['stop_reason'])
                fewer += x['n_asked'] < y['n_asked']
    assert fewer > 0


def test_the_questions_asked_table():
    """the figures the documents quote (scripts/al_session_label_clicks.py prints them): Q = 6, 0.9 at 7/10, the hard rule"""
    stop_hit, stop_m = SL.RULES[0]
    table = {}
    for T, start in ((33, 0), (33, 3), (70, 0), (70, 3), (2, 0)):
        r = SL.sessions(T, start, 0.0, False, 6, stop_hit, stop_m)
        table[(T, start)] = (sum(x['stop_reason'] == SL.RELIABLE for x in r), sum(x['stop_reason'] == S.BUDGET for x in r),
                             sum(x['n_asked'] for x in r))
    assert table == {(33, 0): (8, 8, 74), (33, 3): (10, 6, 53), (70, 0): (5, 11, 86), (70, 3): (10, 6, 64), (2, 0): (16, 0, 8)}


@pytest.mark.parametrize('T', [33, 70])
def test_few_passes_lie_near_a_threshold_or_a_tie(T):
    """what the teacher-forced GPU comparison skips, on the reference alone: per setting at most 5 % of the passes within 1e-3 of
    stop_hit (or of the thresholds in bits), and no label whose runner-up lies within 1e-5"""
    for start, eps, flipped in SL.SETTINGS:
        for stop_hit, stop_m in SL.RULES:
            near = total = 0
            worst = np.inf
            for r in SL.sessions(T, start, eps, flipped, 6, stop_hit, stop_m):
                for p in r['passes']:
                    if p['post']['status'] != Q.LIVE:
                        continue
                    total += 1
                    near += SL.near_threshold(p, stop_hit, stop_m)
                    worst = min(worst, p['label']['margin'])
            print('T=%d start=%s eps=%g rule %.2f@%d/%d: %d of %d live passes near a threshold, smallest label margin %.3e'
                  % (T, start, eps, stop_hit, *SL.THR[stop_m], near, total, worst))
            assert total >= 50 and near <= 0.05 * total
            assert worst >= SL.MARGIN


# ---------------------------------------------------------------------------------------------------------------- the entry point
def test_symbol_is_declared_and_exported_at_abi_9():
    from hual_amd import build, lib
    build.build()
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'hual_seqpan.h')).read(), flags=re.S)
    assert re.search(r'\bint hual_al_session_label\s*\(', src) and re.search(r'#define HUAL_AL_STOP_RELIABLE 6\b', src)
    assert hasattr(ctypes.CDLL(lib.LIB_PATH), 'hual_al_session_label'), 'missing export hual_al_session_label'
    assert lib.load().hual_abi_version() == lib.ABI_VERSION == 9          # a new symbol, the ABI version stays
    assert lib.AL_STOP_REASONS == ('budget', 'entropy', 'gain', 'contradictory', 'poisoned', 'overflow', 'reliable')
    assert lib.AL_STOP_REASONS.index('reliable') == SL.RELIABLE and callable(lib.al_session_label)


def test_entry_point_refuses_bad_arguments_without_a_gpu():
    """every bad argument returns before any HIP call (the device pointers below are never dereferenced; the thresholds are host memory)"""
    from hual_amd import lib
    l = lib.load()
    buf = ctypes.create_string_buffer(64)
    a = ctypes.addressof(buf)
    p = ctypes.c_void_p(a)
    SET = ('vlen', 'tlen', 'ap_off', 'ap_idx', 'ap_pos')
    OUT = ('asked', 'answer', 'q_asked', 'gain', 'entropy', 'n_asked', 'stop_reason', 'label', 'label_conf', 'label_hit')

    def aset(N=4, ld=64, **null):
        f = {k: a for k in SET}
        f.update(null)
        return ctypes.byref(lib.hual_al_set(N, ld, *[f[k] for k in SET]))

    def thr_of(pairs):
        return (ctypes.c_int32 * (2 * len(pairs)))(*[x for nd in pairs for x in nd])

    def call(s=None, s0=p, e0=p, gt=p, sel=p, nsel=2, qmax=6, stop_entropy=-1.0, min_gain=0.0, eps=0.0, thr=thr_of(SL.THR), M=3, stop_m=2,
             stop_hit=0.9, drop=None, _null_set=False):
        outs = [None if k == drop else p for k in OUT]
        return l.hual_al_session_label(None if _null_set else (s or aset()), s0, e0, gt, sel, nsel, qmax, None, stop_entropy, min_gain, eps,
                                       None, thr, M, stop_m, stop_hit, *outs, None)
    cases = [(dict(_null_set=True), b'null pointer'), (dict(thr=None), b'null pointer'), (dict(s0=None), b'null input'),
             (dict(e0=None), b'null input'), (dict(gt=None), b'null gt'), (dict(nsel=0), b'nsel >= 1'), (dict(nsel=-3), b'nsel >= 1'),
             (dict(qmax=0), b'qmax in [1, 16]'), (dict(qmax=17), b'qmax in [1, 16]'), (dict(min_gain=-0.5), b'min_gain >= 0'),
             (dict(min_gain=float('nan')), b'min_gain >= 0'), (dict(eps=0.51), b'eps is 0'), (dict(eps=-0.1), b'eps is 0'),
             (dict(eps=float('nan')), b'eps is 0'), (dict(M=0), b'M <= 4'), (dict(M=5), b'M <= 4'), (dict(stop_m=-1), b'stop_m in [0, M)'),
             (dict(stop_m=3), b'stop_m in [0, M)'), (dict(M=2, stop_m=2), b'stop_m in [0, M)'), (dict(stop_hit=0.0), b'stop_hit'),
             (dict(stop_hit=1.5), b'stop_hit'), (dict(stop_hit=float('nan')), b'stop_hit'),
             (dict(thr=thr_of([(3, 10), (0, 2), (7, 10)])), b'num <= den'), (dict(thr=thr_of([(3, 10), (3, 2), (7, 10)])), b'num <= den'),
             (dict(thr=thr_of([(3, 10), (1, 2), (1, 1025)])), b'num <= den'),
             (dict(s=aset(N=0)), b'N > 0'), (dict(s=aset(ld=1)), b'2 <= ld'), (dict(s=aset(ld=1025)), b'ld <= 1024')]
    cases += [(dict(s=aset(**{k: None})), b'null input') for k in SET]
    cases += [(dict(drop=k), b'null output') for k in OUT]
    for kw, msg in cases:
        rc = call(**kw)
        assert rc == -1 and msg in l.hual_last_error() and b'al_session_label' in l.hual_last_error(), (kw, msg, rc, l.hual_last_error())
    with pytest.raises(lib.HualError, match='stop_m'):
        lib.check(call(stop_m=7))


def test_binding_refuses_bad_arguments_without_a_gpu():
    """every argument fault is a HualError before the library is called: the set below holds pointers nothing may follow"""
    from hual_amd import lib
    N, ld, Qn = 3, 8, 4
    aset = lib.hual_al_set(N, ld, 8, 8, 8, 8, 8)
    s = torch.zeros(N, ld)
    tl = np.full(N, ld)
    gt = torch.zeros(N, 2, dtype=torch.int32)
    sel = torch.zeros(2, dtype=torch.int32)
    i32, i8 = dict(dtype=torch.int32), dict(dtype=torch.int8)
    good = (torch.zeros(N, Qn, **i32), torch.zeros(N, Qn, **i8), torch.zeros(N, Qn), torch.zeros(N, Qn), torch.zeros(N, Qn + 1),
            torch.zeros(N, **i32), torch.zeros(N, **i32), torch.zeros(N, Qn + 1, 2, **i32), torch.zeros(N, Qn + 1), torch.zeros(N, Qn + 1, 3))

    def swap(i, t):
        return good[:i] + (t,) + good[i + 1:]
    for args, kw, msg in (((aset, s.double(), s, tl, gt, Qn), {}, 's0 / e0 must be'), ((aset, s, s[:, :4], tl, gt, Qn), {}, 's0 / e0 must be'),
                          ((aset, s, s, tl[:2], gt, Qn), {}, 'N = 3 row lengths'), ((aset, s, s, np.full(N, 300), gt, Qn), {}, '256'),
                          ((aset, s, s, tl, gt, 0), {}, 'qmax must lie'), ((aset, s, s, tl, gt, 17), {}, 'qmax must lie'),
                          ((aset, s, s, tl, None, Qn), {}, 'gt'), ((aset, s, s, tl, gt.long(), Qn), {}, 'gt'),
                          ((aset, s, s, tl, gt[:2], Qn), {}, 'gt'),
                          ((aset, s, s, tl, gt, Qn), dict(thresholds=(0.3001234567,)), 'denominator'),
                          ((aset, s, s, tl, gt, Qn), dict(thresholds=()), '1 to 4'),
                          ((aset, s, s, tl, gt, Qn), dict(thresholds=(0.1, 0.3, 0.5, 0.7, 0.9)), '1 to 4'),
                          ((aset, s, s, tl, gt, Qn), dict(stop_m=3), 'stop_m'), ((aset, s, s, tl, gt, Qn), dict(stop_m=-1), 'stop_m'),
                          ((aset, s, s, tl, gt, Qn), dict(stop_m=1.5), 'stop_m'), ((aset, s, s, tl, gt, Qn), dict(stop_m=True), 'stop_m'),
                          ((aset, s, s, tl, gt, Qn), dict(thresholds=(0.5,), stop_m=1), 'stop_m'),
                          ((aset, s, s, tl, gt, Qn), dict(stop_hit=0.0), 'stop_hit'), ((aset, s, s, tl, gt, Qn), dict(stop_hit=1.01), 'stop_hit'),
                          ((aset, s, s, tl, gt, Qn), dict(stop_hit=float('nan')), 'stop_hit'),
                          ((aset, s, s, tl, gt, Qn), dict(sel=sel.long()), 'sel must be'), ((aset, s, s, tl, gt, Qn), dict(sel=sel[:0]), 'sel must be'),
                          ((aset, s, s, tl, gt, Qn), dict(budget=torch.zeros(N)), 'budget'),
                          ((aset, s, s, tl, gt, Qn), dict(budget=torch.zeros(N + 1, **i32)), 'budget'),
                          ((aset, s, s, tl, gt, Qn), dict(flip=torch.zeros(N, 2, **i32)), 'flip'),
                          ((aset, s, s, tl, gt, Qn), dict(out=good[:7]), 'out is'),
                          ((aset, s, s, tl, gt, Qn), dict(out=swap(7, None)), 'out is'),
                          ((aset, s, s, tl, gt, Qn), dict(out=swap(7, torch.zeros(N, Qn, 2, **i32))), 'label must be'),
                          ((aset, s, s, tl, gt, Qn), dict(out=swap(7, torch.zeros(N, Qn + 1, 2))), 'label must be'),
                          ((aset, s, s, tl, gt, Qn), dict(out=swap(8, torch.zeros(N, Qn))), 'label_conf must be'),
                          ((aset, s, s, tl, gt, Qn), dict(out=swap(9, torch.zeros(N, Qn + 1, 4))), 'label_hit must be'),
                          ((aset, s, s, tl, gt, Qn), dict(thresholds=(0.5, 0.7), out=good), 'label_hit must be'),
                          ((aset, s, s, tl, gt, Qn), dict(out=swap(4, torch.zeros(N, Qn))), 'entropy must be')):
        with pytest.raises(lib.HualError, match=msg):
            lib.al_session_label(*args, **kw)


# ---------------------------------------------------------------------------------------------------------------- the round
def test_check_round_on_stop_hit():
    from hual_amd import al
    base = al.check_round()
    assert base.stop_hit is None and al.RoundPolicy._fields[-1] == 'hit_iou'
    assert tuple(base) == ('deterministic', 'uncert_video', 'uncert_frame', 'heuristic', None, 1, None, None, None, None, None, False, 1, 0.7)
    sessions = dict(observe_by='info_gain', questions_per_clip=3)
    for extra in ({}, dict(stop_entropy=1.0), dict(answer_noise=0.1), dict(renew_by='posterior'), dict(hit_iou=0.5)):
        off, on = al.check_round(**sessions, **extra), al.check_round(stop_hit=0.9, **sessions, **extra)
        assert off.stop_hit is None and al.check_round(stop_hit=None, **sessions, **extra).stop_hit is None
        assert tuple(on) == tuple(off) and on.stop_hit == 0.9 and on.hit_iou == extra.get('hit_iou', 0.7)
    assert al.check_round(stop_hit=1, **sessions).stop_hit == 1.0
    for kw in (dict(stop_hit=0.9), dict(stop_hit=0.9, observe_by='info_gain'), dict(stop_hit=0.9, observe_by='info_gain', questions_per_clip=1),
               dict(stop_hit=0.9, observe_by='info_gain', questions_at_once=3)):
        with pytest.raises(ValueError, match='stop_hit'):                  # no sessions: nothing to stop
            al.check_round(**kw)
    for bad in (0.0, -0.5, 1.01, float('nan'), True, 'high', (0.9,)):
        with pytest.raises(ValueError, match='stop_hit'):
            al.check_round(stop_hit=bad, **sessions)
    with pytest.raises(ValueError, match='no ensemble form'):

        class _Bank:
            K = Kmax = 3
            pass_s = object()
        al.check_round(posterior='ensemble', bank=_Bank(), stop_hit=0.9, **sessions)


def test_update_labels_refuses_before_touching_a_device(monkeypatch):
    from hual_amd import al

    def boom(*a, **k):
        raise AssertionError('a device was touched')
    monkeypatch.setattr(al.LabelUpdater, '__init__', boom)
    monkeypatch.setattr(al.LabelUpdater, 'from_bank', boom)
    args = ([['v0', 1.0, [0.0, 1.0], 'a']], [['v0', 1.0, [0.0, 1.0], 'a']], [{'vid': 'v0'}], al.get_coff('charades', 1))
    for kw in (dict(stop_hit=0.9), dict(stop_hit=0.9, observe_by='info_gain'), dict(stop_hit=0.0, observe_by='info_gain', questions_per_clip=3),
               dict(stop_hit=1.5, observe_by='info_gain', questions_per_clip=3)):
        with pytest.raises(ValueError, match='stop_hit'):
            al.update_labels(*args, **kw)
    with pytest.raises(AssertionError, match='a device was touched'):      # (the accepted form gets as far as the device)
        al.update_labels(*args, stop_hit=0.9, observe_by='info_gain', questions_per_clip=3)
