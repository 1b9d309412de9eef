"""CPU: core-set clip selection (hual_kcenter_greedy, hual_clip_mean_features) is declared, exported and bound; its float64 reference
(tests/kcenter_ref.py) on a hand-worked example and against a brute-force optimum; argument errors of the C entry points and the
wrappers without a GPU; check_round's new rules and the unchanged RoundPolicy tuple of a round without the new switches."""
import ctypes
import os
import re

import numpy as np
import pytest

import kcenter_ref as KR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_exported_and_the_abi_version_stays():
    from hual_amd import lib
    src = open(os.path.join(ROOT, 'include', 'hual_seqpan.h')).read()
    for name in ('hual_kcenter_greedy', 'hual_kcenter_workspace_bytes', 'hual_clip_mean_features'):
        assert re.search(r'\b%s\s*\(' % name, src)
        assert hasattr(ctypes.CDLL(lib.LIB_PATH), name), 'missing export ' + name
    assert lib.load().hual_abi_version() == lib.ABI_VERSION == 9          # new symbols, the ABI version stays
    assert callable(lib.kcenter_select) and callable(lib.clip_mean_features)
    # the workspace: the counter words, one flag per row, one 16-byte partial per workgroup of 16 rows
    assert lib.kcenter_workspace_bytes(1) == 16 + 16 + 16 and lib.kcenter_workspace_bytes(1031) == 16 + 4128 + 16 * 65
    assert lib.kcenter_workspace_bytes(0) == 0


def test_reference_on_a_hand_worked_example():
    """six points on a line.  Rows 0 / 1 and 2 / 3 are duplicates (unequal and equal weights), row 5 has weight 0.
       step 0, no center: score = w, rows 1 and 4 tie at (1, 1): the lower index, 1; pick_dist +inf
       center 1 (x = 0): mind = 0 0 100 100 16 36, score = 0 - 50 50 16 0: rows 2 and 3 tie in score and weight: 2; pick_dist 100
       center 2 (x = 10): mind = 0 0 0 0 16 16, score = 0 - - 0 16 0: row 4; pick_dist 16
       center 4 (x = 4): mind = 0 0 0 0 0 4, every score 0: the larger weight decides - rows 0 and 3 at 0.5 over row 5 at 0 -, then
       the lower index: 0, then 3, then 5 (pick_dist 0, 0, 4)"""
    x = np.array([[0.0], [0.0], [10.0], [10.0], [4.0], [6.0]])
    w = np.array([0.5, 1.0, 0.5, 0.5, 1.0, 0.0])
    r = KR.greedy(x, 6, w, snapshots=(3,))
    assert r['picked'].tolist() == [1, 2, 4, 0, 3, 5]
    assert r['pick_dist'].tolist() == [np.inf, 100.0, 16.0, 0.0, 0.0, 4.0]
    assert r['state'][3][0].tolist() == [0, 0, 0, 0, 0, 4] and r['state'][3][1].tolist() == [1, 1, 2, 2, 4, 4]
    assert r['mind'].tolist() == [0] * 6 and r['assign'].tolist() == [1, 1, 2, 2, 4, 5]      # a tie at 0 keeps the first center
    # teacher forcing: the scores the next step sees after a given prefix
    st = KR.State(x, w)
    st.add(1)
    score, eligible = st.scores()
    assert score.tolist() == [0, 0, 50, 50, 16, 0] and eligible.tolist() == [True, False, True, True, True, True]
    # init rows are centers and never picked; a negative or NaN weight is never asked; a NaN row neither
    r = KR.greedy(x, 6, np.array([0.5, 1.0, -1.0, np.nan, 1.0, 0.0]), init=[4])
    assert r['picked'].tolist() == [1, 0, 5, -1, -1, -1] and r['pick_dist'].tolist() == [16.0, 0.0, 4.0, -1.0, -1.0, -1.0]
    xn = x.copy()
    xn[2] = np.nan
    r2 = KR.greedy(xn, 6, w)
    assert 2 not in r2['picked'] and r2['picked'][:2].tolist() == [1, 3] and np.isnan(r2['mind'][2]) and r2['picked'][-1] == -1
    assert KR.greedy(x, 3, None)['picked'].tolist() == [0, 2, 4]          # no weights: started at row 0


def test_unweighted_greedy_is_a_2_approximation():
    """Gonzalez: the covering radius of greedy k-center is at most twice the optimum's, on the distances (sqrt of mind)"""
    for seed in range(20):
        x = np.random.default_rng(seed).standard_normal((8, 2))
        r = KR.greedy(x, 3)
        radius = float(np.sqrt(r['mind'].max()))
        assert radius == pytest.approx(KR.cover_radius(x, r['picked']), rel=1e-12)
        opt = KR.optimal_radius(x, 3)
        assert opt <= radius <= 2.0 * opt * (1 + 1e-12), (seed, radius, opt)


def test_bad_arguments_fail_loudly_without_a_gpu():
    import torch
    from hual_amd import lib
    l = lib.load()
    one = ctypes.c_void_p(16)                                             # never dereferenced: every call below fails before any HIP call

    def kc(x=one, N=8, D=4, ld=4, w=None, init=None, n_init=0, n_select=2, out=one, ws=one, ws_bytes=1 << 20):
        return l.hual_kcenter_greedy(x, N, D, ld, w, init, n_init, n_select, out, out, out, out, ws, ws_bytes, None)

    for kw, msg in ((dict(N=0), b'N >= 1'), (dict(D=0), b'1 <= D <= 4096'), (dict(D=4097, ld=4097), b'1 <= D <= 4096'), (dict(ld=3), b'ld >= D'),
                    (dict(n_select=9), b'0 <= n_select <= N'), (dict(n_select=-1), b'0 <= n_select <= N'), (dict(n_init=9), b'0 <= n_init <= N'),
                    (dict(n_init=1), b'null pointer (init'), (dict(x=None), b'null pointer'), (dict(out=None), b'null pointer'),
                    (dict(ws=None), b'null pointer'), (dict(ws_bytes=16), b'workspace smaller'), (dict(ws=ctypes.c_void_p(8)), b'16-byte aligned')):
        rc = kc(**kw)
        assert rc == -1 and msg in l.hual_last_error() and b'hual_kcenter_greedy' in l.hual_last_error(), (kw, rc, l.hual_last_error())
    assert kc(n_select=0, x=None, out=None, ws=None) == 0                 # nothing owed: nothing launched, nothing read
    for args, msg in (((None, one, 2, 8, 1, one, 8), b'null pointer'), ((one, one, 0, 8, 1, one, 8), b'V >= 1'),
                      ((one, one, 2, 4097, 1, one, 4097), b'1 <= vdim <= 4096'), ((one, one, 2, 8, 1, one, 7), b'ld_out >= vdim')):
        rc = l.hual_clip_mean_features(*args, None)
        assert rc == -1 and msg in l.hual_last_error() and b'hual_clip_mean_features' in l.hual_last_error(), (args, l.hual_last_error())
    # the wrapper's own gates come before any launch too
    x = torch.zeros(4, 3)
    for kw, exc in ((dict(n_select=5), ValueError), (dict(n_select=-1), ValueError), (dict(n_select=2, init=[4]), ValueError),
                    (dict(n_select=2, init=[-1]), ValueError), (dict(n_select=2, init=[1, 1]), ValueError),
                    (dict(n_select=2, init=[[1]]), ValueError), (dict(n_select=2, weight=torch.zeros(3)), lib.HualError),
                    (dict(n_select=2, out=(None,) * 3), lib.HualError)):
        with pytest.raises(exc):
            lib.kcenter_select(x, **kw)
    for bad in (torch.zeros(4, 3, dtype=torch.float64), torch.zeros(4), torch.zeros(4, 4097), torch.zeros(4, 6)[:, ::2]):
        with pytest.raises(lib.HualError):
            lib.kcenter_select(bad, 1)
    with pytest.raises(lib.HualError):
        lib.clip_mean_features(torch.zeros(4, 3), torch.zeros(3, dtype=torch.int32))


def test_rank_weights():
    from hual_amd import al
    w = al.rank_weights(np.array([2, 0, 3, 1]))
    assert w.dtype == np.float32 and w.tolist() == [0.75, 0.25, 1.0, 0.5]
    w = al.rank_weights(np.arange(12403)[::-1])
    assert w[-1] == 1.0 and w[0] == np.float32(1.0 / 12403) and (np.diff(w) > 0).all()
    with pytest.raises(ValueError):
        al.rank_weights([0, 0, 1])


def test_check_round_knows_the_selection_switches():
    import torch
    from hual_amd import al
    desc = torch.zeros(6, 8)
    for kw, msg in ((dict(select_by='coreset', descriptors=desc), 'select_by'), (dict(descriptors=desc), 'descriptors without select_by'),
                    (dict(diversity_init='answered'), 'diversity_init without select_by'),
                    (dict(select_by='kcenter'), 'needs descriptors'), (dict(select_by='kcenter', descriptors=desc.double()), 'needs descriptors'),
                    (dict(select_by='kcenter', descriptors=desc[0]), 'needs descriptors'),
                    (dict(select_by='kcenter', descriptors=np.zeros((6, 8), dtype=np.float32)), 'needs descriptors'),
                    (dict(select_by='kcenter', descriptors=torch.zeros(6, 4097)), 'needs descriptors'),
                    (dict(select_by='kcenter', descriptors=desc, diversity_init='all'), 'diversity_init')):
        with pytest.raises(ValueError, match=msg):
            al.check_round(**kw)
    # a round without the switches: the tuple it was, field for field
    pol = al.check_round()
    assert tuple(pol) == ('deterministic', 'uncert_video', 'uncert_frame', 'heuristic', None, 1, None, None, None, None, None, False, 1, 0.7)
    assert pol._fields == ('posterior', 'rank_by', 'observe_by', 'renew_by', 'acquire_by', 'Q', 'stop_entropy', 'noise', 'temperature',
                           'calibrate', 'flip', 'reads_posterior', 'questions_at_once', 'hit_iou')
    assert pol.select_by is None and pol.descriptors is None and pol.diversity_init is None and pol.stop_hit is None
    on = al.check_round(select_by='kcenter', descriptors=desc, diversity_init='answered', rank_by='span_risk')
    assert tuple(on) == tuple(al.check_round(rank_by='span_risk')) and on == al.check_round(rank_by='span_risk')
    assert on.select_by == 'kcenter' and on.descriptors is desc and on.diversity_init == 'answered'
