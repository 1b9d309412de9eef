"""CPU: gradient-embedding acquisition (hual_al_grad_embed, hual_kcenter_sample) is declared, exported and bound; the float64
references (tests/grad_embed_ref.py, tests/kcenter_sample_ref.py) against torch autograd, against the enumeration of the expected
gradient length and against the law of D^2 sampling; argument errors of the C entry points, the wrappers and the policy switches
without a GPU; the unchanged RoundPolicy of a round without the new switches."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import grad_embed_ref as GR
import kcenter_sample_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_exported_and_the_abi_version_stays():
    from hual_amd import lib
    src = open(os.path.join(ROOT, 'include', 'hual_seqpan.h')).read()
    for name in ('hual_al_grad_embed', 'hual_kcenter_sample'):
        assert re.search(r'\b%s\s*\(' % name, src)
        assert hasattr(ctypes.CDLL(lib.LIB_PATH), name), 'missing export ' + name
    assert lib.load().hual_abi_version() == lib.ABI_VERSION == 9          # new symbols, the ABI version stays
    assert callable(lib.al_grad_embed) and callable(lib.kcenter_sample)
    sites = {k: int(v) for k, v in re.findall(r'#define (HUAL_SITE_\w+) (\d+)', src)}
    assert sites['HUAL_SITE_SELECT'] == SR.SITE_SELECT == max(sites.values())
    assert SR.SITE_SELECT > sites['HUAL_SITE_FE'] + 16 * 4 + 8            # above every dropout site in use


def test_reference_is_the_autograd_gradient_of_the_head():
    """CE(softmax(h @ w + b), onehot) on a toy head: d / dw = sum_t (p(t) - y(t)) h(t), in float64"""
    g = np.random.default_rng(0)
    T, v = 9, 7
    h = g.standard_normal((T, GR.H))
    for y in (0, 3, v - 1):
        w = torch.tensor(g.standard_normal(GR.H), dtype=torch.float64, requires_grad=True)
        b = torch.tensor(0.3, dtype=torch.float64)
        z = torch.from_numpy(h[:v]) @ w + b
        loss = -torch.log_softmax(z, dim=0)[y]
        loss.backward()
        r = GR.head(h, z.detach().numpy(), v, y)
        np.testing.assert_allclose(r['g'], w.grad.numpy(), rtol=1e-12, atol=1e-14)
    # no label: the expected feature
    r = GR.head(h, z.detach().numpy(), v, -1)
    np.testing.assert_array_equal(r['g'], r['mu'])
    np.testing.assert_array_equal(GR.head(h, z.detach().numpy(), v, v)['g'], r['mu'])


def test_egl_is_the_expectation_of_the_squared_gradient_length():
    g = np.random.default_rng(1)
    for T, v in ((1, 1), (2, 2), (12, 5), (33, 33)):
        h, z = g.standard_normal((T, GR.H)), 3.0 * g.standard_normal(T)
        want = GR.egl_by_enumeration(h, z, v)
        got = GR.head(h, z, v, -1)['egl']
        assert got == pytest.approx(want, rel=1e-12, abs=1e-300)
    assert GR.head(h[:1], z[:1], 1, -1)['egl'] == 0.0                      # one frame: the model is certain, nothing to learn


def test_embed_marks_poisoned_rows_and_clamps_the_length():
    g = np.random.default_rng(2)
    B, T = 4, 5
    hs, he = g.standard_normal((B * T, GR.H)), g.standard_normal((B * T, GR.H))
    zs, ze = g.standard_normal((B, T)), g.standard_normal((B, T))
    zs[2, 1] = np.inf
    r = GR.embed(hs, he, zs, ze, [9, 0, 5, 3], [[0, 4], [0, 0], [1, 1], [3, 2]], T)
    assert r['poisoned'].tolist() == [False, True, True, False]
    assert np.isnan(r['desc'][1]).all() and r['gnorm2'][2] == r['egl'][2] == -1.0
    np.testing.assert_array_equal(r['desc'][3, :GR.H], GR.head(hs[15:20], zs[3], 3, 3)['mu'])       # hyp 3 lies outside [0, 3): no label
    assert r['gnorm2'][0] == pytest.approx((r['desc'][0] ** 2).sum(), rel=1e-14) and (r['desc_bar'][0] > 0).all()


def test_exponentials_are_unit_exponentials_on_the_grid():
    e = SR.exponentials(seed=7, offset=3, s=2, N=20000)
    assert e.dtype == np.float64 and (e > 0).all() and e.max() < 17.4 and (e.astype(np.float32) == e).all()
    assert abs(e.mean() - 1.0) < 0.03 and abs(e.var() - 1.0) < 0.06
    assert not np.array_equal(e, SR.exponentials(7, 3, 3, 20000)) and not np.array_equal(e, SR.exponentials(7, 4, 2, 20000))
    assert not np.array_equal(e, SR.exponentials(8, 3, 2, 20000)) and not np.array_equal(e, SR.exponentials(7 + (1 << 32), 3, 2, 20000))
    np.testing.assert_array_equal(e[:50], SR.exponentials(7, 3, 2, 50))   # a row's draw does not depend on N


def test_reference_sampler_on_a_hand_worked_example():
    """six points on a line, rows 0 / 1 duplicates.  origin: mind opens as x^2 and assign -1.  Greedy with origin picks the row of
    largest w x^2; rows at distance 0 of a center score an exact zero and go last, in (w, -i) order"""
    x = np.array([[0.0], [0.0], [10.0], [10.0], [4.0], [6.0]])
    w = np.array([0.5, 1.0, 0.5, 0.5, 1.0, 0.0])
    r = SR.run(x, 6, w, sample=False, origin=True)
    assert r['open_mind'].tolist() == [0, 0, 100, 100, 16, 36]
    assert r['picked'].tolist() == [2, 4, 1, 0, 3, 5] and r['pick_dist'].tolist() == [100.0, 16.0, 0.0, 0.0, 0.0, 4.0]
    assert r["assign"].tolist() == [-1, -1, 2, 2, 4, 5]                    # rows 0 / 1 sit on the origin; a pick is its own center
    # both switches off: k-center as it was
    assert SR.run(x, 6, w, sample=False, origin=False)['picked'].tolist() == [1, 2, 4, 0, 3, 5]
    # sampling: zero-mass rows are taken only when nothing else is left, whatever the seed; the same seed gives the same picks
    for seed in range(20):
        s = SR.run(x, 6, w, seed=seed, sample=True, origin=True)
        assert sorted(s['picked'][:2].tolist()) == [2, 4] or sorted(s['picked'][:2].tolist()) == [3, 4]
        assert s['picked'][-1] == 5 and set(s['picked'].tolist()) == set(range(6))
        assert s['picked'].tolist() == SR.run(x, 6, w, seed=seed, sample=True, origin=True)['picked'].tolist()
    firsts = {int(SR.run(x, 1, w, seed=seed)['picked'][0]) for seed in range(64)}
    assert firsts == {2, 3, 4}                                            # mass 50, 50, 16; rows 0, 1, 5 have none


def test_reference_sampler_follows_its_law():
    """n_select = 1 over 2,000 consecutive seeds: the picks against w * mind / sum, chi-square with 5 degrees of freedom below the
    0.001 quantile.  A condition on the reference (the seed base was chosen here), not a measurement of the kernel"""
    x, w, init, mass = SR.law_case()
    assert len(set(mass.tolist())) == 6 and (mass > 0).all()
    counts = np.zeros(6)
    for j in range(SR.LAW_SEEDS):
        r = SR.run(x, 1, w, init=init, seed=SR.LAW_SEED_BASE + j, sample=True, origin=False)
        counts[int(r['picked'][0]) - 1] += 1
    stat = SR.chi_square(counts, mass)
    print('chi-square %.2f (bar %.1f), counts %s, expected %s' % (stat, SR.LAW_BAR, counts.tolist(), np.round(2000 * mass / mass.sum(), 1).tolist()))
    assert stat < SR.LAW_BAR


def test_bad_arguments_fail_loudly_without_a_gpu():
    from hual_amd import lib
    l = lib.load()
    one = ctypes.c_void_p(16)                                             # never dereferenced: every call below fails before any HIP call

    def ks(x=one, N=8, D=4, ld=4, w=None, init=None, n_init=0, n_select=2, out=one, ws=one, ws_bytes=1 << 20):
        return l.hual_kcenter_sample(x, N, D, ld, w, init, n_init, n_select, 1, 0, 1, 1, out, out, out, out, ws, ws_bytes, None)

    for kw, msg in ((dict(N=0), b'N >= 1'), (dict(D=0), b'1 <= D <= 4096'), (dict(D=4097, ld=4097), b'1 <= D <= 4096'), (dict(ld=3), b'ld >= D'),
                    (dict(n_select=9), b'0 <= n_select <= N'), (dict(n_select=-1), b'0 <= n_select <= N'), (dict(n_init=9), b'0 <= n_init <= N'),
                    (dict(n_init=1), b'null pointer (init'), (dict(x=None), b'null pointer'), (dict(out=None), b'null pointer'),
                    (dict(ws=None), b'null pointer'), (dict(ws_bytes=16), b'workspace smaller'), (dict(ws=ctypes.c_void_p(8)), b'16-byte aligned')):
        rc = ks(**kw)
        assert rc == -1 and msg in l.hual_last_error() and b'hual_kcenter_sample' in l.hual_last_error(), (kw, rc, l.hual_last_error())
    assert ks(n_select=0, x=None, out=None, ws=None) == 0                 # nothing owed: nothing launched, nothing read

    def ge(hs=one, he=one, zs=one, ze=one, vl=one, hyp=one, rows=None, B=2, T=4, ld=4, N=8, desc=one, ld_desc=256, gn=one, egl=one):
        return l.hual_al_grad_embed(hs, he, zs, ze, vl, hyp, rows, B, T, ld, N, desc, ld_desc, gn, egl, None)

    for kw, msg in ((dict(hs=None), b'null pointer'), (dict(he=None), b'null pointer'), (dict(zs=None), b'null pointer'),
                    (dict(ze=None), b'null pointer'), (dict(vl=None), b'null pointer'), (dict(hyp=None), b'null pointer'),
                    (dict(desc=None), b'null pointer'), (dict(gn=None), b'null pointer'), (dict(egl=None), b'null pointer'),
                    (dict(B=0), b'B >= 1'), (dict(N=0), b'N >= 1'), (dict(T=0), b'1 <= T <= 256'), (dict(T=257, ld=257), b'1 <= T <= 256'),
                    (dict(ld=3), b'T <= ld <= 1024'), (dict(ld=1025), b'T <= ld <= 1024'), (dict(ld_desc=255), b'ld_desc >= 256')):
        rc = ge(**kw)
        assert rc == -1 and msg in l.hual_last_error() and b'hual_al_grad_embed' in l.hual_last_error(), (kw, rc, l.hual_last_error())

    # the wrappers' own gates come before any launch too
    x = torch.zeros(4, 3)
    for kw, exc in ((dict(n_select=5), ValueError), (dict(n_select=2, init=[4]), ValueError), (dict(n_select=2, init=[1, 1]), ValueError),
                    (dict(n_select=2, seed=-1), ValueError), (dict(n_select=2, seed=1 << 64), ValueError), (dict(n_select=2, seed=1.5), ValueError),
                    (dict(n_select=2, seed=True), ValueError), (dict(n_select=2, offset=1 << 32), ValueError),
                    (dict(n_select=2, offset=-1), ValueError), (dict(n_select=2, weight=torch.zeros(3)), lib.HualError),
                    (dict(n_select=2, out=(None,) * 3), lib.HualError)):
        with pytest.raises(exc):
            lib.kcenter_sample(x, **kw)
    for bad in (torch.zeros(4, 3, dtype=torch.float64), torch.zeros(4), torch.zeros(4, 4097), torch.zeros(4, 6)[:, ::2]):
        with pytest.raises(lib.HualError):
            lib.kcenter_sample(bad, 1)
    B, T, N = 2, 4, 8
    ok = dict(hs=torch.zeros(B * T, 128), he=torch.zeros(B * T, 128), s_logits=torch.zeros(B, T), e_logits=torch.zeros(B, T),
              v_len=torch.zeros(B, dtype=torch.int32), hyp=torch.zeros(B, 2, dtype=torch.int32), desc=torch.zeros(N, 256),
              gnorm2=torch.zeros(N), egl=torch.zeros(N), rows=None)
    for kw in (dict(hs=torch.zeros(B * T, 64)), dict(he=torch.zeros(B * T + 1, 128)), dict(hs=torch.zeros(B * T, 128, dtype=torch.float64)),
               dict(hs=torch.zeros(7, 128), he=torch.zeros(7, 128)), dict(hs=torch.zeros(B * 257, 128), he=torch.zeros(B * 257, 128)),
               dict(s_logits=torch.zeros(B, T - 1)), dict(e_logits=torch.zeros(B, T + 1)), dict(s_logits=torch.zeros(B + 1, T)),
               dict(s_logits=torch.zeros(B, 1025), e_logits=torch.zeros(B, 1025)), dict(e_logits=torch.zeros(B, 2 * T)[:, :T]),
               dict(v_len=torch.zeros(B, dtype=torch.int64)), dict(hyp=torch.zeros(B, 2, dtype=torch.int64)), dict(hyp=torch.zeros(B, dtype=torch.int32)),
               dict(rows=torch.zeros(B, dtype=torch.int64)), dict(rows=torch.zeros(B + 1, dtype=torch.int32)), dict(desc=torch.zeros(N, 255)),
               dict(desc=torch.zeros(1, 256), gnorm2=torch.zeros(1), egl=torch.zeros(1)), dict(gnorm2=torch.zeros(N + 1)),
               dict(egl=torch.zeros(N, dtype=torch.float64)), dict(desc=np.zeros((N, 256), dtype=np.float32))):
        with pytest.raises(lib.HualError):
            lib.al_grad_embed(**dict(ok, **kw))


def test_policy_switches_are_checked_before_anything_runs():
    from hual_amd import al
    desc = torch.zeros(6, 256)
    for kw, msg in ((dict(select_by='badges', descriptors=desc), 'select_by'), (dict(descriptors=desc), 'descriptors without select_by'),
                    (dict(diversity_init='answered'), 'diversity_init without select_by'), (dict(select_by='badge'), 'needs descriptors'),
                    (dict(select_by='badge', descriptors=desc.double()), 'needs descriptors'),
                    (dict(select_by='badge', descriptors=desc[0]), 'needs descriptors'),
                    (dict(select_by='badge', descriptors=torch.zeros(6, 4097)), 'needs descriptors'),
                    (dict(select_by='badge', descriptors=desc, diversity_init='all'), 'diversity_init'),
                    (dict(selection_seed=3), 'selection_seed without select_by'),
                    (dict(select_by='kcenter', descriptors=desc, selection_seed=3), 'selection_seed without select_by'),
                    (dict(select_by='badge', descriptors=desc, selection_seed=-1), 'selection_seed'),
                    (dict(select_by='badge', descriptors=desc, selection_seed=1 << 64), 'selection_seed'),
                    (dict(select_by='badge', descriptors=desc, selection_seed=0.5), 'selection_seed'),
                    (dict(rank_by='egls'), 'rank_by'), (dict(rank_by='egl', acquire_by='label_gain'), 'acquire_by')):
        with pytest.raises(ValueError, match=msg):
            al.check_round(**kw)
    # rank_by='egl' needs the records of a pass that filled a bank
    with pytest.raises(ValueError, match='prop_egl'):
        al.grad_length([{'prop_egl': 1.0}, {}])
    assert al.grad_length([{'prop_egl': 1.5}, {'prop_egl': -1.0}]).tolist() == [1.5, -1.0]
    recs = [{'v_len': 4, 'prop_logits': (np.zeros(4, np.float32),) * 2, 'prop_logits1': (np.zeros(4, np.float32),) * 2,
             'prop_logits2': (np.zeros(4, np.float32),) * 2}]
    old = [['v', 10.0, [1.0, 2.0], 'a sentence']]
    with pytest.raises(ValueError, match='prop_egl'):
        al.update_labels([list(r) for r in old], old, recs, al.get_coff('charades', 1), rank_by='egl')
    # the selection helper and the bank refuse bad arguments on the host
    for kw in (dict(desc=np.zeros((6, 4), np.float32)), dict(seed=-1), dict(seed=2.0), dict(weight=np.ones(5))):
        with pytest.raises(ValueError):
            al.badge_select(**dict(dict(desc=torch.zeros(6, 4), n_select=2), **kw))
    with pytest.raises(ValueError):
        al.GradBank(0, device='cpu')
    bank = al.GradBank(5, device='cpu')
    assert tuple(bank.desc.shape) == (5, 256) and tuple(bank.gnorm2.shape) == tuple(bank.egl.shape) == (5,)
    assert bank.rows([4, 0]).tolist() == [4, 0] and bank.rows([4, 0]).dtype == torch.int32
    for ids in ([5], [-1], [[0]]):
        with pytest.raises(ValueError):
            bank.rows(ids)
    with pytest.raises(ValueError, match='grad_hyp'):
        al.infer_trainset(None, [], grad_bank=bank, grad_hyp='truth')
    with pytest.raises(ValueError, match='grad_bank'):
        al.infer_trainset(None, [], grad_bank=object())
    assert al.infer_trainset(None, [], grad_bank=bank) == ([], [])


def test_a_round_without_the_switches_is_the_round_it_was():
    from hual_amd import al
    pol = al.check_round()
    assert tuple(pol) == ('deterministic', 'uncert_video', 'uncert_frame', 'heuristic', None, 1, None, None, None, None, None, False, 1, 0.7)
    assert pol._fields == ('posterior', 'rank_by', 'observe_by', 'renew_by', 'acquire_by', 'Q', 'stop_entropy', 'noise', 'temperature',
                           'calibrate', 'flip', 'reads_posterior', 'questions_at_once', 'hit_iou')
    assert pol.select_by is None and pol.descriptors is None and pol.diversity_init is None and pol.stop_hit is None
    assert pol.selection_seed is None
    desc = torch.zeros(6, 256)
    on = al.check_round(select_by='badge', descriptors=desc, diversity_init='answered', selection_seed=11, rank_by='egl')
    assert tuple(on)[:1] + tuple(on)[2:] == tuple(pol)[:1] + tuple(pol)[2:] and on.rank_by == 'egl' and len(on) == len(pol)
    assert on.select_by == 'badge' and on.descriptors is desc and on.diversity_init == 'answered' and on.selection_seed == 11
    assert al.check_round(select_by='badge', descriptors=desc).selection_seed is None


def test_taps_that_share_bytes_with_another_buffer_are_copied():
    """_head_taps on hand-made workspace tables: every named buffer in a range of its own -> read in place; another entry inside the
    bytes of head.hs or head.he -> not private, and GradBank.embed would copy the taps out in the forward's stream"""
    import types
    from hual_amd import al

    def model(table):
        ws = torch.zeros(8192, dtype=torch.uint8)
        m = types.SimpleNamespace(_ws_table=table, _ws=ws)
        m.tap = lambda name: ws[table[name][0]:table[name][0] + table[name][1] * table[name][2] * 4].view(torch.float32).view(table[name][1:])
        return m
    apart = {'head.hs': (0, 2, 128), 'head.he': (1024, 2, 128), 'fuse': (2048, 2, 128), 'head.zs': (3072, 2, 1)}
    taps, private = al._head_taps(model(apart))
    assert private and tuple(taps[0].shape) == tuple(taps[1].shape) == (2, 128)
    for name, entry in (('late', (512, 1, 128)), ('late', (1024 + 1020, 1, 1)), ('late', (0, 16, 128)), ('head.hs2', (1020, 1, 1))):
        assert not al._head_taps(model(dict(apart, **{name: entry})))[1], entry
    for entry in ((2048, 1, 128), (3072, 1, 1), (4096, 4, 128)):           # beside the taps, even on another buffer: private
        assert al._head_taps(model(dict(apart, late=entry)))[1], entry
