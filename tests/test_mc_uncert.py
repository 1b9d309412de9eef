"""CPU: the K-pass uncertainty bank's C entry points (hual_al_mc_fold, hual_al_score_mc) are exported and refuse bad arguments before any
HIP call, and the numpy reference the GPU tests compare against (tests/mc_uncert_ref.py) is itself right: RANGE at K = 2 is the
reference's get_uncert_model element for element, STD is sqrt(2) times the float64 sample deviation to 1e-6."""
import ctypes
import os
import re

import numpy as np
import pytest

import mc_uncert_ref as R
from oracle import al_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_declared_and_exported():
    from hual_amd import build, lib
    build.build()
    src = open(os.path.join(ROOT, 'include', 'hual_seqpan.h')).read()
    l = ctypes.CDLL(lib.LIB_PATH)
    for name in ('hual_al_mc_fold', 'hual_al_score_mc'):
        assert re.search(r'\bint %s\s*\(' % name, src), name
        assert hasattr(l, name), 'missing export ' + name
    assert lib.load().hual_abi_version() == lib.ABI_VERSION == 9          # new symbols, the ABI version stays


def _fake_bank(lib, N=4, ld=64, **null):
    """a hual_al_bank over HOST memory: enough for the argument checks, which return before anything is launched"""
    buf = ctypes.create_string_buffer(64)
    a = ctypes.addressof(buf)
    f = {k: a for k in ('tlen', 's0', 'e0', 'lo_s', 'hi_s', 'mean_s', 'm2_s', 'lo_e', 'hi_e', 'mean_e', 'm2_e')}
    f.update(null)
    b = lib.hual_al_bank(N, ld, *[f[k] for k in ('tlen', 's0', 'e0', 'lo_s', 'hi_s', 'mean_s', 'm2_s', 'lo_e', 'hi_e', 'mean_e', 'm2_e')])
    return b, buf, ctypes.c_void_p(a)


def test_fold_refuses_bad_arguments_without_a_gpu():
    from hual_amd import lib
    l = lib.load()
    bank, keep, p = _fake_bank(lib)
    for args, msg in (((None, p, p, p, p, 2, 16, 0, None), b'null bank'),
                      ((ctypes.byref(bank), None, p, p, p, 2, 16, 0, None), b'null input'),
                      ((ctypes.byref(bank), p, p, p, None, 2, 16, 1, None), b'null input'),
                      ((ctypes.byref(_fake_bank(lib, m2_e=None)[0]), p, p, p, p, 2, 16, 1, None), b'null bank'),
                      ((ctypes.byref(_fake_bank(lib, tlen=None)[0]), p, p, p, p, 2, 16, 0, None), b'null bank'),
                      ((ctypes.byref(_fake_bank(lib, ld=1025)[0]), p, p, p, p, 2, 16, 1, None), b'ld <= 1024'),
                      ((ctypes.byref(_fake_bank(lib, N=0)[0]), p, p, p, p, 2, 16, 1, None), b'N > 0'),
                      ((ctypes.byref(bank), p, p, p, p, 2, 65, 1, None), b'T_b <= ld'),
                      ((ctypes.byref(bank), p, p, p, p, 2, 1, 1, None), b'T_b <= ld'),
                      ((ctypes.byref(bank), p, p, p, p, 0, 16, 1, None), b'B > 0'),
                      ((ctypes.byref(bank), p, p, p, p, 2, 16, -1, None), b'k >= 0')):
        rc = l.hual_al_mc_fold(*args)
        assert rc != 0 and msg in l.hual_last_error(), (msg, l.hual_last_error())
    with pytest.raises(lib.HualError):
        lib.check(rc)


def test_score_mc_refuses_bad_arguments_without_a_gpu():
    from hual_amd import lib
    l = lib.load()
    bank, keep, p = _fake_bank(lib)
    a = p.value
    aset = lib.hual_al_set(4, 64, a, a, a, a, a)

    def call(s=ctypes.byref(aset), s0=p, b=ctypes.byref(bank), K=2, stat=0, out=p):
        return l.hual_al_score_mc(s, s0, p, b, K, stat, 0.25, out, p, p, p, p, None, None)
    for kw, msg in ((dict(s=None), b'null pointer'), (dict(b=None), b'null pointer'), (dict(K=1), b'K >= 2'), (dict(K=0), b'K >= 2'),
                    (dict(stat=2), b'stat'), (dict(s0=None), b'null input'), (dict(out=None), b'null output'),
                    (dict(b=ctypes.byref(_fake_bank(lib, hi_e=None)[0])), b'null input'),
                    (dict(b=ctypes.byref(_fake_bank(lib, ld=32)[0])), b'differ in N or ld'),
                    (dict(s=ctypes.byref(lib.hual_al_set(4, 1025, a, a, a, a, a)), b=ctypes.byref(_fake_bank(lib, ld=1025)[0])),
                     b'ld <= 1024')):
        rc = call(**kw)
        assert rc != 0 and msg in l.hual_last_error(), (msg, l.hual_last_error())


def test_range_at_two_passes_is_get_uncert_model(golden_dir):
    g = np.load(os.path.join(golden_dir, 'uncert.npz'))
    for k in range(3):
        lg, vlen = g['u%d_logits' % k], int(g['u%d_vlen' % k])
        fs = R.fold_passes([R.probs(lg[1][0], vlen), R.probs(lg[2][0], vlen)])
        fe = R.fold_passes([R.probs(lg[1][1], vlen), R.probs(lg[2][1], vlen)])
        got = R.uncert(fs, fe, 'range')
        assert got.dtype == np.float32
        np.testing.assert_array_equal(got, A.get_uncert_model(lg[1], lg[2], vlen))
        np.testing.assert_array_equal(got, g['u%d_uncert' % k].astype(np.float32))
        # and in the other order of the two passes
        fs = R.fold_passes([R.probs(lg[2][0], vlen), R.probs(lg[1][0], vlen)])
        fe = R.fold_passes([R.probs(lg[2][1], vlen), R.probs(lg[1][1], vlen)])
        np.testing.assert_array_equal(R.uncert(fs, fe, 'range'), got)


@pytest.mark.parametrize('K', [2, 3, 8, 16])
@pytest.mark.parametrize('noise', [0.3, 0.01, 1e-3])
def test_std_is_sqrt2_times_the_float64_deviation(K, noise):
    """logits as test_gpu_al's _synthetic_round draws them: 1.5 N(0,1) for the deterministic pass, passes = that + noise N(0,1)"""
    g = np.random.default_rng(100 * K + int(noise * 1000))
    base = (g.standard_normal((37, 100)) * 1.5).astype(np.float32)
    vlen = g.integers(1, 101, size=37)
    ps = np.stack([R.probs(base + noise * g.standard_normal(base.shape).astype(np.float32), vlen) for _ in range(K)])
    f = R.fold_passes(ps)
    ref = R.spread64(ps)
    assert f.std().dtype == np.float32 and f.mean.dtype == np.float32 and f.m2.dtype == np.float32
    assert np.abs(f.std().astype(np.float64) - ref).max() <= 1e-6
    assert np.abs(f.mean.astype(np.float64) - ps.astype(np.float64).mean(axis=0)).max() <= 1e-6
    np.testing.assert_array_equal(f.lo, ps.min(axis=0))
    np.testing.assert_array_equal(f.hi, ps.max(axis=0))
    assert (f.std()[np.arange(100)[None, :] >= vlen[:, None]] == 0).all()          # zeroed frames have no spread
    if K == 2:
        assert np.abs(f.std().astype(np.float64) - np.abs(ps[0].astype(np.float64) - ps[1])).max() <= 1e-6
