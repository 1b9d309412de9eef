"""CPU: the information-theoretic acquisition's C entry points (hual_al_mc_fold_info, hual_al_score_info) are declared, exported and refuse
bad arguments before any HIP call, and the float64 reference the GPU tests compare against (tests/mc_info_ref.py) has the properties that
define the three statistics."""
import ctypes
import os
import re

import numpy as np
import pytest

import mc_info_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BANK_FIELDS = ('tlen', 's0', 'e0', 'lo_s', 'hi_s', 'mean_s', 'm2_s', 'lo_e', 'hi_e', 'mean_e', 'm2_e')


def test_symbols_are_declared_and_exported():
    from hual_amd import build, lib
    build.build()
    src = open(os.path.join(ROOT, 'include', 'hual_seqpan.h')).read()
    l = ctypes.CDLL(lib.LIB_PATH)
    for name in ('hual_al_mc_fold_info', 'hual_al_score_info'):
        assert re.search(r'\bint %s\s*\(' % name, src), name
        assert hasattr(l, name), 'missing export ' + name
    assert re.search(r'typedef struct hual_al_info \{\s*float \*ent_s, \*ent_e;', src)
    for name, value in (('BALD', 2), ('ENTROPY', 3), ('EXPECTED_ENTROPY', 4)):
        assert re.search(r'#define HUAL_AL_STAT_%s %d\b' % (name, value), src), name
    assert lib.AL_STAT_INFO == {'bald': 2, 'entropy': 3, 'expected_entropy': 4} and lib.AL_STAT == {'range': 0, 'std': 1}
    assert lib.load().hual_abi_version() == lib.ABI_VERSION == 9          # new symbols, the ABI version stays


class _Host:
    """a hual_al_bank, hual_al_info and hual_al_set over HOST memory: enough for the argument checks, which return before anything is
    launched"""

    def __init__(self, lib):
        self.lib = lib
        self.buf = ctypes.create_string_buffer(64)
        self.a = ctypes.addressof(self.buf)
        self.p = ctypes.c_void_p(self.a)

    def bank(self, N=4, ld=64, **null):
        f = {k: self.a for k in BANK_FIELDS}
        f.update(null)
        return ctypes.byref(self.lib.hual_al_bank(N, ld, *[f[k] for k in BANK_FIELDS]))

    def info(self, **null):
        f = dict(ent_s=self.a, ent_e=self.a)
        f.update(null)
        return ctypes.byref(self.lib.hual_al_info(f['ent_s'], f['ent_e']))

    def set(self, N=4, ld=64):
        a = self.a
        return ctypes.byref(self.lib.hual_al_set(N, ld, a, a, a, a, a))


def test_fold_info_refuses_bad_arguments_without_a_gpu():
    from hual_amd import lib
    l = lib.load()
    h = _Host(lib)
    p = h.p

    def call(bank=None, info=None, ids=p, end=p, B=2, T=16, k=1, _null_bank=False, _null_info=False):
        return l.hual_al_mc_fold_info(None if _null_bank else (bank or h.bank()), None if _null_info else (info or h.info()), ids, p, p, end,
                                      B, T, k, None)
    for kw, msg in ((dict(_null_info=True), b'null info'), (dict(info=h.info(ent_s=None)), b'ent_s'), (dict(info=h.info(ent_e=None)), b'ent_e'),
                    (dict(T=65), b'T_b <= ld'), (dict(T=1), b'T_b <= ld'),
                    # and hual_al_mc_fold's own checks, in its own words
                    (dict(_null_bank=True), b'null bank'), (dict(ids=None), b'null input'), (dict(end=None), b'null input'),
                    (dict(bank=h.bank(m2_e=None)), b'null bank'), (dict(bank=h.bank(tlen=None), k=0), b'null bank'),
                    (dict(bank=h.bank(ld=1025)), b'ld <= 1024'), (dict(bank=h.bank(N=0)), b'N > 0'), (dict(B=0), b'B > 0'),
                    (dict(k=-1), b'k >= 0')):
        rc = call(**kw)
        assert rc != 0 and msg in l.hual_last_error(), (kw, msg, l.hual_last_error())
    with pytest.raises(lib.HualError):
        lib.check(rc)


def test_score_info_refuses_bad_arguments_without_a_gpu():
    from hual_amd import lib
    l = lib.load()
    h = _Host(lib)
    p = h.p

    def call(s=None, s0=p, bank=None, info=None, K=2, stat=2, out=p, _null=()):
        return l.hual_al_score_info(None if 's' in _null else (s or h.set()), s0, p, None if 'bank' in _null else (bank or h.bank()),
                                    None if 'info' in _null else (info or h.info()), K, stat, 0.25, out, p, p, p, p, None, None)
    for kw, msg in ((dict(_null=('info',)), b'null info'), (dict(info=h.info(ent_s=None)), b'ent_s'), (dict(info=h.info(ent_e=None)), b'ent_e'),
                    (dict(stat=0), b'stat'), (dict(stat=1), b'stat'), (dict(stat=5), b'stat'), (dict(stat=-1), b'stat'),
                    (dict(K=1, stat=2), b'K >= 2'), (dict(K=0, stat=3), b'K >= 1'), (dict(K=0, stat=4), b'K >= 1'),
                    (dict(bank=h.bank(ld=32)), b'differ in N or ld'), (dict(bank=h.bank(N=5)), b'differ in N or ld'),
                    (dict(_null=('s',)), b'null pointer'), (dict(_null=('bank',)), b'null pointer'), (dict(s0=None), b'null input'),
                    (dict(bank=h.bank(mean_e=None)), b'null input'), (dict(out=None), b'null output'),
                    (dict(s=h.set(ld=1025), bank=h.bank(ld=1025)), b'ld <= 1024')):
        rc = call(**kw)
        assert rc != 0 and msg in l.hual_last_error(), (kw, msg, l.hual_last_error())
    # the existing entry point is what it was: the new constants are not its business
    rc = l.hual_al_score_mc(h.set(), p, p, h.bank(), 2, 2, 0.25, p, p, p, p, p, None, None)
    assert rc != 0 and b'stat' in l.hual_last_error()


# ---------------------------------------------------------------------------------------------------------------------
# the reference's own properties, for random float32 probabilities
def _random_passes(K, seed, shape=(37, 100)):
    g = np.random.default_rng(seed)
    base = g.standard_normal(shape) * 2.0
    lg = np.clip(base[None] + g.standard_normal((K,) + shape) * 1.5, -8.0, 8.0).astype(np.float32)
    vlen = g.integers(1, shape[1] + 1, size=shape[0])
    return np.stack([R.probs(x, vlen) for x in lg]), vlen


def test_h2_64_values():
    p = np.array([0.0, 1.0, 0.5, 0.25, 0.75, -0.0, 1e-30], dtype=np.float32)
    want = [0.0, 0.0, 1.0, 0.8112781244591328, 0.8112781244591328, 0.0, 1e-30 * np.log2(1e30)]
    h = R.h2_64(p)
    assert h.dtype == np.float64
    np.testing.assert_allclose(h, want, rtol=1e-6, atol=0)
    assert R.h2_64(np.float32(np.nextafter(np.float32(1), np.float32(2)))) == 0.0          # p >= 1 -> 0, never NaN


@pytest.mark.parametrize('K', [1, 2, 5, 16])
def test_entropy_is_bald_plus_expected_entropy(K):
    ps, vlen = _random_passes(K, 300 + K)
    pe, _ = _random_passes(K, 400 + K)
    fs, fe = R.fold_passes(ps), R.fold_passes(pe)
    for f in (fs, fe):
        assert f.mi().min() >= -1e-12                                      # Jensen, up to float64 rounding
        assert f.ent.min() >= 0 and f.entropy().max() <= 1.0 + 1e-12
    b, h, e = (R.uncert(fs, fe, s) for s in R.STATS)
    assert b.dtype == h.dtype == e.dtype == np.float64
    assert b.min() >= 0 and h.max() <= 2.0 + 1e-12
    assert np.abs(h - (b + e)).max() <= 1e-12
    if K > 1:
        assert b.max() > 0.01                                             # the passes do disagree somewhere
    masked = np.arange(ps.shape[2])[None, :] >= vlen[:, None]
    assert (R.uncert(fs, fs, 'entropy')[masked] == 0).all() and (R.uncert(fs, fs, 'expected_entropy')[masked] == 0).all()


@pytest.mark.parametrize('K', [2, 3, 7])
def test_identical_passes_have_no_mutual_information(K):
    ps, _ = _random_passes(1, 500 + K)
    f = R.fold_passes([ps[0]] * K)
    assert np.abs(f.mi()).max() <= 1e-12 and f.bald().max() <= 1e-12
    assert f.entropy().max() > 0.9                                        # while every pass is unsure somewhere


def test_opposite_passes_have_one_bit_per_head():
    ps, _ = _random_passes(1, 600, shape=(11, 40))
    p = ps[0][ps[0] > 0]
    f = R.fold_passes([p, (np.float32(1) - p).astype(np.float32)])
    assert np.abs(f.entropy() - 1.0).max() <= 1e-12
    assert np.abs(R.uncert(f, f, 'entropy') - 2.0).max() <= 1e-12
