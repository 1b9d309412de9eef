"""CPU: hual_adamw_clip_step_ema (averaged weights in the optimizer launch) - the symbol, and the host-side argument checks that
return before any HIP call (no GPU needed)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ema_entry_point_is_declared_and_exported():
    from hual_amd import build, lib
    build.build()
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'hual_seqpan.h')).read(), flags=re.S)
    assert re.search(r'\bint hual_adamw_clip_step_ema\s*\(', src)
    assert hasattr(ctypes.CDLL(lib.LIB_PATH), 'hual_adamw_clip_step_ema')
    assert lib.load().hual_abi_version() == lib.ABI_VERSION
    # the three older optimizer entry points are still there
    for n in ('hual_adamw_clip_step', 'hual_adamw_clip_step_rng', 'hual_adamw_clip_step_loop'):
        assert hasattr(ctypes.CDLL(lib.LIB_PATH), n)


def _call(l, ema, count, decay, warmup=1):
    p = ctypes.c_void_p(0x1000)      # never dereferenced: every case below is refused on the host
    return l.hual_adamw_clip_step_ema(p, p, p, p, p, 1024, p, 1.0, 1.0, p, None, None, None, None, 0, 0, 0, ema, count, decay, warmup, None)


def test_ema_and_counter_go_together():
    from hual_amd import lib
    import pytest
    l = lib.load()
    p = ctypes.c_void_p(0x2000)
    rc = _call(l, None, p, 0.999)
    assert rc == -1 and b'ema_count without ema' in l.hual_last_error(), l.hual_last_error()
    rc = _call(l, p, None, 0.999)
    assert rc == -1 and b'ema without ema_count' in l.hual_last_error(), l.hual_last_error()
    with pytest.raises(lib.HualError, match='ema'):
        lib.check(rc)


def test_ema_decay_outside_the_unit_interval_is_refused():
    from hual_amd import lib
    l = lib.load()
    p = ctypes.c_void_p(0x2000)
    for decay in (1.0, 1.5, -0.1, float('nan'), float('inf')):
        rc = _call(l, p, p, decay)
        assert rc == -1 and b'ema_decay' in l.hual_last_error(), (decay, l.hual_last_error())
        rc = _call(l, None, None, decay)       # ... with or without a shadow
        assert rc == -1 and b'ema_decay' in l.hual_last_error(), (decay, l.hual_last_error())


def test_config_keys_are_validated_without_a_gpu():
    """train.ema_decay / train.ema_warmup as SeqPAN and Runner read them: absent or 0 = off, warm-up on by default, a decay outside
    [0, 1) refused"""
    import pytest
    from hual_amd import lib
    from hual_amd.model import ema_settings
    assert ema_settings(dict(train=dict(lr=1e-3))) == (0.0, True)
    assert ema_settings(dict(train=dict(ema_decay=0))) == (0.0, True)
    assert ema_settings(dict(train=dict(ema_decay=0.999, ema_warmup=False))) == (0.999, False)
    assert ema_settings(lib.make_cfg()) == (0.0, True)
    assert ema_settings(lib.make_cfg(), ema_decay=0.99) == (0.99, True)
    for bad in (1.0, -0.5, 2):
        with pytest.raises(lib.HualError, match='train.ema_decay'):
            ema_settings(dict(train=dict(ema_decay=bad)))
