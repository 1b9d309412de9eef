"""csrc/bf16x3.h pow2_scale<EB_MAX, C, INV_LOG2>: the one power-of-two operand scale behind f16_row_scale (bf16x3.h), the attention
backward's scales (attn.hip), cq_img_autoscale (cqimg.h) and the running scale of the weight-gradient kernel (gemm.hip).
A numpy restatement of the template is compared bit for bit with the four formulas as the call sites spelled them before they shared
it - every exponent byte 0..255 with both mantissa extremes, a mid mantissa, and 0, the denormals and Inf by name.  CPU only."""
import numpy as np
import pytest

U = np.uint32


def pow2_scale(bits, eb_max, c, inv_log2=0):
    """the template's body on the raw bits of amax; returns the raw bits of (scale, inv)"""
    eb = (bits >> U(23)) & U(0xff)
    eb = np.where(eb < 27, U(27), np.where(eb > eb_max, U(eb_max), eb)).astype(U)
    return (U(c) - eb) << U(23), (eb - U(c - 254) - U(inv_log2)) << U(23)


def _eb(bits, lo, hi):
    eb = (bits >> U(23)) & U(0xff)
    return np.where(eb < lo, U(lo), np.where(eb > hi, U(hi), eb)).astype(U)


def f16_row_scale(bits):             # HUAL_F16_WSCALE_LOG2 = 10
    eb = _eb(bits, 27, 254)
    return (U(267) - eb) << U(23), (eb - U(13) - U(10)) << U(23)


def att_scale(bits):
    eb = _eb(bits, 27, 240)
    return (U(267) - eb) << U(23), (eb - U(13)) << U(23)


def cq_autoscale(bits):
    eb = _eb(bits, 27, 240)
    return (U(267) - eb) << U(23), (eb - U(13)) << U(23)


def dw_running(bits):
    eb = _eb(bits, 27, 240)
    return (U(265) - eb) << U(23), (eb - U(11)) << U(23)


def _inputs():
    eb = np.arange(256, dtype=U) << U(23)
    bits = np.concatenate([eb, eb | U(0x7fffff), eb | U(0x400001), eb | U(1)])
    named = np.array([0.0, np.finfo(np.float32).tiny, 1e-45, 1.1754942e-38, np.inf, np.finfo(np.float32).max], dtype=np.float32).view(U)
    return np.concatenate([bits, named]).astype(U)


SITES = [('f16_row_scale', f16_row_scale, (254, 267, 10)), ('attn', att_scale, (240, 267, 0)),
         ('cq_img_autoscale', cq_autoscale, (240, 267, 0)), ('dw running', dw_running, (240, 265, 0))]


@pytest.mark.parametrize('name,orig,params', SITES, ids=[s[0] for s in SITES])
def test_pow2_scale_bit_exact(name, orig, params):
    bits = _inputs()
    s0, i0 = orig(bits)
    s1, i1 = pow2_scale(bits, *params)
    assert np.array_equal(s0, s1) and np.array_equal(i0, i1)
    # both are finite powers of two and exact inverses of each other up to the folded weight scale
    sc, inv = s1.view(np.float32).astype(np.float64), i1.view(np.float32).astype(np.float64)
    assert np.all(np.isfinite(sc)) and np.all(sc > 0) and np.all(inv > 0)
    assert np.array_equal(sc * inv * 2.0 ** params[2], np.ones_like(sc))


def test_pow2_scale_source_parameters():
    """the four call sites name the parameter sets tested above"""
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'hual_amd', 'csrc')
    found = {}
    for f in ('bf16x3.h', 'attn.hip', 'cqimg.h', 'gemm.hip'):
        found[f] = re.findall(r'pow2_scale<(\d+)u, (\d+)u(?:, (\w+))?>', open(os.path.join(csrc, f)).read())
    assert found['bf16x3.h'] == [('254', '267', 'HUAL_F16_WSCALE_LOG2')]
    assert set(found['attn.hip']) == {('240', '267', '')} and found['cqimg.h'] == [('240', '267', '')] and found['gemm.hip'] == [('240', '265', '')]
    assert '#define HUAL_F16_WSCALE_LOG2 10' in open(os.path.join(csrc, 'bf16x3.h')).read()
