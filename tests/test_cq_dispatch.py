"""Host only: which padded shapes still need the score scratch of the global-operand context-query kernels.  The range predicate of
the wide kernels (csrc/cqwide.hip cq_wide_ok) has no entry point of its own, but the workspace table (hual_seqpan_ws_table) shows its
effect: `cq.gs` / `d.cq.gd` are reserved exactly for the shapes cq_fwd_global / cq_bwd_global (csrc/cq.hip) name, and a shape the
wide kernels serve reserves neither."""
import os

import pytest

from hual_amd import lib

pytestmark = pytest.mark.skipif(os.environ.get('HUAL_CQ_NO_WIDE', '0') not in ('', '0'), reason='HUAL_CQ_NO_WIDE takes csrc/cqwide.hip out')


def _scratch(T, L, B=16):
    cfg = lib.make_cfg(vdim=64, max_vlen=256, num_words=200, num_chars=30)
    t = lib.ws_table(cfg, B, T, L, 8)
    return sorted(k for k in t if k in ('cq.gs', 'd.cq.gd'))


@pytest.mark.parametrize('TL', [(100, 33), (100, 45), (100, 64), (64, 40), (128, 64), (64, 64), (100, 32), (256, 20), (256, 32)])
def test_shapes_of_the_wide_kernels_reserve_no_score_scratch(TL):
    assert _scratch(*TL) == []


@pytest.mark.parametrize('TL,want', [((100, 65), ['d.cq.gd']), ((100, 79), ['d.cq.gd']), ((256, 40), ['cq.gs', 'd.cq.gd']),
                                     ((256, 33), ['cq.gs', 'd.cq.gd']), ((129, 64), ['cq.gs', 'd.cq.gd'])])
def test_shapes_beyond_the_range_keep_their_score_scratch(TL, want):
    """as on the commit before the 64-row kernels: queries of more than 64 words, or of more than 32 words against more than 128 frames"""
    assert _scratch(*TL) == want


def test_workspace_shrinks_by_the_score_scratch():
    """B=16, T=100: L = 64 (wide) against L = 65 (global-operand backward) - the step from 64 to 65 words adds the GD scratch on top of
    the rows, the step from 63 to 64 adds rows only"""
    cfg = lib.make_cfg(vdim=64, max_vlen=256, num_words=200, num_chars=30)
    q = [lib.query_workspace(cfg, 16, 100, L, 8) for L in (63, 64, 65)]
    assert q[2] - q[1] > 2 * (q[1] - q[0]), q
