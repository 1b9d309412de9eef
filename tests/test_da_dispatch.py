"""Host only: the case table of tests/test_gpu_da_forms.py names every kernel instantiation its restatement of the dual attention
dispatch (csrc/attn.hip launch_attn_fwd / launch_attn_bwd, the row tiles of csrc/dablock.hip) can return for clips and queries of up to
256 rows - a later change of that restatement, which the GPU cases hold to the launched symbols, cannot take a form out of coverage
silently."""
import pytest

import test_gpu_da_forms as t
from test_gpu_da_bwd_fused import _rows_per_workgroup


def test_case_table_names_every_attention_instantiation():
    fwd = {t.attn_fwd_form(T, L) for T in range(1, 257) for L in range(1, 257)}
    bwd = {t.attn_bwd_form(T, L) for T in range(1, 257) for L in range(1, 257)}
    assert fwd == {'attn_fwd_kernel<%d, %d>' % f for f in ((2, 256), (2, 512), (4, 512), (8, 512), (16, 512))}, sorted(fwd)
    assert bwd == {'attn_bwd_chain_kernel', 'attn_bwd_big_kernel', 'attn_bwd_kernel'}, sorted(bwd)
    assert fwd | bwd <= t.covered_symbols(), sorted((fwd | bwd) - t.covered_symbols())


def test_case_table_names_every_row_tile_instantiation():
    """clip counts up to 256 at the bench lengths and at the row-tile cases' own: one to four tiles for ln_proj, one to three for the
    kernels whose workgroups hold at most 48 rows"""
    syms = {s for T, L in ((128, 20), (64, 8)) for B in range(1, 257) for s in t.dispatch(B, T, L) if not s.startswith('attn_')}
    want = {'ln_proj_kernel<%d, true>' % n for n in (1, 2, 3, 4)}
    for n in (1, 2, 3):
        want |= {'da_post_kernel<%d>' % n, 'ln_proj_bwd_kernel<false, %d>' % n, 'da_mid_bwd_kernel<%d>' % n, 'ln_proj_bwd_kernel<false, %d, true>' % n}
    assert syms == want, sorted(syms ^ want)
    assert syms <= t.covered_symbols(), sorted(syms - t.covered_symbols())


def test_every_backward_kernel_runs_with_and_without_whole_xcd_groups():
    for sym in ('attn_bwd_chain_kernel', 'attn_bwd_big_kernel', 'attn_bwd_kernel'):
        Bs = {sh['B'] for _, _, sh in t.CASES if t.attn_bwd_form(sh['T'], sh['L']) == sym}
        assert any(B % 8 == 0 for B in Bs) and any(B % 8 for B in Bs), (sym, sorted(Bs))
        assert any(layer == 1 for _, layer, sh in t.CASES if t.attn_bwd_form(sh['T'], sh['L']) == sym), sym


def test_cases_sit_on_both_sides_of_each_boundary():
    """the rows of the table run what they are listed for"""
    for cls, what, shapes in t.TABLE:
        for B, T, L in shapes:
            f, b = t.attn_fwd_form(T, L), t.attn_bwd_form(T, L)
            if what.startswith('fwd <'):
                assert f == 'attn_fwd_kernel<%s>' % what[5:what.index('>')].replace(',', ', '), (what, T, L, f)
            elif cls in ('chain', 'big'):
                assert b == 'attn_bwd_%s_kernel' % cls, (what, T, L, b)
            elif cls == 'plain':
                assert b == 'attn_bwd_kernel', (what, T, L, b)
    # mixed key-panel widths in one forward launch: 16 padded key tiles next to 2
    assert all(T > 128 and L <= 32 for _, T, L in t.TABLE[4][2])


@pytest.mark.parametrize('nt,shape', [(n + 2, sh) for n, sh in enumerate(sh for c, _, sh in t.CASES if c == 'tiles' and sh['T'] == 64)], ids=t._id)
def test_row_tile_cases_sit_just_over_their_row_counts(nt, shape):
    """the NT = 2, 3, 4 cases: the smallest B with more than 4096 / 8192 / 12288 rows.  ln_proj (up to 64 rows per workgroup) runs nt
    tiles, the kernels of at most 48 rows min(nt, 3); the last workgroup's rows end inside its tile and the workgroup's last tile is
    partly used - but for the 48-row kernels beyond 12288 rows, which sit at their cap of three whole tiles"""
    B, T, L = shape['B'], shape['T'], shape['L']
    R_, Nv = B * (T + L), B * T
    assert (B - 1) * (T + L) <= 4096 * (nt - 1) < R_
    mt4, mt3 = t.tile_rows(R_, Nv, t.LP_ROWS), t.tile_rows(R_, Nv, t.DP_ROWS)
    assert mt3 == _rows_per_workgroup(R_, Nv)
    assert t.row_tiles(B, T, L) == (nt, min(nt, 3)), (mt4, mt3)
    assert R_ % mt4 != 0 and mt4 % 16 != 0 and R_ % mt3 != 0, (R_, mt4, mt3)
    assert mt3 % 16 != 0 or (nt == 4 and mt3 == t.DP_ROWS), (R_, mt3)
