"""Host only: the case table of tests/test_gpu_cb_forms.py names every class of tile form its restatement of the conv block's and the
predictor's dispatch (csrc/convblock.hip, csrc/common.h xcd_clip_rows, the caps 46 / 40; csrc/heads.hip, csrc/attn.hip, csrc/dablock.hip
for the predictor) tells apart, with cases on both sides of each boundary - a later change of that restatement, which the GPU cases hold to
the launched symbols, or of the table cannot take a form out of coverage silently."""
import test_gpu_cb_forms as t


def _cb(cls=None):
    return [(c, sh, t.cb_form(sh['B'], sh['T'], sh['L'])) for c, sh in t.CB_CASES if cls in (None, c)]


def _pred(cls=None):
    return [(c, sh, t.pred_form(sh['B'], sh['T'])) for c, sh in t.PRED_CASES if cls in (None, c)]


def test_four_tile_thresholds_of_the_restatement():
    """forward layer l takes four tiles from MT 31 / 37 / 43 (l = 0 / 1 / 2), backward layer i from MT 25 / 31 / 37 (i = 3 / 2 / 1);
    the last forward layer (no halo) and the first backward layer never do"""
    for mt in range(16, t.CB_FWD_CAP + 1):
        assert t.fwd_tiles(mt) == [4 if mt >= 31 else 3, 4 if mt >= 37 else 3, 4 if mt >= 43 else 3, 3], mt
    for mt in range(16, t.CB_BWD_CAP + 1):
        assert t.bwd_tiles(mt) == [3, 4 if mt >= 37 else 3, 4 if mt >= 31 else 3, 4 if mt >= 25 else 3], mt


def test_every_class_is_named_by_a_case_that_runs_it():
    want = {'t3': lambda f: f['mt'] == (16, 16),
            'b4': lambda f: f['mt'][0] == f['mt'][1] and 25 <= f['mt'][0] <= 30,
            'f1b2': lambda f: f['mt'][0] == f['mt'][1] and 31 <= f['mt'][0] <= 36,
            'mt37': lambda f: f['mt'][0] == f['mt'][1] and 37 <= f['mt'][0] <= 40,
            'fcap': lambda f: f['mt'][0] in (41, 42) and f['mt'][1] == 40,
            'f3': lambda f: 43 <= f['mt'][0] <= 46 and f['mt'][1] == 40,
            'round2': lambda f: f['mt'] == (46, 40) and f['grid'][0][1] == 2 and f['grid'][1][1] == 2,
            'short': lambda f: f['mt'][0] >= 16}
    assert [c for c, _, _ in t.CB_TABLE] == list(want)
    for cls, sh, f in _cb():
        assert want[cls](f), (cls, sh, f)
    # the tile products the classes stand for
    assert all(f['fwd_tiles'] == [3, 3, 3, 3] and f['bwd_tiles'] == [3, 3, 3, 3] for _, _, f in _cb('t3'))
    assert all(f['fwd_tiles'] == [3, 3, 3, 3] and f['bwd_tiles'] == [3, 3, 3, 4] for _, _, f in _cb('b4'))
    assert all(f['fwd_tiles'] == [4, 3, 3, 3] and f['bwd_tiles'] == [3, 3, 4, 4] for _, _, f in _cb('f1b2'))
    assert all(f['fwd_tiles'] == [4, 4, 3, 3] and f['bwd_tiles'] == [3, 4, 4, 4] for _, _, f in _cb('mt37') + _cb('fcap'))
    assert all(f['fwd_tiles'] == [4, 4, 4, 3] and f['bwd_tiles'] == [3, 4, 4, 4] for _, _, f in _cb('f3') + _cb('round2'))


def test_cases_sit_on_both_sides_of_each_boundary():
    mts = {m for _, _, f in _cb() for m in f['mt']}
    for lo, hi in ((16, 24), (25, 30), (31, 36), (37, 40)):
        assert any(lo <= m <= hi for m in mts), (lo, hi, sorted(mts))
    fwd = {f['mt'][0] for _, _, f in _cb()}
    assert any(m >= 41 for m in fwd) and any(41 <= m <= 42 for m in fwd) and any(43 <= m <= 46 for m in fwd) and 46 in fwd, sorted(fwd)
    # the predictor: T 128 / 129, and its row tiles on both sides of the conv block's boundaries too
    Ts = {sh['T'] for _, sh in t.PRED_CASES}
    assert {128, 129} <= Ts and any(T > 129 for T in Ts) and any(T < 7 for T in Ts), sorted(Ts)
    pm = {f['mt'] for _, _, f in _pred()}
    assert (16, 16) in pm and (41, 40) in pm and (40, 40) in pm and any(25 <= a <= 30 for a, _ in pm) and any(31 <= a <= 36 for a, _ in pm), sorted(pm)


def test_short_clip_cases_have_a_masked_tap_on_every_row_above_16_rows_per_workgroup():
    short = _cb('short')
    assert len(short) >= 5
    for _, sh, f in short:
        assert sh['T'] < 7 or sh['L'] < 7, sh
        assert f['mt'][0] + 24 >= 2 * (sh['T'] + 0)      # several clips inside one tile plus halo
    assert sum(f['mt'][0] > 16 for _, _, f in short) >= 4 and any(f['mt'] == (16, 16) for _, _, f in short)
    assert any(sh['T'] == 1 and sh['L'] == 1 for _, sh, _ in short)                     # every tap but the centre masked on every row
    assert any(sh['L'] == 1 and sh['T'] > 1 for _, sh, _ in short)                      # one-word queries next to real clips
    assert any(sh['T'] < 7 and sh['L'] < 7 and f['mt'][0] >= 36 for _, sh, f in short)  # dozens of clips per tile: 60 rows of 6 / 3
    assert any(f['mt'][0] > f['mt'][1] for _, _, f in short)                            # and across tiles of different height
    assert any(not f['ragged'][0] for _, sh, f in short if (sh['B'], sh['T'], sh['L']) == (1000, 5, 1))      # R % MT == 0 on purpose
    # the predictor's position-embedding index row - lo with every row at a clip edge
    assert any(sh['T'] < 7 for _, sh, _ in _pred('p_tiny')) and any(sh['T'] <= 8 and f['mt'][0] >= 31 for _, sh, f in _pred('p_four'))


def test_listed_cases_straddle_the_video_query_boundary_and_end_inside_a_tile():
    for cls, sh, f in _cb():
        if cls != 'short':
            assert f['straddle'][0] and f['ragged'][0], (cls, sh, f)
    assert all(f['straddle'] == (True, True) for _, _, f in _cb('t3'))
    assert sum(f['straddle'][1] for _, _, f in _cb()) >= 6
    assert any(f['straddle'][0] and not f['straddle'][1] for _, _, f in _cb())      # the boundary inside a forward tile, at the edge of a backward one


def test_forward_and_backward_tiles_differ_where_the_class_says_so():
    for cls, sh, f in _cb() + _pred():
        if cls in ('fcap', 'f3', 'round2', 'p_fcap'):
            assert f['mt'][0] > f['mt'][1] == t.CB_BWD_CAP, (cls, sh, f)
        elif cls != 'short':
            assert f['mt'][0] == f['mt'][1], (cls, sh, f)
    assert any(sh['L'] == 1 for _, sh, _ in _cb('fcap')) and any(sh['L'] == 3 and sh['T'] == 256 for _, sh, _ in _cb('mt37'))


def test_second_round_case_has_more_workgroups_than_compute_units():
    (_, sh, f), = _cb('round2')
    assert f['grid'][0][0] > 256 and f['grid'][1][0] > 256 and f['mt'] == (t.CB_FWD_CAP, t.CB_BWD_CAP), f
    # every other forward launch fits one round (its MT is the smallest that does)
    assert all(f['grid'][0][1] == 1 for c, _, f in _cb() if c != 'round2')


def test_predictor_cases_name_every_instantiation_of_their_families():
    syms = {s for _, sh in t.PRED_CASES for s in t.pred_dispatch(sh['B'], sh['T'])}
    assert {'heads_kernel<8>', 'heads_kernel<16>', 'attn_bwd_kernel', 'attn_bwd_big_kernel'} <= syms, sorted(syms)
    assert {'attn_fwd_kernel<2, 256>', 'attn_fwd_kernel<8, 512>', 'attn_fwd_kernel<16, 512>'} <= syms, sorted(syms)
    # ln_proj / ln_proj_pair at more than one row tile on a one-row-space launch, the pair at its cap of four
    for fam, nts in (('ln_proj_kernel<%d, true>', (1, 2, 3)), ('ln_proj_kernel<%d, false>', (1, 2, 3)), ('ln_proj_pair_kernel<%d>', (1, 4)),
                     ('ln_proj_bwd_kernel<true, %d>', (1, 2, 3)), ('ln_proj_bwd_kernel<false, %d>', (1, 2, 3))):
        assert {fam % n for n in nts} <= syms, (fam, sorted(syms))
    for cls, sh, f in _pred():
        if cls in ('p_ragged', 'p_fcap', 'p_max'):
            assert sh['T'] > 128 and t.attn1_bwd_form(sh['T']) == 'attn_bwd_big_kernel', sh
        if cls == 'p_ragged':
            assert f['ragged'] == (True, True) and sh['T'] % 16 != 0, f
        if cls == 'p_fcap':
            assert f['ln_proj'] == 41, f
        if cls == 'p_max':
            assert f['mt'] == (40, 40) and sh['T'] == 256, f


def test_every_class_runs_with_and_without_dropout():
    for table, runs in ((t.CB_TABLE, t.CB_RUNS), (t.PRED_TABLE, t.PRED_RUNS)):
        for cls, _, shapes in table:
            drops = [d for c, sh, d in runs if c == cls]
            assert drops.count(t.DROP) == len(shapes) and drops.count(0.0) >= 1, (cls, drops)
    assert set(t.M) == {c for c, _, _ in t.CB_TABLE + t.PRED_TABLE} and all(m <= t.CAP for m in t.M.values())
