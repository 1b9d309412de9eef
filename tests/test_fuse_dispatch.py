"""Host only: the case table of tests/test_gpu_fuse_forms.py names every class and switch point its restatement of the fuse stage's
dispatch (csrc/seqpan.hip fwd_fuse / bwd_fuse / run_block, csrc/heads.hip launch_pool_align_bwd / rowgrid, csrc/mproj.hip mproj_rows /
launch_mproj) tells apart - every instantiation, every row-tile count of the addend form, each boundary from both sides - and the
restated constants and conditions are the ones the sources hold: a change of the dispatch fails here first, a change of the restatement
or of the table cannot take a form out of coverage silently.  The composed oracle of the GPU test is held to R.forward here too (no GPU
needed for that)."""
import os
import re

import test_gpu_fuse_forms as t

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'hual_amd', 'csrc')


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _define(name, text):
    (v,) = re.findall(r'^#define %s (\d+)\b' % name, text, re.M)
    return int(v)


def _forms(cls=None):
    return [(c, sp, t.fuse_form(sp)) for c, sp in t.FUSE_CASES if cls in (None, c)]


# ---------------------------------------------------------------------------------------------------- the sources
def test_restated_constants_are_the_sources():
    h = _src('heads.hip')
    assert 'int match_fwd_blocks(int Nv) { return rowgrid(Nv, %d); }' % t.MATCH_FWD_CAP in h
    assert 'int match_bwd_blocks(int Nv) { return rowgrid(Nv, %d); }' % t.MATCH_BWD_CAP in h
    assert t.MP_ROWS == _define('MP_ROWS', _src('mproj.hip'))
    assert 'MPF_ADD == %d' % t.MPF_ADD in _src('mproj.hip') and 'case 3: MPROJ_NT(%d); break;       // addend' % t.MPF_ADD in _src('mproj.hip')


def test_restated_conditions_are_the_sources():
    """the very expressions the restatement mirrors: an edit of one of them fails here and asks for the restatement to follow"""
    h = _src('heads.hip')
    assert 'int g = cdiv(R, 8);' in h and 'return g < cap ? (g > 0 ? g : 1) : cap;' in h
    assert 'if (rs.T <= %d) {' % t.PAB_T in h
    lo = 'if (rs.L <= %d) PAB(%%d, 8); else if (rs.L <= %d) PAB(%%d, 16); else if (rs.L <= %d) PAB(%%d, 32); else PAB(64, 64);' % t.PAB_L
    assert lo % (32, 32, 32) in h and lo % (64, 64, 64) in h
    # the KT / KL table as instantiated: exactly the seven forms
    assert sorted(set(re.findall(r'PAB\((\d+), (\d+)\);', h))) == sorted((str(a), str(b)) for a, b in t.PAB_FORMS)
    assert 'const int row0 = min((int)blockIdx.x * 8 + grp, rs.Nv - 1);' in h and 'const int rn = min(row + (int)gridDim.x * 8, rs.Nv - 1);' in h
    assert 'const int t = min(grp + 4 * k, T - 1);' in h and 'rF[k] = pa.F2[(qrow0 + min(grp + 4 * k, L - 1)) * HUAL_D + c];' in h
    assert 'if (T <= 128) HUAL_LAUNCH(0.0, hb, heads_kernel<8>' in h and 'else HUAL_LAUNCH(0.0, hb, heads_kernel<16>' in h
    m = _src('mproj.hip')
    assert 'else { while (t < MP_ROWS && cdiv(R0, t) > 256) ++t; }' in m
    assert 'if (nt <= 2) MPROJ_LAUNCH(2, FS);' in m and 'else if (nt == 3) MPROJ_LAUNCH(3, FS);' in m
    assert 'addv[rt] = ld4((st.add && closes) ? st.add + (size_t)(row / st.add_div) * st.ldadd + ecol : wdummy);' in m
    sp = _src('seqpan.hip')
    assert 'pr.s[0].add = f.pool.PW; pr.s[0].ldadd = D; pr.s[0].add_div = c.T;' in sp
    assert 'const bool whole = c.sel_stage < 0 || (c.sel_stage == ST_FUSE && lab);' in sp
    assert 'if (opt->deferred_loss_terms && whole) {' in sp and 'if (!opt->align_external && whole) {' in sp
    assert 'c.chk(launch_match_fwd(ma, c.rs, (lab && !opt->align_external) ? &as : nullptr, c.stream));' in sp
    assert 'if (c.live()) c.chk(launch_pool_align_fwd(f.pool, lab ? &f.align : nullptr, c.rs, c.stream));' in sp
    # one definition of the close of the loss: the whole model and the labelled fuse block call the same function
    assert sp.count('launch_loss_tail(') == 1 and sp.count('close_loss(c, k, fu, b, out, opt)') == 2
    assert 'HUAL_REQUIRE(labels && labels->match_labels && labels->inner_labels, "hual_fuse_bwd: needs the labels of the forward call");' in sp


def test_restated_functions_at_their_boundaries():
    assert [t.mproj_rows(n) for n in (1, 4096, 4097, 8192, 8193, 12288, 12289, 10 ** 6)] == [16, 16, 17, 32, 33, 48, 49, t.MP_ROWS]
    assert [t.mproj_nt(m) for m in (16, 32, 33, 48, 49, 64)] == [2, 2, 3, 3, 4, 4]
    assert [t.rowgrid(n, 256) for n in (1, 8, 9, 2048, 2049, 10 ** 5)] == [1, 1, 2, 256, 256, 256]
    assert [t.pab_form(T, L) for T, L in ((128, 32), (128, 33), (128, 64), (128, 65), (128, 128), (128, 129), (129, 32), (129, 33), (129, 65),
                                          (129, 129), (1, 1), (256, 256))] == \
        [(32, 8), (32, 16), (32, 16), (32, 32), (32, 32), (64, 64), (64, 8), (64, 16), (64, 32), (64, 64), (32, 8), (64, 64)]


# ---------------------------------------------------------------------------------------------------- the case table
def test_every_pool_align_bwd_instantiation_and_switch_side():
    f = _forms('pab')
    assert sorted({x['pab'] for _, _, x in f}) == sorted(t.PAB_FORMS)
    shapes = {(sp['T'], sp['L']) for _, sp, _ in f}
    assert {(128, 32), (128, 33), (100, 64), (100, 65), (128, 128), (100, 129), (129, 32), (256, 33), (256, 65), (256, 128), (200, 256),
            (256, 256)} <= shapes
    # each switch point from both sides; every query-side switch with short and with long clips
    assert {sp['T'] for _, sp, _ in f} >= {t.PAB_T, t.PAB_T + 1}
    for lim in t.PAB_L:
        assert {lim, lim + 1} <= {sp['L'] for _, sp, _ in f}
        for long_clip in (False, True):
            assert {sp['L'] for _, sp, _ in f if (sp['T'] > t.PAB_T) == long_clip} & {lim, lim + 1}, (lim, long_clip)
    # row clamps: T and L below the four row groups, and no multiples of four
    clamp = {(sp['T'], sp['L']) for _, sp, _ in _forms('clamp')}
    assert {(3, 2), (1, 1), (5, 3)} <= clamp and any(T % 4 and L % 4 and T > 4 and L > 4 for T, L in clamp)
    # every labelled case predicts exactly one backward instantiation
    for _, sp, x in _forms():
        d = t.fuse_dispatch(sp)
        assert sum(v for k, v in d.items() if k.startswith('pool_align_bwd_kernel')) == (1 if sp['labels'] else 0)


def test_matching_head_grids():
    f = _forms('grid')
    assert any(x['Nv'] < 8 for _, _, x in f)
    assert any(x['Nv'] % 8 and 8 < x['Nv'] <= 8 * t.MATCH_BWD_CAP for _, _, x in f)
    for cap, key in ((t.MATCH_BWD_CAP, 'bwd_loops'), (t.MATCH_FWD_CAP, 'fwd_loops')):
        assert any(x['Nv'] == 8 * cap and not x[key] for _, _, x in f)                                       # the last shape without a loop
        assert any(8 * cap < x['Nv'] < 8 * cap + 64 and x['Nv'] % 8 and x[key] for _, _, x in f)              # its first stride step, ragged
    assert any(x['bwd_loops'] and not x['fwd_loops'] for _, _, x in f)


def test_every_row_tile_count_of_the_addend_form():
    f = _forms()
    assert {x['nt'] for _, _, x in f} == {2, 3, 4}
    syms = {s for _, sp in t.FUSE_CASES for s in t.fuse_dispatch(sp)}
    assert {'mproj_kernel<%d, %d>' % (nt, fs) for nt in (2, 3, 4) for fs in (t.MPF_ADD, 0)} <= syms
    assert {'pool_align_bwd_kernel<%d, %d>' % kk for kk in t.PAB_FORMS} <= syms
    tiles = _forms('tiles')
    nv = sorted(x['Nv'] for _, _, x in tiles)
    assert any(4096 < n <= 8192 for n in nv) and 8192 in nv and any(8192 < n < 8192 + 64 for n in nv) and 12288 in nv and any(12288 < n <= 12544 for n in nv)
    assert [x['nt'] for _, _, x in tiles if x['Nv'] in (8192, 12288)] == [2, 3]
    for _, sp, x in tiles:
        if x['nt'] > 2 and x['Nv'] not in (8192, 12288):
            assert x['straddle'] and sp['T'] % x['mt'], (sp, x)              # tiles that hold rows of two clips: the addend row changes inside a tile
    assert all(sp['B'] <= 64 and sp['L'] <= 8 for _, sp, _ in tiles)
    assert all(sp['B'] <= 64 for _, sp in t.FUSE_CASES)


def test_loss_forms_and_alignment_edges():
    loss = [sp for _, sp, _ in _forms('loss')]
    assert any(not sp['labels'] for sp in loss) and any(sp['ext'] and not sp['deferred'] for sp in loss)
    assert {bool(sp['drop']) for sp in loss if sp['gumbel'] and not sp['deferred']} == {True, False} and t.TAU != 1.0
    assert any(sp['denom'] > 0 for sp in loss) and any(sp['deferred'] and not sp['ext'] for sp in loss) and any(sp['deferred'] and sp['ext'] for sp in loss)
    for sp in loss:
        d = t.fuse_dispatch(sp)
        assert ('loss_tail_kernel' in d) == (sp['labels'] and not sp['deferred']) and ('match_bwd_kernel' in d) == sp['labels']
        assert ('align_sim_rows_kernel' in d) == sp['ext']
    align = [sp for _, sp, _ in _forms('align')]
    assert {1, 2} <= {sp['B'] for sp in align} and any(sp['B'] % 4 and sp['B'] > 4 for sp in align)
    assert {sp['edge'] for sp in align} == {None, 'dead', 'one'} and all(sp['dscale'] == 0.0 for sp in align)
    alone = [sp for _, sp, _ in _forms('alone')]
    assert all(sp['dscale'] == 0.0 and sp['lam'] == 0.0 for sp in alone) and {sp['ext'] for sp in alone} == {False, True}
    assert all(sp['lam'] == 1.0 for c, sp, _ in _forms() if c != 'alone')
    assert set(t.M) == {c for c, _, _ in t.FUSE_TABLE} | {'loc'} and all(m <= t.CAP for m in t.M.values())
    assert len({(cls, t._id(sp)) for cls, sp in t.FUSE_CASES}) == len(t.FUSE_CASES)
    assert t.LOC_T == [1, 5, 128, 129, 256]


def test_case_batches_hold_what_they_are_there_for():
    for cls, sp in t.FUSE_CASES:
        if sp['B'] * sp['T'] > 2048 and sp['edge'] is None:
            continue                                                             # (the same construction at more rows)
        cfg, p, wv, b, labels = t.make_case(sp)
        lens, inner, words = b['lens'].long(), labels[3], (b['word_ids'] != 0).sum(1)
        assert int(lens.max()) == sp['T'] and int(words.max()) == sp['L'] and int(lens.min()) >= 1 and int(words.min()) >= 1
        assert cfg.no_gumbel == (not sp['gumbel'])
        for k in range(sp['B']):
            live = float(inner[k, :lens[k]].sum())
            assert float(inner[k, lens[k]:].sum()) == 0.0 and (live == 0.0) == (sp['edge'] == 'dead' and k == 1), (sp, k)
        if sp['edge'] == 'one':
            assert int(lens[1]) == 1 and int(words[1]) == 1


def test_localizing_cases_hold_what_they_are_there_for():
    for T in t.LOC_T:
        s, e, mask, y1, y2 = t.loc_case(T, 31)
        lens = mask.sum(1)
        assert int(lens.max()) == T and int(lens.min()) == 1 and float((y1 * (1 - mask)).abs().max()) == 0.0
        sums = y1.sum(1)
        assert float(sums[3]) == 0.0 and float(y2[3].abs().max()) == 0.0 and abs(float(sums[0]) - 0.2) < 1e-5 and abs(float(sums[2]) - 3.0) < 1e-5
        o, s_part = t.loc_oracle(s, e, mask, y1, y2, t.torch.float64)
        assert bool(t.torch.isfinite(o['ds']).all()) and float(o['loc_part'][3]) == 0.0


# ---------------------------------------------------------------------------------------------------- the oracle
def test_composed_oracle_is_the_reference_forward():
    t.prove_composition()
