"""Host only: the case table of tests/test_gpu_input_forms.py names every class of form its restatement of the input stage's dispatch
(csrc/seqpan.hip setup_ctx / fwd_input / bwd_input, csrc/gemm.hip launch_feature_ksplit, csrc/embed.hip launch_embed_fwd / _bwd,
csrc/mproj.hip mproj_rows / launch_mproj) tells apart, and the restated constants and conditions are the ones the sources hold - a
change of the dispatch fails here first, a change of the restatement or of the table cannot take a form out of coverage silently.  The
composed oracle of the GPU test is held to R.forward here too (no GPU needed for that)."""
import os
import re

import torch

import test_gpu_input_forms as t
from oracle import seqpan_ref as R

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'hual_amd', 'csrc')


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _define(name, text):
    (v,) = re.findall(r'^#define %s (\d+)\b' % name, text, re.M)
    return int(v)


def _forms(cls=None):
    return [(c, sp, t.input_form(sp)) for c, sp in t.IN_RUNS if cls in (None, c)]


# ---------------------------------------------------------------------------------------------------- the sources
def test_restated_constants_are_the_sources():
    assert t.MP_ROWS == _define('MP_ROWS', _src('mproj.hip')) and t.MP_MAX == _define('MP_MAX', _src('mproj.h'))
    assert t.NALL == _define('NALL', _src('embed_gather.h')) and t.NCH == _define('NCH', _src('embed_gather.h'))
    assert t.DW_JOBS == _define('HUAL_MAX_DW_JOBS', _src('gemm.h'))
    assert 'static inline int cpad(int char_dim) { return (char_dim + 15) / 16 * 16; }' in _src('embed.hip')
    assert [t.cpad(c) for c in (1, 16, 17, 20, 50, 100)] == [16, 16, 32, 32, 64, 112]


def test_restated_conditions_are_the_sources():
    """the very expressions the restatement mirrors: an edit of one of them fails here and asks for the restatement to follow"""
    sp = _src('seqpan.hip')
    assert 'c.ksplit = (cfg->vdim % 256) == 0 && cfg->vdim <= 1024 && (catw % 8) == 0 && qks <= 256;' in sp
    assert sp.count('const int qks = ((catw + 3) / 4 + 63) & ~63;') == 2
    assert 'int catw() const { return cfg->word_dim + 100; }' in sp
    assert 'const bool pos_rides = c.sel_stage < 0;' in sp
    assert 'c.chk(launch_embed_bwd(ea, eg, Nq, c.drop, c.stream, &embed_dw, false));' in sp      # the last embed step rides in colsum_kernel
    g = _src('gemm.hip')
    assert 'const double m16 = frexp((double)((j.drop_site >= 0 && drop.enabled) ? drop.scale : 1.0f), &e) * 16.0;' in g
    assert 'b.j[i].a_bf16 = (m16 == floor(m16)) ? 2 : 1;' in g
    e = _src('embed.hip')
    assert 'const int mtp = (g.MT + C - 1) / C * C;' in e and 'if ((C & (C - 1)) == 0 && C <= 16 && mtp <= 64) {' in e
    assert 'g.R = nrows * a.C; g.MT = mproj_rows(g.R); g.nsteps = 1;' in e and 'st.rep = cdiv(4 * CP, 128);' in e
    assert 'j.R = M; j.MT = mproj_rows(M); j.nsteps = cdiv(4 * CP, 128);' in e
    m = _src('mproj.hip')
    assert 'if (R1 > 0) { while (t < MP_ROWS && mproj_pair_grid(R0, R1, t) > 256) ++t; }' in m
    assert 'else { while (t < MP_ROWS && cdiv(R0, t) > 256) ++t; }' in m and 'inline int mproj_pair_lo(int nb, int x) { return nb * x / 8; }' in m
    assert 'if (nt <= 2) MPROJ_LAUNCH(2, FS);' in m and 'else if (nt == 3) MPROJ_LAUNCH(3, FS);' in m
    assert 'case 1: MPROJ_NT(32); break;' in m and 'case 7: MPROJ_NT(128); break;' in m and 'default: MPROJ_NT(63); break;' in m


def test_restated_functions_at_their_boundaries():
    assert [v for v in range(64, 1281, 64) if t.ksplit(v)] == [256, 512, 768, 1024]
    assert [t.a_bf16(True, r) for r in (0.0, 0.2, 0.5, 0.1, 0.3)] == [2, 2, 2, 1, 1] and t.a_bf16(False, 0.1) == 0
    assert t.mproj_rows(4096) == 16 and t.mproj_rows(4097) == 17 and t.mproj_rows(10 ** 6) == t.MP_ROWS
    assert t.mproj_rows(60, 18) == 16 and t.mproj_rows(3850, 350) > 16
    assert [t.mproj_nt(m) for m in (16, 32, 33, 48, 49, 64)] == [2, 2, 3, 3, 4, 4]
    assert [t.char_steps(c) for c in (20, 32, 33, 50, 64, 65, 100)] == [1, 1, 2, 2, 2, 3, 4] and t.char_steps(100) <= t.MP_MAX
    assert [t.pool_epilogue(18, C)[0] for C in (4, 5, 8, 12, 16, 32)] == [True, False, True, False, True, False]


# ---------------------------------------------------------------------------------------------------- the case table
def test_every_class_of_form_has_a_case():
    f = _forms()
    # 1. feature load: both paths, every quarter size
    assert {x['quarter'] for _, _, x in f if x['ksplit']} == {64, 128, 192, 256}
    assert any(not x['ksplit'] and x['part_k'] and sp['vdim'] > 128 for _, sp, x in f)      # full weight blocks, then a partial one
    assert any(not x['ksplit'] and sp['vdim'] < 128 for _, sp, x in f)                      # one block, narrower than 128
    # 2. bfloat16: both forms in the K-split kernel at the smallest and the largest quarter, once on the pair path
    for q in (64, 256):
        assert {x['a_bf16'] for _, _, x in f if x['ksplit'] and x['quarter'] == q} == {0, 1, 2}
    assert any(x['a_bf16'] and not x['ksplit'] for _, _, x in f)
    assert all(sp['rate'] in (0.0, 0.1, t.DROP) for _, sp, _ in f)
    # 3. char CNN: 1, 2 and 4 weight steps; epilogue and stored tile, pairwise; above 4096 window rows
    assert {x['char_steps'] for _, _, x in _forms('char')} == {1, 2, 4} and not any(x['pool'] for _, _, x in _forms('char'))
    pool = _forms('pool')
    assert sorted({sp['C'] for _, sp, x in pool if x['pool']}) == [4, 8, 16] and sorted({sp['C'] for _, sp, x in pool if not x['pool']}) == [5, 12, 32]
    big = [(sp, x) for _, sp, x in pool if sp['B'] * sp['L'] * sp['C'] > 4096]
    assert big and all(x['pool'] and x['mt_win'] > 16 and x['mt_char'] % sp['C'] == 0 and x['mt_char'] > x['mt_win'] and x['char_ragged'] for sp, x in big)
    # 4. query projection: four K-blocks, the last 16 wide
    assert all(x['q_steps'] == 4 and x['q_last'] == 16 for _, _, x in f)
    # 5. word rows: frozen and fine-tuned
    assert sorted(sp['words'] for _, sp, _ in _forms('words') if sp['rate']) == ['finetune', 'frozen']
    # 6. the per-block call: the position table's launch and the riding embed step are in every case's prediction
    for _, sp, _ in f:
        d = t.input_dispatch(sp)
        assert d['pos_bwd_kernel'] == d['ln_bwd_kernel'] == d['colsum_kernel'] == 1 and 'ln_pos_bwd_kernel' not in d and 'embed_finish_kernel' not in d
    # rows: above 256 x 16 rows on both feature paths, ragged against 16 and against the pair's tile
    rows = _forms('rows')
    assert {x['ksplit'] for _, _, x in rows} == {True, False} and all(x['R'] > 4096 and x['R'] % 16 for _, _, x in rows)
    assert all(x['mt_pair'] > 16 and (sp['B'] * sp['T']) % x['mt_pair'] for _, sp, x in rows if not x['ksplit'])
    # edges: one row of each kind; T = L = max_vlen
    edges = [sp for _, sp, _ in _forms('edges')]
    assert any((sp['B'], sp['T'], sp['L'], sp['C']) == (1, 1, 1, 4) for sp in edges) and any(sp['T'] == sp['L'] == sp.get('max_vlen') for sp in edges)


def test_predicted_symbols_cover_every_instantiation_the_stage_reaches_at_these_sizes():
    syms = {s for _, sp in t.IN_RUNS for s in t.input_dispatch(sp)}
    want = {'feature_ksplit_kernel', 'ln_fwd_kernel', 'mproj_pair_kernel<2, 63>', 'mproj_kernel<2, 128>', 'mproj_kernel<2, 0>', 'char_pool_kernel',
            'mproj_kernel<2, 32>', 'char_pool_bwd_kernel', 'pos_bwd_kernel', 'ln_bwd_kernel', 'dw_f16_balanced_kernel', 'colsum_kernel'}
    assert want <= syms, sorted(want - syms)
    # the one-step and the several-step window-gradient product
    assert any(t.input_dispatch(sp).get('mproj_kernel<2, 0>') == 2 for _, sp in t.IN_RUNS)                          # stored tile forward + one column block
    assert any(t.input_dispatch(sp).get('mproj_kernel<2, 32>') == 2 for _, sp in t.IN_RUNS)                         # d cat + several column blocks


def test_every_class_runs_with_and_without_dropout():
    for cls, _, cases in t.IN_TABLE:
        rates = [sp['rate'] for c, sp in t.IN_RUNS if c == cls]
        assert len(rates) == len(cases) + 1 and rates.count(0.0) >= 1 and rates.count(t.DROP) >= len(cases) - 3, (cls, rates)
    assert set(t.M) == {c for c, _, _ in t.IN_TABLE} and all(m <= t.CAP for m in t.M.values())
    assert len({(cls, t._id(sp)) for cls, sp in t.IN_RUNS}) == len(t.IN_RUNS)


def test_words_batch_holds_what_it_is_there_for():
    for _, sp in t.IN_CASES:
        if sp.get('words'):
            cfg, p, wv, b, labels = t.make_case(sp)
            w, ch = b['word_ids'], b['char_ids']
            assert int((w == 1).sum()) >= 2 and int((w[:, -1] == 0).sum()) >= 1 and int((w > 0).sum(1).min()) == 1
            assert int(((ch == 0).all(-1) & (w > 1)).sum()) >= 2 and len(set(w[w > 1].tolist())) < int((w > 1).sum())       # repeated words


# ---------------------------------------------------------------------------------------------------- the oracle
def test_composed_oracle_is_the_reference_forward():
    """float32, dropout on, the oracle's own max-pool: x0 of the composition is R.forward's cb.x0 tap, bit for bit"""
    for sp in (t.IN_CASES[0][1], [sp for _, sp in t.IN_CASES if sp.get('words') == 'frozen'][0]):
        cfg, p, wv, b, labels = t.make_case(sp)
        x0 = t.compose(p, wv, b, t.oracle_rng(t.DROP))
        out = R.forward(p, cfg, wv, b['video'], b['lens'], b['word_ids'], b['char_ids'], drop_rate=t.DROP, seed=t.SEED, offset=t.OFFSET, want_tap=True)
        B, T, L = sp['B'], sp['T'], sp['L']
        assert torch.equal(x0, torch.cat([out['tap']['cb.x0.v'].reshape(B * T, 128), out['tap']['cb.x0.q'].reshape(B * L, 128)]))
