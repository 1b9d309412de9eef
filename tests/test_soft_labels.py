"""CPU: hual_al_span_marginals (the start / end marginals of the span posterior given the answered active points) and the soft-label
assembly entry points hual_assemble_batch_soft / hual_assemble_batch_cursor_soft are declared, exported and refuse bad arguments
before any HIP call; al.update_labels / al.run_round refuse a bad soft_out / soft_labels before they touch anything; and the float64
reference the GPU tests compare against (tests/soft_label_ref.py) has the properties that define the quantity - on the very cases the
GPU tests use (al_query_ref.case: T in {2, 33, 70, 256}, 16 rows, after 0, 1, 3 and 6 truthful answers)."""
import copy
import ctypes
import os
import re
import types

import numpy as np
import pytest

import al_query_ref as Q
import soft_label_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('hual_al_span_marginals', 'hual_assemble_batch_soft', 'hual_assemble_batch_cursor_soft')


def test_symbols_are_declared_and_exported():
    from hual_amd import build, lib
    build.build()
    src = open(os.path.join(ROOT, 'include', 'hual_seqpan.h')).read()
    so = ctypes.CDLL(lib.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r'\bint %s\s*\(' % name, src), name
        assert hasattr(so, name), 'missing export ' + name
    assert re.search(r'typedef struct hual_soft_labels\s*\{', src)
    assert lib.load().hual_abi_version() == lib.ABI_VERSION == 9          # new symbols, the ABI version stays
    assert callable(lib.al_span_marginals)
    assert ctypes.sizeof(lib.hual_soft_labels) == 32


def _fails(l, rc, msg, what):
    assert rc == -1 and msg in l.hual_last_error(), (what, msg, rc, l.hual_last_error())      # HUAL_ERR_INVALID


def test_marginals_refuse_bad_arguments_without_a_gpu():
    from hual_amd import lib
    l = lib.load()
    buf = ctypes.create_string_buffer(64)
    a = ctypes.addressof(buf)
    p = ctypes.c_void_p(a)
    SET = ('vlen', 'tlen', 'ap_off', 'ap_idx', 'ap_pos')

    def aset(N=4, ld=64, **null):
        f = {k: a for k in SET}
        f.update(null)
        return ctypes.byref(lib.hual_al_set(N, ld, *[f[k] for k in SET]))

    def call(s=None, s0=p, e0=p, ys=p, ye=p, st=p, _null_set=False):
        return l.hual_al_span_marginals(None if _null_set else (s or aset()), s0, e0, ys, ye, st, None)
    for kw, msg in ((dict(_null_set=True), b'null set'), (dict(s0=None), b'null input'), (dict(e0=None), b'null input'),
                    (dict(s=aset(vlen=None)), b'null input'), (dict(s=aset(tlen=None)), b'null input'),
                    (dict(s=aset(ap_off=None)), b'null input'), (dict(s=aset(ap_idx=None)), b'null input'),
                    (dict(s=aset(ap_pos=None)), b'null input'),
                    (dict(ys=None), b'null output'), (dict(ye=None), b'null output'), (dict(st=None), b'null output'),
                    (dict(s=aset(N=0)), b'N > 0'), (dict(s=aset(N=-2)), b'N > 0'), (dict(s=aset(ld=1)), b'2 <= ld'),
                    (dict(s=aset(ld=1025)), b'ld <= 1024')):
        rc = call(**kw)
        _fails(l, rc, msg, kw)
        assert b'al_span_marginals' in l.hual_last_error()
    with pytest.raises(lib.HualError):
        lib.check(rc)


@pytest.mark.parametrize('cursor', [False, True])
def test_soft_assembly_refuses_bad_arguments_without_a_gpu(cursor):
    from hual_amd import lib
    l = lib.load()
    buf = ctypes.create_string_buffer(64)
    a = ctypes.addressof(buf)
    p = ctypes.c_void_p(a)
    name = b'hual_assemble_batch_cursor_soft' if cursor else b'hual_assemble_batch_soft'
    DS = ('feat_bank', 'feat_off', 'vdim', 'sample_vid', 'word_off', 'word_bank', 'char_off', 'char_bank', 's_ind', 'e_ind')

    def ds(**kw):
        f = {k: a for k in DS}
        f['vdim'] = 8
        f.update(kw)
        return ctypes.byref(lib.hual_dataset(*[f[k] for k in DS]))

    def soft(y1=a, y2=a, w=a, ld=8):
        return ctypes.byref(lib.hual_soft_labels(y1, y2, w, ld))

    def call(d='ds', sel=p, cur=p, B=2, T=4, L=3, C=4, video=p, lens=p, wi=p, ci=p, y1=p, y2=p, m=p, inn=p, carry=(None, None, 0), s='soft'):
        d = ds() if d == 'ds' else d
        s = soft() if s == 'soft' else s
        if cursor:
            return l.hual_assemble_batch_cursor_soft(d, sel, cur, B, T, L, C, video, lens, wi, ci, y1, y2, m, inn, s, None)
        return l.hual_assemble_batch_soft(d, sel, B, T, L, C, video, lens, wi, ci, y1, y2, m, inn, *carry, s, None)
    cases = [(dict(d=None), b'null dataset'),
             (dict(s=None), name + b': null soft labels'),
             (dict(s=soft(y1=None)), name + b': null soft->y1, soft->y2 or soft->w'),
             (dict(s=soft(y2=None)), name + b': null soft->y1, soft->y2 or soft->w'),
             (dict(s=soft(w=None)), name + b': null soft->y1, soft->y2 or soft->w'),
             (dict(s=soft(ld=0)), name + b': soft->ld >= 1'),
             (dict(y1=None, y2=None, m=None, inn=None), name + b': soft labels need the label feeds'),
             # those of the plain entry points, behind the banks
             (dict(d=ds(feat_bank=None)), b'assemble: null dataset pointer'), (dict(sel=None), b'assemble: null dataset pointer'),
             (dict(video=None), b'assemble: null output pointer'), (dict(ci=None), b'assemble: null output pointer'),
             (dict(B=0), b'assemble: bad shape'), (dict(d=ds(vdim=6)), b'assemble: bad shape'),
             (dict(y2=None), b'assemble: labels need'), (dict(d=ds(s_ind=None)), b'assemble: labels need')]
    if cursor:
        cases.append((dict(cur=None), b'null dataset / cursor'))
    else:
        cases += [(dict(carry=(None, None, 3)), b'assemble: carry needs'), (dict(carry=(p, p, -1)), b'assemble: carry needs')]
    for kw, msg in cases:
        _fails(l, call(**kw), msg, kw)


def _train_lists():
    data_old = [['v0', 10.0, [1.0, 2.0], 'a b'], ['v1', 12.0, [3.0, 4.0], 'c d']]
    return data_old, copy.deepcopy(data_old)


def test_update_labels_refuses_a_bad_soft_out():
    from hual_amd import al
    data_old, keep = _train_lists()
    for bad in ([], 'y1', 0.5):
        with pytest.raises(ValueError, match='soft_out'):
            al.update_labels(data_old, copy.deepcopy(data_old), [{'vid': 'v0'}, {'vid': 'v1'}], al.get_coff('charades', 1), soft_out=bad)
    assert data_old == keep


def test_run_round_refuses_bad_soft_labels(monkeypatch):
    from hual_amd import al, dist

    class Untouchable:
        vlen_h = np.array([20, 24], dtype=np.int32)

        def __getattr__(self, k):                                       # anything beyond the clip lengths: the round has started
            raise AssertionError('the dataset was touched: ' + k)
    ds = Untouchable()
    prop = [{'vid': 'v0', 'v_len': 20}, {'vid': 'v1', 'v_len': 24}]
    data_old, keep = _train_lists()

    def run(soft_labels, last_prop=prop):
        return al.run_round(None, ds, data_old, copy.deepcopy(data_old), last_prop, 'charades', 1, 1, 2, 1e-4, 0.2, soft_labels=soft_labels)
    for lam in (0.0, -0.5, 1.5, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='soft_labels'):
            run(lam)
    with pytest.raises(ValueError, match='v_len'):
        run(0.5, [{'vid': 'v0', 'v_len': 20}, {'vid': 'v1', 'v_len': 23}])
    monkeypatch.setattr(dist, 'world_size', lambda: 2)
    with pytest.raises(ValueError, match='single-process'):
        run(0.5)
    assert data_old == keep


def test_the_host_fed_path_refuses_soft_labels():
    from hual_amd import feeder, runner
    with pytest.raises(ValueError, match='soft labels'):
        feeder.HostFeeder.feed_records(None, [], {}, 1e-4, 0.2, soft_labels=(None, None, None))
    r = types.SimpleNamespace(feed='host', train_set=None)
    with pytest.raises(ValueError, match='soft labels'):
        runner.Runner.set_soft_labels(r, None, None, None)


# ---------------------------------------------------------------------------------------------------------------------
# the reference's own properties
@pytest.mark.parametrize('T', Q.TS)
def test_reference_marginal_properties(T):
    c = S.case(T)
    collapsed = modes_differ = 0
    for h in Q.HISTORIES:
        for n in range(Q.N_ROWS):
            r, v, aps = c['mref'][h][n], int(c['v'][n]), c['aps'][h][n]
            assert r['status'] == S.LIVE, (T, h, n)                     # a truthful annotator never contradicts itself
            ys, ye = r['y_start'], r['y_end']
            assert ys.shape == ye.shape == (v,) and ys.min() >= 0 and ye.min() >= 0
            assert abs(ys.sum() - 1.0) <= 1e-12 and abs(ye.sum() - 1.0) <= 1e-12
            assert np.abs(S.incl_from_marginals(r) - c['ref'][h][n]['incl']).max() <= 1e-12
            pos = [f for f, is_pos in aps if is_pos]
            neg = [f for f, is_pos in aps if not is_pos]
            if pos:
                assert (ys[min(pos) + 1:] == 0).all() and (ye[:max(pos)] == 0).all()
            for f in neg:
                assert ys[f] == 0 and ye[f] == 0
            ps = np.asarray(c['ps'][n][:v], dtype=np.float64)
            if h == 0 and v > 1:
                assert np.abs(ys - ps).max() > 1e-6                     # not the model's softmax: i <= j moves mass to early starts
            modes_differ += int(np.argmax(ys)) != int(np.argmax(ps))
            if int((Q.consistent(v, aps)).sum()) == 1:                  # collapsed: one-hot rows
                collapsed += 1
                assert sorted(ys)[-1] == 1.0 and sorted(ye)[-1] == 1.0 and (ys > 0).sum() == 1 and (ye > 0).sum() == 1
            if v == 1:
                assert ys[0] == 1.0 and ye[0] == 1.0
    assert collapsed > 0
    assert modes_differ > 0 or T == 2


def test_reference_edge_rules():
    c = Q.case(33)
    ps, pe = c['ps'][0], c['pe'][0]
    r = S.marginals_ref(ps, pe, 33, [(5, True), (9, True), (7, False)])       # a negative inside the positive hull
    assert r['status'] == S.CONTRADICTORY and not r['y_start'].any() and not r['y_end'].any() and r['y_start'].shape == (33,)
    assert S.marginals_ref(ps, pe, 3, [(0, False), (1, False), (2, False)])['status'] == S.CONTRADICTORY      # every frame negative
    assert S.marginals_ref(ps, pe, 0, [])['status'] == S.POISONED
    nan = S.marginals_ref(ps, pe, 33, [], nan_logit=True)
    assert nan['status'] == S.POISONED and not nan['y_start'].any() and not nan['y_end'].any()
    a, b = S.marginals_ref(ps, pe, 20, [(4, True)]), S.marginals_ref(ps, pe, 20, [(4, True), (20, False), (-1, True), (33, True)])
    assert (a['y_start'] == b['y_start']).all() and (a['y_end'] == b['y_end']).all()      # an active point outside [0, v) is ignored
    one = S.marginals_ref(ps, pe, 20, [(3, False), (4, True), (5, False)])    # one consistent span: collapsed, not an error
    assert one['status'] == S.LIVE and one['y_start'][4] == 1.0 and one['y_end'][4] == 1.0
    assert one['y_start'].sum() == 1.0 and one['y_end'].sum() == 1.0
    v1 = S.marginals_ref(ps, pe, 1, [])
    assert v1['status'] == S.LIVE and v1['y_start'].tolist() == [1.0] and v1['y_end'].tolist() == [1.0]


def test_the_numpy_blend_is_three_float32_roundings():
    g = np.random.default_rng(5)
    r, b = g.random(64, dtype=np.float32), g.random(64, dtype=np.float32)
    for lam in (0.25, 0.3, 1.0):
        got = S.blend(r, b, lam, 40)
        d = (b[:40].astype(np.float64) - r[:40]).astype(np.float32)
        m = (np.float64(np.float32(lam)) * d).astype(np.float32)
        want = (r[:40].astype(np.float64) + m).astype(np.float32)
        assert got.dtype == np.float32 and (got[:40].view(np.int32) == want.view(np.int32)).all() and (got[40:] == r[40:]).all()
    nan = np.full(64, np.nan, dtype=np.float32)
    assert (S.blend(r, nan, 0.0, 40).view(np.int32) == r.view(np.int32)).all()      # weight 0: the bank is not read
