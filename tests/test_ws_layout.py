"""The workspace layout is behaviour: every pointer a kernel receives is workspace base + an offset of this table, and the offsets
follow from the ORDER in which the forward and backward graphs first request their buffers (csrc/seqpan.hip).  A restructuring of the
host code must leave the table as it was - names, offsets, shapes, order and the total - so this test compares `lib.ws_table` /
`lib.query_workspace` with digests recorded from a build of an earlier commit (tests/ws_layout.json names it).

Re-recording (only when a change is MEANT to move the layout): build the commit that defines the layout, then
    python tests/test_ws_layout.py --write
which rewrites tests/ws_layout.json from the library of that checkout (HUAL_LIB_PATH picks another build)."""
import hashlib
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIGESTS = os.path.join(ROOT, 'tests', 'ws_layout.json')
BASE = dict(num_words=200, num_chars=30, max_vlen=256)
# name -> ((B, T, L, C), cfg overrides)
CASES = {
    'bench_64x128x20': ((64, 128, 20, 8), dict(vdim=1024)),
    'b16_t100_l79_c22': ((16, 100, 79, 22), {}),
    'b32_t256_l40': ((32, 256, 40, 8), {}),
    'wide_cq_l64': ((16, 100, 64, 8), {}),             # last query length of the wide on-chip context-query kernels (33-64 words)
    'wide_cq_l65': ((16, 100, 65, 8), {}),             # first one beyond them
    'single_clip': ((1, 1, 1, 4), {}),
    'vdim320_no_ksplit': ((16, 100, 20, 8), dict(vdim=320)),
    'attn_layer_1': ((16, 100, 20, 8), dict(attn_layer=1)),
    'attn_layer_3': ((16, 100, 20, 8), dict(attn_layer=3)),
    'finetune_word_emb': ((16, 100, 20, 8), dict(finetune_word_emb=1)),
    'gumbel': ((16, 100, 20, 8), dict(no_gumbel=0)),
    'no_gumbel': ((16, 100, 20, 8), dict(no_gumbel=1)),
}


def _digest(name):
    from hual_amd import lib
    shape, over = CASES[name]
    cfg = lib.make_cfg(**dict(BASE, **over))
    table = lib.ws_table(cfg, *shape)      # (a dict in table order)
    h = hashlib.sha256()
    for n, (off, rows, cols) in table.items():
        h.update(('%s %d %d %d\n' % (n, off, rows, cols)).encode())
    return {'entries': len(table), 'bytes': lib.query_workspace(cfg, *shape), 'sha256': h.hexdigest()}


@pytest.mark.parametrize('name', sorted(CASES))
def test_workspace_table_is_the_recorded_one(name):
    from hual_amd import build
    build.build()
    rec = json.load(open(DIGESTS))
    assert sorted(rec['cases']) == sorted(CASES), 'tests/ws_layout.json and CASES list different cases'
    got = _digest(name)
    print(name, got)
    assert got == rec['cases'][name], 'workspace layout of %s differs from the one commit %s had' % (name, rec['generated_from'])


if __name__ == '__main__':
    assert sys.argv[1:] == ['--write'], __doc__
    sys.path.insert(0, ROOT)
    commit = subprocess.check_output(['git', 'rev-parse', 'HEAD'], cwd=ROOT).decode().strip()
    dirty = subprocess.check_output(['git', 'status', '--porcelain', '--', 'hual_amd/csrc', 'include'], cwd=ROOT).decode().strip()
    assert not dirty, 'the library sources differ from the commit: record the layout from a clean checkout\n' + dirty
    rec = {'generated_from': commit,
           'what': 'per case: number of workspace entries, hual_seqpan_query_workspace bytes, sha256 over "name offset rows cols\\n" '
                   'of hual_seqpan_ws_table in table order',
           'cases': {n: _digest(n) for n in sorted(CASES)}}
    with open(DIGESTS, 'w') as fh:
        json.dump(rec, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print('wrote', DIGESTS, 'from', commit)
