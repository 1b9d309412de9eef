"""The round policy of update_labels as a table: which combinations of its switches reach the device and which are refused.

al_policy_outcomes.txt holds one character per combination of the twelve axes below, in itertools.product order ('1' = reached the
device, '0' = refused with ValueError), recorded from update_labels before its validation was gathered into al.check_round."""
import copy
import itertools
import os

from hual_amd import al

AXES = (('posterior', ('deterministic', 'ensemble')),
        ('rank_by', ('uncert_video', 'span_risk', 'span_bald')),
        ('observe_by', ('uncert_frame', 'info_gain')),
        ('renew_by', ('heuristic', 'posterior')),
        ('acquire_by', (None, 'label_gain')),
        ('soft_out', (None, {})),
        ('questions_per_clip', (1, 3)),
        ('stop_entropy', (None, 1.0)),
        ('answer_noise', (None, 0.1)),
        ('temperature', (None, 2.0)),
        ('calibrate', (None, 'evidence')),
        ('bank', (None, 'stub')))
ACCEPTED = 633


class _Bank:
    K = Kmax = 3
    pass_s = object()


class _Reached(Exception):
    pass


def combinations():
    for values in itertools.product(*(v for _, v in AXES)):
        kw = dict(zip((n for n, _ in AXES), values))
        kw['bank'] = _Bank() if kw['bank'] == 'stub' else None
        kw['soft_out'] = None if kw['soft_out'] is None else {}
        yield kw


def outcomes(update_labels):
    """-> (the '0' / '1' string, the refusals that were no ValueError, the refusals that touched data_old)"""
    data = [['v0', 10.0, [1.0, 4.0], 'a'], ['v1', 8.0, [2.0, 6.0], 'b']]
    prop = [{'vid': 'v0', 'v_len': 20, 'prop_conf': 0.5}, {'vid': 'v1', 'v_len': 16, 'prop_conf': 0.25}]
    coff = al.get_coff('charades', 1)
    out, wrong_type, touched = [], [], []
    for kw in combinations():
        old = copy.deepcopy(data)
        try:
            update_labels(old, copy.deepcopy(data), prop, coff, **kw)
            raise AssertionError('update_labels returned without a device')
        except _Reached:
            out.append('1')
            continue
        except ValueError:
            pass
        except Exception as exc:                                 # noqa: BLE001 (reported below, with its combination)
            wrong_type.append((kw, repr(exc)))
        out.append('0')
        if old != data:
            touched.append(kw)
    return ''.join(out), wrong_type, touched


def test_update_labels_accepts_and_refuses_what_it_did(monkeypatch):
    def reached(*a, **k):
        raise _Reached()
    monkeypatch.setattr(al.LabelUpdater, '__init__', reached)
    monkeypatch.setattr(al.LabelUpdater, 'from_bank', reached)
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'al_policy_outcomes.txt')) as f:
        want = f.read().strip()
    got, wrong_type, touched = outcomes(al.update_labels)
    assert len(want) == len(got) == 6144
    differ = [i for i in range(6144) if want[i] != got[i]]
    print('%d combinations, %d accepted, %d differ from the record' % (len(got), got.count('1'), len(differ)))
    assert not wrong_type, wrong_type[:3]
    assert not touched, touched[:3]
    assert got == want, [kw for i, kw in enumerate(combinations()) if i in differ[:3]]
    assert got.count('1') == ACCEPTED
