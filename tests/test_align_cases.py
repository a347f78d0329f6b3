"""The alignment cases and their goldens without a GPU: the inputs still hash to what the
reference saw, the numpy restatement of include/ftmi.h's alignment semantics (tests/align_cases.py)
reproduces the reference on them, each planted defect changes a named case, and the public
surface (argument errors, create_align_features' file layout, header / binding agreement)."""
import ctypes
import pickle
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import align_cases as ac
from conftest import load_golden
from forwardtacotron_amd import _lib, align, ops

HEADER = Path(__file__).resolve().parent.parent / 'include' / 'ftmi.h'
ALIGN_FUNCS = ('ftmi_align_workspace_bytes', 'ftmi_align_dijkstra', 'ftmi_align_count',
               'ftmi_attention_score')
TIE_CASES = {'onehot_skip'}


@pytest.fixture(scope='module')
def gold():
    return load_golden('goldens_align')


@pytest.fixture(scope='module')
def cases():
    return ac.duration_cases()


@pytest.fixture(scope='module')
def restated(cases):
    return {n: ac.durations_dp(c['att'], c['mel_len'], c['x_len']) for n, c in cases.items()}


def test_inputs_hash_to_the_goldens(gold, cases):
    for n, c in cases.items():
        assert ac.sha(c['att']) == str(gold[f'sha/{n}']), n
    assert ac.sha(ac.batch_case(cases)['att']) == str(gold['sha/batch'])
    assert ac.sha(ac.score_case()) == str(gold['sha/scores'])


def test_case_list_covers_the_shapes(cases):
    shapes = {(c['mel_len'], c['x_len']) for c in cases.values()}
    assert {(1, 1), (1, 5), (7, 1), (3, 9), (37, 11), (40, 63), (40, 64), (40, 65), (40, 129),
            (600, 130), (40, 512), (30, 12)} <= shapes
    long = cases['long_600x130']
    assert long['att'].shape[0] == 640 and long['ld_row'] == 136 and ac.strided(long).shape == (640, 136)
    assert cases['wide_40x512']['att'].shape[1] == 512
    for c in cases.values():  # padding that would be noticed
        assert c['att'].shape[0] > c['mel_len'] and c['att'].dtype == np.float32
    b = ac.batch_case(cases)
    assert len(b['mel_len']) == 5 and 1 in b['x_len'] and len(set(b['x_len'])) == 5


def test_only_the_named_case_is_tied(cases, restated):
    tied = {n for n, (_, _, unique) in restated.items() if not unique}
    assert tied == TIE_CASES == {n for n, c in cases.items() if c['tied']}


def test_restatement_equals_reference(gold, cases, restated):
    """Unique-path cases: the reference's durations exactly and scipy's distance bit for bit.
    The tie case: the same under the diagonal-first rule."""
    for n, c in cases.items():
        dur, cost, _ = restated[n]
        assert np.array_equal(dur, gold[f'dij/{n}']), n
        assert cost == float(gold[f'cost/{n}']), n
        assert dur.sum() == c['mel_len'] and not dur[c['x_len']:].any(), n
        cnt = ac.durations_count(c['att'], c['mel_len'], c['x_len'])
        assert np.array_equal(cnt, gold[f'cnt/{n}']) and cnt.sum() == c['mel_len'], n
    assert (restated['deg_3x9'][0][:9] == 0).any()  # more tokens than frames
    assert np.array_equal(restated['onehot_skip'][0][:4], [1, 1, 1, 1])  # no token left empty
    assert restated['ones_path'][1] == 0.0 and restated['onehot_stay'][1] == 0.0


def test_scores_restatement_equals_reference(gold):
    att = ac.score_case()
    assert att.shape == (3, 50, 20)
    for r in ac.SCORE_R:
        ml = ac.SCORE_MEL_LENS[r]
        assert ml[0] // r == 50 and (r == 1 or all(m % r for m in ml))
        loc, sharp = ac.scores(att, ml, r)
        assert np.array_equal(loc, gold[f'loc64/{r}'])
        assert np.abs(sharp - gold[f'sharp64/{r}']).max() <= 2.0 ** -50
        assert np.array_equal(loc.astype(np.float32), gold[f'loc32/{r}'])
        drift = np.abs(gold[f'sharp32/{r}'] - gold[f'sharp64/{r}'])
        assert drift.max() < 1e-6  # the fp32 reference is an fp32 rounding or two away


@pytest.mark.parametrize('defect,name', [
    ('no_diag', 'soft05_37x11'), ('src_weight', 'soft05_37x11'), ('first_col', 'deg_3x9'),
    ('read_pad_rows', 'soft05_37x11'), ('ignore_x_len', 'soft05_37x11'),
    ('no_diag', 'onehot_advance'), ('first_col', 'soft05_40x129')])
def test_planted_dp_defects_show(cases, restated, defect, name):
    c = cases[name]
    bad = ac.durations_dp(c['att'], c['mel_len'], c['x_len'], defect)[0]
    assert not np.array_equal(bad, restated[name][0]), (defect, name)


@pytest.mark.parametrize('defect,name', [
    ('unrepaired', 'count_jump11'), ('last_argmax', 'count_tie'), ('read_pad_rows', 'count_beyond'),
    ('ignore_x_len', 'count_short')])
def test_planted_count_defects_show(gold, cases, defect, name):
    c = cases[name]
    bad = ac.durations_count(c['att'], c['mel_len'], c['x_len'], defect)
    assert not np.array_equal(bad, gold[f'cnt/{name}']), (defect, name)


def test_count_cases_mean_what_they_say(gold, cases):
    j11, j10 = gold['cnt/count_jump11'], gold['cnt/count_jump10']
    assert j11[3] == 11 and not j11[14:19].any()  # the repair cascades: every later row joins token 3
    assert j10[13] == 2 and j10[3] == 1           # a jump of exactly 10 is kept
    short = cases['count_short']
    assert np.flatnonzero(gold['cnt/count_short']).max() < short['x_len'] - 1
    assert gold['cnt/count_tie'][4] == 2 and gold['cnt/count_tie'][7] == 1


@pytest.mark.parametrize('defect', ['sharp_by_mel_len', 'loc_over_rows'])
def test_planted_score_defects_show(gold, defect):
    att = ac.score_case()
    loc, sharp = ac.scores(att, ac.SCORE_MEL_LENS[1], 1, defect)
    got = sharp if defect.startswith('sharp') else loc
    ref = gold['sharp64/1'] if defect.startswith('sharp') else gold['loc64/1']
    assert np.abs(got - ref).max() > 1e-3


# ---- public surface -----------------------------------------------------------------------

def test_header_and_binding_agree():
    text = re.sub(r'/\*.*?\*/', '', HEADER.read_text(), flags=re.S)
    ctype = {'int32_t': _lib.c_int, 'int64_t': _lib.c_int64, 'int': _lib.c_int}
    for name in ALIGN_FUNCS:
        ret, params = re.search(r'(\w+)\s+%s\(([^)]*)\)' % name, text).groups()
        want = [_lib.P if ('*' in p or 'ftmi_stream_t' in p) else ctype[p.split()[-2]]
                for p in params.split(',')]
        res, args = _lib.SIGNATURES[name]
        assert args == want, name
        assert res == ctype[ret], name
    assert _lib.ABI_VERSION == 22
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in ALIGN_FUNCS)


def test_entry_point_argument_errors():
    lib = _lib.load()
    f, g = ctypes.c_void_p(256), ctypes.c_void_p(258)
    assert lib.ftmi_align_workspace_bytes(2, 40, 512) >= 2 * (40 + 511) * 512
    assert lib.ftmi_align_workspace_bytes(1, 40, 513) == 0
    assert lib.ftmi_align_workspace_bytes(0, 40, 12) == 0 and lib.ftmi_align_workspace_bytes(1, 0, 12) == 0
    assert lib.ftmi_align_workspace_bytes(3, 7, 5) % 16 == 0
    assert lib.ftmi_align_dijkstra(None, 12, 480, 1, 40, 12, f, None, f, None, f, None) == 1001
    assert lib.ftmi_align_dijkstra(f, 12, 480, 1, 40, 12, f, None, f, None, None, None) == 1001
    assert lib.ftmi_align_dijkstra(f, 12, 480, 0, 40, 12, f, None, f, None, f, None) == 1001
    assert lib.ftmi_align_dijkstra(f, 513, 513 * 40, 1, 40, 513, f, None, f, None, f, None) == 1003
    assert lib.ftmi_align_dijkstra(f, 11, 480, 1, 40, 12, f, None, f, None, f, None) == 1002
    assert lib.ftmi_align_dijkstra(g, 12, 480, 1, 40, 12, f, None, f, None, f, None) == 1004
    assert lib.ftmi_align_dijkstra(f, 12, 480, 1, 40, 12, f, None, f, None, ctypes.c_void_p(264), None) == 1004
    assert lib.ftmi_align_count(f, 12, 480, 1, 40, 12, None, None, f, None) == 1001
    assert lib.ftmi_align_count(f, 513, 513 * 40, 1, 40, 513, f, None, f, None) == 1003
    assert lib.ftmi_align_count(f, 12, 480, 1, 40, 12, f, g, f, None) == 1004
    assert lib.ftmi_attention_score(f, 12, 480, 1, 40, 12, f, 0, f, f, None) == 1001
    assert lib.ftmi_attention_score(f, 12, 480, 1, 40, 12, f, 1, None, None, None) == 1001
    assert lib.ftmi_attention_score(f, 513, 513 * 40, 1, 40, 513, f, 1, f, f, None) == 1003


def test_wrapper_argument_errors():
    att = torch.zeros(2, 6, 4)
    with pytest.raises(RuntimeError, match='HIP device only'):
        align.extract_durations(att, [6, 6])
    with pytest.raises(RuntimeError, match='HIP device only'):
        align.attention_score(att, torch.tensor([6, 6]))
    with pytest.raises(ValueError, match='method'):
        align.extract_durations(att, [6, 6], method='viterbi')
    with pytest.raises(ValueError, match='return_cost'):
        align.extract_durations(att, [6, 6], method='count', return_cost=True)
    with pytest.raises(ValueError, match='att must be'):
        align.extract_durations(torch.zeros(4), [1])
    dev = torch.device('cpu')
    for bad, hi in (([0, 3], 6), ([3, 7], 6), ([3], 6), ([2.0, 3.0], 6)):
        with pytest.raises(ValueError):
            align._lengths(bad, 2, hi, 'mel_len', dev)
    got = align._lengths(torch.tensor([6, 1]), 2, 6, 'mel_len', dev)
    assert got.dtype == torch.int32 and got.tolist() == [6, 1]
    assert align._lengths(5, 1, 6, 'mel_len', dev).tolist() == [5]
    with pytest.raises(RuntimeError, match='HIP device only'):
        ops.align_dijkstra(att, torch.tensor([6, 6], dtype=torch.int32))


def test_create_align_features_layout(tmp_path, monkeypatch, cases):
    """The .npy / .pkl layout with the model and the two device calls stubbed by the
    restatement: dur[:x_len] per item as int32, the score dict keyed by item id."""
    names = ('soft05_37x11', 'deg_3x9', 'nonmono_30x12')
    cores = [cases[n]['att'][:cases[n]['mel_len'], :cases[n]['x_len']] for n in names]

    def batch(ks):
        rows, T = max(cores[k].shape[0] for k in ks) + 1, max(cores[k].shape[1] for k in ks)
        att = torch.from_numpy(np.stack([ac.embed(cores[k], rows, T, seed=k) for k in ks]))
        return {'x': torch.zeros(len(ks), T, dtype=torch.long), 'mel': torch.zeros(len(ks), 80, rows),
                'item_id': [names[k] for k in ks], 'att': att,
                'mel_len': torch.tensor([cores[k].shape[0] for k in ks]),
                'x_len': torch.tensor([cores[k].shape[1] for k in ks])}

    class Model(torch.nn.Module):
        r = 1

        def __init__(self):
            super().__init__()
            self.p = torch.nn.Parameter(torch.zeros(1))
            self.batches = {}

        def forward(self, x, m):
            return None, None, self.batches[tuple(x.shape)]

    def fake_scores(att, mel_lens, r=1):
        loc, sharp = ac.scores(att.numpy(), mel_lens.tolist(), r)
        return torch.from_numpy(loc).float(), torch.from_numpy(sharp).float()

    def fake_durations(att, mel_len, x_len=None, method='dijkstra', return_cost=False):
        assert method == 'dijkstra'
        return torch.from_numpy(np.stack([ac.durations_dp(a, int(m), int(c))[0] for a, m, c in
                                          zip(att.numpy(), mel_len, x_len)]))

    monkeypatch.setattr(align, 'attention_score', fake_scores)
    monkeypatch.setattr(align, 'extract_durations', fake_durations)
    model = Model()
    train, val = [batch([0, 1])], [batch([2])]
    for b in train + val:
        model.batches[tuple(b['x'].shape)] = b.pop('att')
    (tmp_path / 'alg').mkdir()
    n = align.create_align_features(model, train, val, tmp_path / 'alg', tmp_path)
    assert n == 3 and sorted(p.name for p in (tmp_path / 'alg').iterdir()) == sorted(f'{k}.npy' for k in names)
    with open(tmp_path / 'att_score_dict.pkl', 'rb') as f:
        d = pickle.load(f)
    assert sorted(d) == sorted(names)
    for k, core in zip(names, cores):
        dur = np.load(tmp_path / 'alg' / f'{k}.npy', allow_pickle=False)
        assert dur.dtype == np.int32 and dur.shape == (core.shape[1],) and dur.sum() == core.shape[0]
        assert np.array_equal(dur, ac.durations_dp(core, *core.shape)[0])
        assert isinstance(d[k], tuple) and len(d[k]) == 2 and all(type(v) is float for v in d[k])
    model.r = 2
    with pytest.raises(AssertionError, match='Reduction factor'):
        align.create_align_features(model, train, val, tmp_path / 'alg', tmp_path)
