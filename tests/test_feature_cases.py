"""The phoneme pitch / energy cases and their goldens without a GPU: the inputs still hash to
what the reference saw, the float64 restatement of include/ftmi.h's semantics
(tests/feature_cases.py) reproduces the reference's files within the reference's own recorded
fp32 error, each planted defect changes a named case, and the host-side surface of
forwardtacotron_amd.align (argument errors before any launch, create_align_features' new
keywords)."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import feature_cases as fc
from conftest import load_golden
from forwardtacotron_amd import _lib, align

HEADER = Path(__file__).resolve().parent.parent / 'include' / 'ftmi.h'
FEATURE_FUNCS = ('ftmi_phoneme_features', 'ftmi_nonzero_moments', 'ftmi_normalize_nonzero')


@pytest.fixture(scope='module')
def gold():
    return load_golden('goldens_features')


@pytest.fixture(scope='module')
def cases():
    return fc.feature_cases()


@pytest.fixture(scope='module')
def restated(cases):
    return {n: fc.run(c) for n, c in cases.items()}


def test_inputs_hash_to_the_goldens(gold, cases):
    for n, c in cases.items():
        assert fc.sha(c) == str(gold[f'sha/{n}']), n
    assert fc.sha(fc.batch_case(cases)) == str(gold['sha/batch'])


def test_case_list_covers_the_mechanisms(cases):
    c = cases
    assert len(c['t1']['dur']) == 1 and c['t1']['mel_len'] == 1
    z = c['zero_runs']['dur'][:c['zero_runs']['x_len']]
    assert z[0] == 0 and z[-1] == 0 and any(not z[k:k + 3].any() for k in range(len(z) - 2))
    b = c['tokens_beyond_frames']
    assert b['dur'].tolist() == [1, 0, 0, 1] and b['mel_len'] == 2 < b['x_len'] == 4
    d = c['x_len_decoys']
    assert d['x_len'] < len(d['dur']) and d['dur'][d['x_len']:].all()
    assert c['strided']['ld_bin'] > c['strided']['mel'].shape[1] == fc.strided(c['strided']).shape[1] - 13
    cum = np.cumsum(c['pitch_cut_inside']['dur'])
    assert c['pitch_cut_inside']['pitch_len'] not in cum and c['pitch_cut_before']['pitch_len'] in cum
    assert c['pitch_longer']['pitch_len'] > c['pitch_longer']['mel_len']
    assert {len(c[n]['dur']) for n in ('t64', 't65', 't512')} == {64, 65, 512}
    assert max(c['long_token']['dur']) == 1300
    assert {c[f'frames_{L}']['mel_len'] for L in (2047, 2048, 2049)} == {fc.CHUNK - 1, fc.CHUNK, fc.CHUNK + 1}
    assert {v['mel'].shape[0] for v in c.values()} == {80, 13}
    p = c['at_max']['pitch']
    assert p[0] == np.float32(fc.PITCH_MAX) and p[2] == np.nextafter(np.float32(fc.PITCH_MAX), np.float32(0))
    assert float(np.float32(fc.PITCH_MAX)) == fc.PITCH_MAX
    for v in c.values():  # padding that would be noticed
        L, C, PL = v['mel_len'], v['x_len'], v['pitch_len']
        assert v['mel'].dtype == np.float32 and np.isnan(v['mel'][:, L:]).all() and v['mel'].shape[1] > L
        assert np.isfinite(v['mel'][:, :L]).all() and v['mel'][:, :L].max() < 40
        assert v['dur'][:C].sum() == L and (v['pitch'][PL:] == 50.0).all() and len(v['pitch']) > PL
    bt = fc.batch_case(c)
    assert bt['mel'].shape[0] == 5 and len(set(bt['x_len'])) > 2 and bt['mel'].shape[1] == 80


def test_restatement_equals_reference(gold, cases, restated):
    """Energy within the reference's recorded fp32 error of the float64 value; the same zeros;
    the token rule of the reference's loop on [1, 0, 0, 1]."""
    for n, c in cases.items():
        p64, e64 = restated[n]
        e, p = gold[f'energy/{n}'].astype(np.float64), gold[f'pitch/{n}']
        assert float(gold[f'err_e/{n}']) <= 2.0 ** -20
        assert np.array_equal(e == 0, e64 == 0) and np.array_equal(p == 0, p64 == 0), n
        live = e64 != 0  # the quotient as the goldens script recorded it
        assert (np.abs(e[live] - e64[live]) / e64[live] <= float(gold[f'err_e/{n}'])).all(), n
        assert not e64[min(c['x_len'], c['mel_len']):].any() and np.isfinite(e64).all(), n
    p64, e64 = restated['tokens_beyond_frames']
    assert e64[0] > 0 and e64[3] == 0 and p64[0] == 120.0 and p64[3] == 0
    assert restated['unvoiced_token'][0][1] == 0 and restated['above_max_token'][0][1] == 0
    assert restated['at_max'][0][0] == 100.0  # the value equal to the maximum is dropped
    below = float(np.nextafter(np.float32(fc.PITCH_MAX), np.float32(0)))
    assert restated['at_max'][0][1] == (below + 100.0) / 2  # an ulp below is kept
    assert restated['pitch_cut_inside'][0][2] == 150.0 and restated['pitch_cut_inside'][0][3] == 0


def test_normalisation_restatement_equals_reference(gold, cases, restated):
    normed, mean, std = fc.normalize([restated[n][0] for n in cases])
    assert np.array_equal(gold['mean_std64'], [mean, std])
    m32, s32 = gold['mean_std'].astype(np.float64)
    assert abs(m32 - mean) <= 2.0 ** -20 * mean and abs(s32 - std) <= 2.0 ** -20 * std
    for n, t in zip(cases, normed):
        assert (np.abs(gold[f'pitch/{n}'] - t) <= float(gold[f'err_p/{n}'])).all(), n
        assert float(gold[f'err_p/{n}']) < 1e-5
    cnt, m2, s2 = fc.moments([np.array([0.0, 1.0, 3.0]), np.array([[0.0, 5.0]])])
    assert (cnt, m2) == (3, 3.0) and s2 == np.sqrt(8.0 / 3.0)


@pytest.mark.parametrize('defect,name', [
    ('all_tokens', 'tokens_beyond_frames'), ('le_max', 'at_max'), ('le_max', 'above_max_token'),
    ('pitch_by_frames', 'zero_runs'), ('ignore_pitch_len', 'pitch_cut_inside'),
    ('ignore_pitch_len', 'pitch_cut_before'), ('read_pad_frames', 'x_len_decoys')])
def test_planted_defects_show(cases, restated, defect, name):
    assert defect in fc.DEFECTS
    bp, be = fc.run(cases[name], defect)
    good = restated[name]
    assert not (np.array_equal(bp, good[0]) and np.array_equal(be, good[1], equal_nan=True)), (defect, name)


# ---- public surface -----------------------------------------------------------------------

def test_header_and_binding_agree():
    text = re.sub(r'/\*.*?\*/', '', HEADER.read_text(), flags=re.S)
    ctype = {'int32_t': _lib.c_int, 'int64_t': _lib.c_int64, 'int': _lib.c_int, 'float': _lib.c_float}
    for name in FEATURE_FUNCS:
        ret, params = re.search(r'(\w+)\s+%s\(([^)]*)\)' % name, text).groups()
        want = [_lib.P if ('*' in p or 'ftmi_stream_t' in p) else ctype[p.split()[-2]]
                for p in params.split(',')]
        res, args = _lib.SIGNATURES[name]
        assert args == want, name
        assert res == ctype[ret], name
    assert _lib.ABI_VERSION == 22


def test_wrapper_argument_errors():
    mel, dur = torch.zeros(2, 80, 6), torch.ones(2, 3, dtype=torch.int32)
    with pytest.raises(RuntimeError, match='HIP device only'):
        align.phoneme_pitch_energy(mel, [6, 6], dur)
    with pytest.raises(RuntimeError, match='HIP device only'):
        align.normalize_values(torch.ones(4))
    with pytest.raises(RuntimeError, match='HIP device only'):
        align.normalize_values([torch.ones(4)])
    with pytest.raises(ValueError, match='mel must be'):
        align.phoneme_pitch_energy(torch.zeros(6), [6], dur)
    with pytest.raises(ValueError, match='nothing to normalise'):
        align.normalize_values([])
    with pytest.raises(ValueError, match='non-empty data set'):
        align.extract_pitch_energy([], '.', '.', '.', '.', '.', 400.0)


def test_create_align_features_keywords_come_together():
    class Model:
        r = 1
    with pytest.raises(ValueError, match='pitch_max_freq needs'):
        align.create_align_features(Model(), [], [], '.', '.', pitch_max_freq=400.0)
    with pytest.raises(ValueError, match='need pitch_max_freq'):
        align.create_align_features(Model(), [], [], '.', '.', dataset=[('a', 1)])
    assert 'without the pitch' not in align.create_align_features.__doc__
