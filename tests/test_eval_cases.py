"""The yardstick of the validation-loss tests, without a GPU: the cases of tests/eval_cases.py are
the ones the goldens were made from, the float64 restatement equals the reference evaluated in
float64, and the case set meets the conditions the GPU test relies on.

Each case's own error |fp32 - float64| / |float64| of the reference is printed.  For the
mixture-of-logistics cases it reaches 60 x 2^-23 on a reduced loss and 2.8e-4 on a single sample:
the reference's fp32 cdf_delta, a difference of two sigmoids, is ill-conditioned near its 1e-5
threshold.  That is why the float64 evaluation, not the fp32 run, is what the device is held
to."""
import numpy as np
import pytest

import eval_cases as ec
from conftest import load_golden

L1, CE, MOL = ec.l1_cases(), ec.ce_cases(), ec.mol_cases()


@pytest.fixture(scope='module')
def gold():
    return load_golden('goldens_eval')


def close(got, want, tol=1e-12):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if np.isnan(want).any():
        return np.array_equal(np.isnan(got), np.isnan(want))
    return got.shape == want.shape and bool((np.abs(got - want) <= tol * np.abs(want)).all())


def test_shas(gold):
    for kind, cases in (('l1', L1), ('ce', CE), ('mol', MOL)):
        for n, c in cases.items():
            assert ec.sha(c) == str(gold[f'sha/{kind}/{n}']), (kind, n)
    assert ec.sha(ec.ce_rejected()) == str(gold['sha/ce/rejected'])
    stored = {k for k in gold if k.startswith('sha/')}
    assert len(stored) == len(L1) + len(CE) + len(MOL) + 1


@pytest.mark.parametrize('name', list(L1))
def test_l1_restatement(gold, name):
    print(name, 'reference own error', float(gold[f'err/l1/{name}']) / 2.0 ** -23, 'x 2^-23')
    assert close(ec.run_l1(L1[name]), gold[f'f64/l1/{name}'])


@pytest.mark.parametrize('name', list(CE))
def test_ce_restatement(gold, name):
    print(name, 'reference own error', float(gold[f'err/ce/{name}']) / 2.0 ** -23, 'x 2^-23')
    assert close(ec.cross_entropy(CE[name]['logits'], CE[name]['target']), gold[f'f64/ce/{name}'])


@pytest.mark.parametrize('name', list(MOL))
def test_mol_restatement(gold, name):
    print(name, 'reference own error', float(gold[f'err/mol/{name}']) / 2.0 ** -23, 'x 2^-23')
    assert close(ec.run_mol(MOL[name]), gold[f'f64/mol/{name}'])


def test_l1_case_set():
    """What the cases are there for."""
    big = L1['big_wide']
    assert big['x'].shape == (8, 80, 1500) and list(big['lens']) == [1500, 1, 0, 777, 1499, 64, 65, 2000]
    mag = np.abs(big['x'])
    assert mag.min() < 2e-3 and mag.max() > 500.0
    assert not L1['lens_all_zero']['lens'].any() and np.isnan(ec.run_l1(L1['lens_all_zero']))
    assert 0 in L1['lens_zero']['lens'] and L1['lens_over']['lens'].max() > L1['lens_over']['x'].shape[2]
    p = L1['pad_1e30']
    assert (p['x'][0, :, 33:] == np.float32(1e30)).all() and np.isfinite(ec.run_l1(p))
    nanp = ec.nan_padding(L1['mel_3x80x37'])
    assert np.isnan(nanp['x']).any() and ec.run_l1(nanp) == ec.run_l1(L1['mel_3x80x37'])
    assert 'lens' not in L1['plain']


def test_l1_fp32_accumulator_fails_the_big_case(gold):
    """A sequential fp32 sum of the big case is off by far more than the 2^-23 the device is
    allowed, so the bound does tell an fp32 accumulator from an fp64 one."""
    c = L1['big_wide']
    acc, count = np.float32(0.0), 0
    for b, n in enumerate(np.clip(c['lens'], 0, c['x'].shape[2])):
        d = np.abs(c['x'][b, :, :n] - c['target'][b, :, :n]).reshape(-1)
        acc = np.float32(acc + np.cumsum(d, dtype=np.float32)[-1]) if d.size else acc
        count += int(n)
    want = float(gold['f64/l1/big_wide'])
    got = float(acc) / (80 * count)
    assert abs(got - want) > 4 * 2.0 ** -23 * want


def test_ce_case_set():
    assert {c['logits'].shape[1] for c in CE.values()} >= {2, 30, 512, 513, 1024}
    assert {c['logits'].shape[0] for c in CE.values()} >= {1, 63, 65, 1400}
    s = CE['scaled300']['logits'].astype(np.float64)
    with np.errstate(over='ignore'):
        assert np.isinf(np.exp(s).sum(1)).all()  # an unstabilised sum overflows on every row
    assert np.ptp(s.max(1)) > 200.0
    assert (CE['argmax']['target'] == CE['argmax']['logits'].argmax(1)).all()
    assert (CE['argmin']['target'] == CE['argmin']['logits'].argmin(1)).all()
    bad = ec.ce_rejected()
    C = bad['logits'].shape[1]
    assert sorted(bad['target'][(bad['target'] < 0) | (bad['target'] >= C)]) == [-1, C]


def test_mol_case_set():
    assert {c['y_hat'].shape[2] // 3 for c in MOL.values()} == {1, 10, 11}
    assert any(c['num_classes'] == 256 for c in MOL.values())
    assert any('log_scale_min' in c for c in MOL.values()) and any(not c['reduce'] for c in MOL.values())
    e = MOL['edge_k10']
    assert e['y_hat'].shape == (3, 257, 30)
    y = e['y'].reshape(-1)
    assert (y == -1).sum() >= 5 and (y == 1).sum() >= 5
    for v in (ec.HI, ec.LO):
        for w in (v, np.nextafter(v, np.float32(2 * v)), np.nextafter(v, np.float32(0))):
            assert (y == w).any(), w
    assert (e['y_hat'][..., 20:] == -40.0).sum() == 2


def test_mol_branches_and_threshold_distance():
    """Over the case set every branch takes at least 1 % of the (sample, component) pairs, and no
    pair's float64 cdf_delta lies within a relative 1e-6 of the 1e-5 threshold, so the device
    and the float64 oracle cannot land on different sides of it."""
    counts, nearest = np.zeros(4), np.inf
    for n, c in MOL.items():
        _, branch, delta = ec.mol(c['y_hat'], c['y'], c['num_classes'], c.get('log_scale_min'))
        counts += np.bincount(branch.reshape(-1), minlength=4)
        tested = branch >= 2  # the pairs whose branch the threshold decides
        if tested.any():
            nearest = min(nearest, float(np.abs(delta[tested] / 1e-5 - 1.0).min()))
    share = counts / counts.sum()
    print('branch shares', share, 'closest cdf_delta to the threshold (relative)', nearest)
    assert (share >= 0.01).all(), share
    assert nearest > 1e-6
