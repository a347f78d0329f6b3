"""Phoneme-level pitch and energy on the HIP path (forwardtacotron_amd/align.py,
csrc/align.hip) against the float64 restatement (tests/feature_cases.py) and the reference's
recorded files (tests/golden/goldens_features.npz).

Bounds.  A phoneme mean is an fp64 sum of at most a few thousand terms divided once and
rounded to fp32 once: within 2^-23 relative of the restatement (half of that is the rounding,
the rest is slack for the order of the fp64 sums and the last bit of exp).  The reference's own
fp32 arithmetic is off by the error the goldens script recorded per case, so its files are
matched within that plus 2^-23.  Mean and std are fp64 over fp32-rounded values: 2^-23
relative.  A normalised pitch t = (v - mean) / std carries five half-ulp roundings (v, mean,
std, the subtraction, the division), each at most 2^-24 of |t| + mean / std in t's units, and
the bound allows eight: 4 * 2^-24 * (|t| + mean / std).  Given the same fp32 mean and std the
normalisation itself is numpy's, bit for bit."""
import pickle

import numpy as np
import pytest
import torch

import feature_cases as fc
from conftest import load_golden

pytestmark = pytest.mark.gpu

CASES = fc.feature_cases()
EPS = 2.0 ** -23


@pytest.fixture(scope='module')
def gold():
    g = load_golden('goldens_features')
    for n, c in CASES.items():
        assert fc.sha(c) == str(g[f'sha/{n}']), n
    return g


@pytest.fixture(scope='module')
def restated():
    """name -> (pitch_char, energy_char) float64, and the data set's normalisation."""
    r = {n: fc.run(c) for n, c in CASES.items()}
    normed, mean, std = fc.normalize([r[n][0] for n in CASES])
    return r, dict(zip(CASES, normed)), mean, std


def device_case(c):
    """The case on the device: mel as a view with the case's bin stride, lengths as ints."""
    buf = torch.from_numpy(fc.strided(c)).cuda()
    return (buf[:, :c['mel'].shape[1]], c['mel_len'], torch.from_numpy(c['dur']).cuda(), c['x_len'],
            torch.from_numpy(c['pitch']).cuda(), c['pitch_len'], fc.PITCH_MAX)


@pytest.fixture(scope='module')
def computed():
    """name -> (pitch_char, energy_char) fp32 numpy, each case as a single-item call."""
    from forwardtacotron_amd import align
    out = {}
    for n, c in CASES.items():
        p, e = align.phoneme_pitch_energy(*device_case(c))
        assert p.shape == e.shape == (len(c['dur']),) and p.dtype == e.dtype == torch.float32 and p.is_cuda
        out[n] = (p.cpu().numpy(), e.cpu().numpy())
    return out


def rel(got, want):
    live = want != 0
    return float(np.max(np.abs(got[live] - want[live]) / np.abs(want[live]), initial=0.0))


@pytest.mark.parametrize('name', list(CASES))
def test_values(gold, restated, computed, name):
    c = CASES[name]
    (p, e), (p64, e64) = computed[name], restated[0][name]
    ge = gold[f'energy/{name}'].astype(np.float64)
    assert np.isfinite(p).all() and np.isfinite(e).all()  # no NaN padding frame was read
    assert np.array_equal(e == 0, ge == 0) and np.array_equal(p == 0, gold[f'pitch/{name}'] == 0)
    assert np.array_equal(e == 0, e64 == 0) and np.array_equal(p == 0, p64 == 0)
    assert not e[min(c['x_len'], c['mel_len']):].any()
    err_ref = float(gold[f'err_e/{name}'])
    print(name, 'energy rel err', rel(e, e64) / EPS, 'pitch rel err', rel(p, p64) / EPS,
          'x 2^-23; vs reference', rel(e, ge) / EPS, 'reference own', err_ref / EPS)
    assert rel(e, e64) <= EPS and rel(p, p64) <= EPS
    assert (np.abs(e - ge) <= (err_ref + EPS) * e64).all()


def all_pitches(computed):
    return np.concatenate([computed[n][0] for n in CASES])


def test_moments(restated, computed):
    from forwardtacotron_amd import ops
    v = all_pitches(computed)
    dev = torch.from_numpy(v).cuda()
    cnt, mean, std = ops.nonzero_moments(dev).tolist()
    again = ops.nonzero_moments(dev)
    c64, m64, s64 = fc.moments([restated[0][n][0] for n in CASES])
    c32, m32, s32 = fc.moments([v])  # the same fp32 values in float64: the kernel alone
    print('count', cnt, c64, 'mean', mean, m64, abs(mean - m64) / m64 / EPS, 'std', std, s64,
          abs(std - s64) / s64 / EPS, 'x 2^-23; kernel alone', abs(mean - m32) / m32, abs(std - s32) / s32)
    assert cnt == c64 == c32 == np.count_nonzero(v)
    assert abs(mean - m64) <= EPS * m64 and abs(std - s64) <= EPS * s64
    assert abs(mean - m32) <= 2.0 ** -45 * m32 and abs(std - s32) <= 2.0 ** -45 * s32
    assert again.tolist() == [cnt, mean, std]
    # sizes around the 1024 x 8 stride of the reduction, zeros included
    g = np.random.Generator(np.random.PCG64(3))
    for n in (1, 1023, 1025, 8191, 8193, 20000):
        w = g.uniform(60.0, 400.0, n).astype(np.float32)
        w[g.random(n) < 0.3] = 0.0
        w[0] = 123.0
        c, m, s = ops.nonzero_moments(torch.from_numpy(w).cuda()).tolist()
        cw, mw, sw = fc.moments([w])
        assert c == cw and abs(m - mw) <= 2.0 ** -45 * mw and abs(s - sw) <= 2.0 ** -45 * max(sw, 1.0), n


def test_normalize_is_numpys_bit_for_bit(gold, computed):
    from forwardtacotron_amd import ops
    v = all_pitches(computed)
    for mean, std in (tuple(gold['mean_std']), (np.float32(201.37), np.float32(0.3))):
        want = v.copy()
        nz = want != 0
        want[nz] = (want[nz] - np.float32(mean)) / np.float32(std)
        dev = torch.from_numpy(v.copy()).cuda()
        assert ops.normalize_nonzero(dev, float(mean), float(std)) is dev
        assert np.array_equal(dev.cpu().numpy().view(np.uint32), want.view(np.uint32))


def test_normalize_values_end_to_end(gold, restated, computed):
    from forwardtacotron_amd import align
    _, normed, m64, s64 = restated
    devs = [torch.from_numpy(computed[n][0].copy()).cuda() for n in CASES]
    mean, std = align.normalize_values(devs)
    assert type(mean) is float and type(std) is float
    assert mean == float(np.float32(mean)) and std == float(np.float32(std))
    assert abs(mean - m64) <= EPS * m64 and abs(std - s64) <= EPS * s64
    gm, gs = gold['mean_std'].astype(np.float64)
    gm64, gs64 = gold['mean_std64']
    assert abs(mean - gm) <= EPS * m64 + abs(gm - gm64) and abs(std - gs) <= EPS * s64 + abs(gs - gs64)
    for n, d in zip(CASES, devs):
        got, t = d.cpu().numpy().astype(np.float64), normed[n]
        bound = 4 * 2.0 ** -24 * (np.abs(t) + m64 / s64)
        print(n, 'normalised pitch err / bound', float(np.max(np.abs(got - t) / bound)))
        assert np.array_equal(got == 0, t == 0)
        assert (np.abs(got - t) <= bound).all()
        assert (np.abs(got - gold[f'pitch/{n}']) <= bound + float(gold[f'err_p/{n}'])).all()
    one = torch.from_numpy(all_pitches(computed)).cuda()  # a single tensor: the same moments
    assert align.normalize_values(one) == (mean, std)
    with pytest.raises(ValueError, match='no non-zero'):
        align.normalize_values(torch.zeros(5, device='cuda'))


def test_batch_rows_equal_single_items(gold, computed):
    """A mixed batch of five through strided views, twice: every row is bit for bit the
    single-item result, NaN frames, decoy durations and decoy pitches notwithstanding; and
    energy alone (no pitch) gives the same energies."""
    from forwardtacotron_amd import align
    b = fc.batch_case(CASES)
    assert fc.sha(b) == str(gold['sha/batch'])
    B, n_mels, rows = b['mel'].shape
    mel = torch.full((B, n_mels, rows + 5), float('nan'), device='cuda')
    mel[:, :, :rows] = torch.from_numpy(b['mel']).cuda()
    dur = torch.full((B, b['dur'].shape[1] + 3), 7, dtype=torch.int32, device='cuda')
    dur[:, :b['dur'].shape[1]] = torch.from_numpy(b['dur']).cuda()
    pit = torch.full((B, b['pitch'].shape[1] + 2), 50.0, device='cuda')
    pit[:, :b['pitch'].shape[1]] = torch.from_numpy(b['pitch']).cuda()
    args = (mel[:, :, :rows], torch.tensor(b['mel_len']), dur[:, :b['dur'].shape[1]], b['x_len'],
            pit[:, :b['pitch'].shape[1]], torch.tensor(b['pitch_len']).cuda(), fc.PITCH_MAX)
    assert not args[0].is_contiguous() and not args[2].is_contiguous() and not args[4].is_contiguous()
    p, e = align.phoneme_pitch_energy(*args)
    p2, e2 = align.phoneme_pitch_energy(*args)
    none, e3 = align.phoneme_pitch_energy(*args[:4])
    assert p.shape == e.shape == (B, b['dur'].shape[1]) and none is None
    assert torch.equal(p, p2) and torch.equal(e, e2) and torch.equal(e, e3)
    assert bool(torch.isfinite(p).all()) and bool(torch.isfinite(e).all())
    for k, n in enumerate(fc.BATCH_ITEMS):
        T = len(CASES[n]['dur'])
        sp, se = computed[n]
        assert np.array_equal(p[k, :T].cpu().numpy().view(np.uint32), sp.view(np.uint32)), n
        assert np.array_equal(e[k, :T].cpu().numpy().view(np.uint32), se.view(np.uint32)), n
        assert not p[k, T:].any() and not e[k, T:].any()
    again = align.phoneme_pitch_energy(*device_case(CASES['t512']))
    assert np.array_equal(again[0].cpu().numpy(), computed['t512'][0])
    assert np.array_equal(again[1].cpu().numpy(), computed['t512'][1])


def test_duration_sum_mismatch_and_limits():
    from forwardtacotron_amd import _lib, align, ops
    mel, L, dur, C, pitch, PL, fmax = device_case(CASES['x_len_decoys'])
    bad = dur.clone()
    bad[1] += 1
    with pytest.raises(ValueError, match=r'sum of durations.*item\(s\) \[0\]'):
        align.phoneme_pitch_energy(mel, L, bad, C, pitch, PL, fmax)
    with pytest.raises(ValueError, match='sum of durations'):  # the decoys count without x_len
        align.phoneme_pitch_energy(mel, L, dur, None, pitch, PL, fmax)
    neg = dur.clone()
    neg[0] -= 3  # a negative entry still counts in the sum the host compares
    with pytest.raises(ValueError, match='sum of durations'):
        align.phoneme_pitch_energy(mel, L, neg, C, pitch, PL, fmax)
    both = torch.stack([dur, bad])
    with pytest.raises(ValueError, match=r'item\(s\) \[1\]'):
        align.phoneme_pitch_energy(torch.stack([mel, mel]), [L, L], both, [C, C])
    wide = torch.ones(1, 513, dtype=torch.int32, device='cuda')
    with pytest.raises(ValueError, match='tokens'):
        align.phoneme_pitch_energy(mel[None], [L], wide)
    with pytest.raises(_lib.FtmiError, match='status 1003'):
        ops.phoneme_features(mel[None].contiguous(), torch.tensor([L], dtype=torch.int32).cuda(), wide)
    with pytest.raises(ValueError, match='mel_len'):
        align.phoneme_pitch_energy(mel, mel.size(1) + 1, dur, C)
    with pytest.raises(ValueError, match='pitch_len'):
        align.phoneme_pitch_energy(mel, L, dur, C, pitch, pitch.numel() + 1)


# ---- the data-set functions ------------------------------------------------------------------

ORDER = sorted(CASES, key=lambda n: -CASES[n]['mel'].shape[0])  # 12 items of 80 bins, then 13 bins


def write_dataset(root, cases, names):
    for k in ('alg', 'mel', 'raw_pitch', 'phon_pitch', 'phon_energy'):
        (root / k).mkdir()
    for n in names:
        c = cases[n]
        np.save(root / 'alg' / f'{n}.npy', c['dur'][:c['x_len']], allow_pickle=False)
        np.save(root / 'mel' / f'{n}.npy', c['mel'][:, :c['mel_len']], allow_pickle=False)
        np.save(root / 'raw_pitch' / f'{n}.npy', c['pitch'][:c['pitch_len']], allow_pickle=False)
    return [(n, cases[n]['mel_len']) for n in names]


def test_extract_pitch_energy_files(gold, restated, tmp_path):
    """The cases as a data set on disk, four items per batch: the files and (mean, std) the
    reference wrote from the same three folders."""
    from forwardtacotron_amd import align
    assert [CASES[n]['mel'].shape[0] for n in ORDER] == [80] * 12 + [13] * 7  # no batch mixes bins
    data = write_dataset(tmp_path, CASES, ORDER)
    mean, std = align.extract_pitch_energy(data, tmp_path / 'alg', tmp_path / 'mel', tmp_path / 'raw_pitch',
                                           tmp_path / 'phon_pitch', tmp_path / 'phon_energy',
                                           fc.PITCH_MAX, batch_size=4)
    r, normed, m64, s64 = restated
    gm, gs = gold['mean_std'].astype(np.float64)
    gm64, gs64 = gold['mean_std64']
    assert abs(mean - gm) <= EPS * m64 + abs(gm - gm64) and abs(std - gs) <= EPS * s64 + abs(gs - gs64)
    assert sorted(p.name for p in (tmp_path / 'phon_pitch').iterdir()) == sorted(f'{n}.npy' for n in CASES)
    for n, c in CASES.items():
        C = c['x_len']
        p = np.load(tmp_path / 'phon_pitch' / f'{n}.npy', allow_pickle=False)
        e = np.load(tmp_path / 'phon_energy' / f'{n}.npy', allow_pickle=False)
        assert p.dtype == e.dtype == np.float32 and p.shape == e.shape == (C,), n
        ge, gp, e64, t = gold[f'energy/{n}'][:C], gold[f'pitch/{n}'][:C], r[n][1][:C], normed[n][:C]
        assert np.array_equal(e == 0, ge == 0) and np.array_equal(p == 0, gp == 0), n
        assert (np.abs(e - ge.astype(np.float64)) <= (float(gold[f'err_e/{n}']) + EPS) * e64).all(), n
        bound = 4 * 2.0 ** -24 * (np.abs(t) + m64 / s64) + float(gold[f'err_p/{n}'])
        assert (np.abs(p - gp.astype(np.float64)) <= bound).all(), n
    np.save(tmp_path / 'alg' / 't1.npy', np.array([2], np.int32), allow_pickle=False)
    with pytest.raises(ValueError, match='t1.*sum of durations'):
        align.extract_pitch_energy(data[:4], tmp_path / 'alg', tmp_path / 'mel', tmp_path / 'raw_pitch',
                                   tmp_path / 'phon_pitch', tmp_path / 'phon_energy', fc.PITCH_MAX)


def test_create_align_features_with_pitch_and_energy(tmp_path):
    """The synthetic Tacotron (r = 1) over three items.  Without the new keywords no pitch or
    energy file appears; with them the folders hold what a separate extract_pitch_energy call
    over the written durations gives, byte for byte."""
    import json

    from conftest import GOLDEN
    from forwardtacotron_amd import align
    from forwardtacotron_amd.gta import collate_tts
    from forwardtacotron_amd.synthetic import default_config, synthetic_array, synthetic_tokens
    from forwardtacotron_amd.tacotron import Tacotron
    keys = json.loads((GOLDEN / 'tacotron_state_dict_keys.json').read_text())
    model = Tacotron.from_config(default_config())
    model.load_state_dict({k: torch.from_numpy(synthetic_array(k, shape, dt, 0, 'tacotron'))
                           for k, shape, dt in keys})
    model = model.to('cuda').eval()
    rng = np.random.Generator(np.random.PCG64(6))
    for k in ('alg', 'alg2', 'mel', 'raw_pitch', 'phon_pitch', 'phon_energy', 'pitch2', 'energy2'):
        (tmp_path / k).mkdir()
    items = []
    for k, (x_len, mel_len) in enumerate(((12, 35), (12, 38), (8, 31))):
        x = synthetic_tokens(1, x_len, seed=300 + k)[0]
        mel = (rng.normal(0.0, 2.0, (80, mel_len)) - 4.0).astype(np.float32)
        pitch = rng.uniform(60.0, 560.0, mel_len).astype(np.float32)
        pitch[rng.random(mel_len) < 0.3] = 0.0
        np.save(tmp_path / 'mel' / f'utt{k}.npy', mel, allow_pickle=False)
        np.save(tmp_path / 'raw_pitch' / f'utt{k}.npy', pitch, allow_pickle=False)
        items.append({'x': x, 'mel': mel, 'item_id': f'utt{k}', 'x_len': x_len, 'mel_len': mel_len})
    train, val = [collate_tts(items[:1], 1)], [collate_tts(items[1:], 1)]
    data = [(it['item_id'], it['mel_len']) for it in items]
    assert align.create_align_features(model, train, val, tmp_path / 'alg2', tmp_path) == 3
    assert not list((tmp_path / 'phon_pitch').iterdir()) and not list((tmp_path / 'phon_energy').iterdir())
    assert align.create_align_features(
        model, train, val, tmp_path / 'alg', tmp_path, pitch_max_freq=400.0, dataset=data,
        mel_path=tmp_path / 'mel', raw_pitch_path=tmp_path / 'raw_pitch',
        phon_pitch_path=tmp_path / 'phon_pitch', phon_energy_path=tmp_path / 'phon_energy') == 3
    with open(tmp_path / 'att_score_dict.pkl', 'rb') as f:
        assert sorted(pickle.load(f)) == ['utt0', 'utt1', 'utt2']
    mean, std = align.extract_pitch_energy(data, tmp_path / 'alg', tmp_path / 'mel', tmp_path / 'raw_pitch',
                                           tmp_path / 'pitch2', tmp_path / 'energy2', 400.0)
    assert 60.0 < mean < 400.0 and 0.0 < std < 200.0
    for it in items:
        n, C = f'{it["item_id"]}.npy', it['x_len']
        assert np.array_equal(np.load(tmp_path / 'alg' / n), np.load(tmp_path / 'alg2' / n))
        for a, b in (('phon_pitch', 'pitch2'), ('phon_energy', 'energy2')):
            assert (tmp_path / a / n).read_bytes() == (tmp_path / b / n).read_bytes(), (a, n)
        e = np.load(tmp_path / 'phon_energy' / n)
        dur = np.load(tmp_path / 'alg' / n)
        assert e.dtype == np.float32 and e.shape == (C,) and np.array_equal(e != 0, dur != 0)
        want = fc.features(it['mel'], it['mel_len'], dur, C, np.zeros(1, np.float32), 0)[1]
        assert rel(e.astype(np.float64), want) <= EPS
