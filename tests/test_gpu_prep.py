"""The silence trim and audio preparation on the device (csrc/prep.hip, DSP.trim_silence /
prepare_batch / prepare_wav, python -m forwardtacotron_amd.preprocess) against the numpy
restatement of tests/prep_cases.py.  tests/test_prep_cases.py (CPU) asserts what the equalities
below rely on: no frame of a case within 0.01 dB of the threshold, no mu-law value within 1e-9
of a rounding boundary.

Bounds: power within 2^-23 relative of the float64 mean (one float32 rounding is 2^-24; the
fp64 accumulation of at most 2048 non-negative terms adds less than 2^-41); everything after
that is an equality."""
import copy
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import prep_cases as pc
from forwardtacotron_amd import dsp as D
from forwardtacotron_amd.dsp import DSP

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
CONFIG = ROOT / 'tests' / 'golden' / 'dsp_config.json'
CASES = pc.cases()


@pytest.fixture(scope='module')
def base_dsp():
    return DSP.from_config(json.loads(CONFIG.read_text()))


def _dsp_for(base, case):
    """The module's DSP (its device plan shared) under a preparation case's switches."""
    d = copy.copy(base)
    d.should_peak_norm = case.peak_norm
    d.should_trim_start_end_silence = case.trim
    d.trim_silence_top_db = case.top_db
    kind, bits = case.mode
    d.voc_mode = 'MOL' if kind == 'mol' else 'RAW'
    d.mu_law = kind == 'mu'
    d.bits = 9 if kind == 'mol' else bits  # MOL ignores bits: 16 whatever the config says
    return d


def _device_rows(case):
    y, lengths = pc.rows(case)
    rows = torch.from_numpy(y).cuda()
    # a row stride greater than L: the rows are a view of a wider buffer
    wide = torch.full((rows.shape[0], rows.shape[1] + 13), pc.PLANT, device='cuda')
    wide[:, :rows.shape[1]] = rows
    return wide[:, :rows.shape[1]], torch.from_numpy(lengths).cuda()


@pytest.mark.parametrize('case', CASES, ids=lambda c: c.name)
def test_frame_power(case):
    y, lengths = _device_rows(case)
    assert y.stride(0) > y.shape[1]
    p1 = D.frame_power(y, lengths, case.frame_length, case.hop)
    p2 = D.frame_power(y, lengths, case.frame_length, case.hop)
    torch.cuda.synchronize()
    assert p1.shape == (len(case.items), 1 + y.shape[1] // case.hop) and p1.dtype == torch.float32
    assert torch.equal(p1.view(torch.int32), p2.view(torch.int32))  # two launches, the same bits
    got = p1.cpu().numpy()
    for b, v in enumerate(case.items):
        want = pc.frame_power_np(v, case.frame_length, case.hop, np.float64)
        Fb = len(want)
        err = np.abs(got[b, :Fb].astype(np.float64) - want)
        rel = (err / np.maximum(want, np.finfo(np.float64).tiny)).max()
        print(f'{case.name}[{b}]: max relative error {rel:.3e}')
        assert (err <= 2.0 ** -23 * want).all()
        assert (got[b, Fb:] == 0).all()


@pytest.mark.parametrize('case', CASES, ids=lambda c: c.name)
def test_trim_bounds(case):
    y, lengths = _device_rows(case)
    got = D.trim_bounds(y, lengths, case.top_db, case.frame_length, case.hop)
    assert got.dtype == torch.int32 and got.shape == (len(case.items), 2)
    got = [tuple(r) for r in got.cpu().tolist()]
    assert got == list(pc.expected_bounds(case.name, 'float64'))
    assert got == list(pc.expected_bounds(case.name, 'float32'))


def test_trim_bounds_without_lengths():
    case = next(c for c in CASES if c.name == 'ref-12345')
    y = torch.from_numpy(case.items[0]).cuda()[None]
    got = tuple(D.trim_bounds(y, None, case.top_db)[0].tolist())
    assert got == pc.expected_bounds(case.name, 'float64')[0]


def test_trim_silence_numpy_and_tensor(base_dsp):
    case = next(c for c in CASES if c.name == 'ref-30000')
    v = case.items[0]
    assert base_dsp.trim_silence_top_db == case.top_db
    s, e = pc.expected_bounds(case.name, 'float64')[0]
    assert 0 < s < e < len(v)
    out = base_dsp.trim_silence(v)
    assert isinstance(out, np.ndarray) and out.dtype == v.dtype and np.array_equal(out, v[s:e])
    out64 = base_dsp.trim_silence(v.astype(np.float64))
    assert out64.dtype == np.float64 and np.array_equal(out64, v[s:e].astype(np.float64))
    t = torch.from_numpy(v).cuda()
    out_t = base_dsp.trim_silence(t)
    assert isinstance(out_t, torch.Tensor) and out_t.is_cuda and torch.equal(out_t, t[s:e])


@pytest.mark.parametrize('case', pc.prep_cases(), ids=lambda c: c.name)
def test_prepare_batch(base_dsp, case):
    d = _dsp_for(base_dsp, case)
    y, lengths = _device_rows(case)
    p = d.prepare_batch(y, lengths)
    torch.cuda.synchronize()
    B, L = y.shape
    assert p._fields == ('wav', 'lengths', 'mel', 'frames', 'quant', 'bounds', 'peak')
    assert p.wav.shape == (B, L) and p.quant.shape == (B, L) and p.quant.dtype == torch.int64
    assert p.mel.shape == (B, d.n_mels, 1 + L // d.hop_length)
    wav, quant, mel = p.wav.cpu().numpy(), p.quant.cpu().numpy(), p.mel.cpu().numpy()
    kind, bits = case.mode
    for b, v in enumerate(case.items):
        s, e, peak, w, _ = pc.prepare_np(v, case.top_db, case.peak_norm, case.mode, case.trim)
        n = e - s
        assert tuple(p.bounds[b].tolist()) == (s, e)
        assert int(p.lengths[b]) == n and int(p.frames[b]) == 1 + n // d.hop_length
        assert np.float32(p.peak[b].item()) == peak
        # bit-equal to numpy's float32 y[s:e] / peak (or y[s:e] when unscaled), zero beyond
        assert np.array_equal(wav[b, :n].view(np.int32), w.view(np.int32))
        assert (wav[b, n:] == 0).all() and (quant[b, n:] == 0).all()
        if not v.any():  # the all-zero item: unscaled, no NaN from a 0 / 0
            assert peak == 0 and (wav[b] == 0).all()
        # labels against the project's own static methods
        if kind == 'mu':
            want = DSP.encode_mu_law(w.astype(np.float64), 2 ** bits).astype(np.int64)
        else:
            want = DSP.float_2_label(w, bits).astype(np.int64)
        assert np.array_equal(quant[b, :n], want)
        # the mel of the item's prepared samples alone, bit for bit; zeros past its frames
        alone = d.wav_to_mel(w)
        fr = alone.shape[1]
        assert fr == 1 + n // d.hop_length
        assert np.array_equal(mel[b, :, :fr].view(np.int32), alone.view(np.int32))
        assert (mel[b, :, fr:] == 0).all()


def test_prepare_wav_is_the_single_file_form(base_dsp):
    case = next(c for c in pc.prep_cases() if c.name == 'mu9-norm-off')
    d = _dsp_for(base_dsp, case)
    v = case.items[0]
    s, e, peak, w, q = pc.prepare_np(v, case.top_db, case.peak_norm, case.mode)
    mel, quant = d.prepare_wav(v)
    assert mel.dtype == np.float32 and mel.shape == (d.n_mels, 1 + (e - s) // d.hop_length)
    assert quant.dtype == np.int64 and np.array_equal(quant, q)
    assert np.array_equal(mel, d.wav_to_mel(w))


def test_trim_long_silences_is_refused(base_dsp):
    d = copy.copy(base_dsp)
    d.should_trim_long_silences = True
    y = torch.zeros(1, 4096, device='cuda')
    with pytest.raises(NotImplementedError, match='webrtcvad'):
        d.prepare_batch(y)
    with pytest.raises(NotImplementedError, match='webrtcvad'):
        d.prepare_wav(np.zeros(4096, np.float32))


def test_cli_writes_the_reference_files(base_dsp, tmp_path):
    wavdir, out = tmp_path / 'wavs', tmp_path / 'out'
    wavdir.mkdir()
    sigs = {'a_long': pc.item(12345, 41, 4000, 9000), 'b_short': pc.item(6000, 42, 2000, 4500),
            'c_mid': pc.item(9001, 43, 3000, 7000, amp=0.8)}
    for k, v in sigs.items():
        base_dsp.save_wav(v, wavdir / f'{k}.wav')
    r = subprocess.run([sys.executable, '-m', 'forwardtacotron_amd.preprocess', '--path',
                        str(wavdir), '--out', str(out), '--config', str(CONFIG), '--batch', '2'],
                       cwd=str(ROOT), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    listed = dict(json.loads((out / 'dataset.json').read_text()))
    assert sorted(listed) == sorted(sigs)
    for k in sigs:
        mel, quant = base_dsp.prepare_wav(base_dsp.load_wav(wavdir / f'{k}.wav'))
        got_mel = np.load(out / 'mel' / f'{k}.npy', allow_pickle=False)
        got_q = np.load(out / 'quant' / f'{k}.npy', allow_pickle=False)
        assert got_mel.dtype == np.float32 and got_mel.shape == mel.shape
        assert got_q.dtype == np.int64 and got_q.shape == quant.shape
        assert np.array_equal(got_mel, mel) and np.array_equal(got_q, quant)
        assert listed[k] == mel.shape[1] and 0 < len(quant) < len(sigs[k])
