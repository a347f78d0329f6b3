"""The WaveRNN kernels (csrc/wavernn.hip) at every launch shape and off the default config,
against the fp64 oracle on the same fp32 weights and inputs (tests/wr_cases.py; the table's
preconditions and the defects it must catch are checked on the CPU by
tests/test_wavernn_cases.py).

  * teacher-forced logits per case: |logits - oracle fp64| <= max(1e-4, 10 drift), drift the
    oracle's own fp32 - fp64 gap on the case; status word clean;
  * the draw check of tests/test_gpu_wavernn.py at 256 and 16 classes and in MOL mode on hop 6;
  * ftmi_wr_stretch_conv against float64 conv2d(stretch2d(x)) with a derived bound per element:
    a chain of `taps` FMAs from 0 errs by at most (taps + 2) 2^-24 sum_k |w_k| |v_k| (taps
    roundings of partial sums each bounded by the sum of magnitudes, to first order; + 2 covers
    the higher-order terms);
  * ftmi_wr_unfold against the oracle's float64 tail (mu-law, crossfade, fade-out) to 1e-12;
  * the one-instance launches <16,1> and <32,1> (FTMI_WR_NI=1, read once per process: a child).

Every test prints its figures (`WR ...` lines) before it asserts.
"""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import wr_cases as C
from forwardtacotron_amd import _lib, ops
from oracle import wr_torch_cpu as wr

from conftest import load_golden

pytestmark = pytest.mark.gpu

DEV = 'cuda'
ROOT = Path(__file__).resolve().parent.parent


def _run(c):
    return C.gpu_logits(c, C.build_model(c.cfg, c.sd, DEV))


@pytest.mark.parametrize('name', list(C.CASES))
def test_teacher_forced_logits(name):
    c, l64, bound = C.case(name), C.oracle(name), C.bound(name)
    got, status = _run(c)
    err = float(np.abs(got - l64).max()) if np.isfinite(got).all() else float('inf')
    print(f'WR case {name} launches={C.launches(c.B)} drift={C.drift(name):.3e} bound={bound:.3e} '
          f'err={err:.3e} status={status}')
    assert status == 0
    assert got.shape == (c.B, c.L, c.NC) and got.dtype == np.float32
    assert np.isfinite(got).all()
    assert err <= bound, (name, err, bound)


@pytest.mark.parametrize('name', ['b17', 'fold42'])
def test_repeat_launch_is_bit_identical(name):
    c = C.case(name)
    m = C.build_model(c.cfg, c.sd, DEV)
    a, sa = C.gpu_logits(c, m)
    b, sb = C.gpu_logits(c, m)
    assert sa == sb == 0
    assert np.array_equal(a, b)


@pytest.mark.parametrize('bits,mode', [(8, 'RAW'), (4, 'RAW'), (9, 'MOL')])
def test_draws_off_the_default_config(bits, mode):
    """19 folds of 60 at hop 6 (1140 draws), then generate()'s tail: mu-law at 256 / 16 classes."""
    factors, T, target, overlap, seed = (2, 3), 171, 50, 5, 40 + bits
    cfg = C.small_config(factors, bits, mode)
    m = C.build_model(cfg, C.state_dict(factors, bits, mode, seed), DEV)
    assert m.n_classes == (30 if mode == 'MOL' else 2 ** bits)
    rng = np.random.Generator(np.random.PCG64(seed))
    mels = (rng.normal(0.0, 1.0, (1, 80, T)) - 4.0).astype(np.float32)
    smp = C.check_draws(m, cfg, mels, seed, target, overlap)
    assert smp.shape == (19, 60) and smp.size >= 1000
    if mode == 'RAW':  # every sample is a class value
        idx = np.rint((smp + 1.0) * (m.n_classes - 1) / 2.0)
        assert idx.min() >= 0 and idx.max() <= m.n_classes - 1
        assert np.array_equal(smp, (2.0 * idx.astype(np.float32) / np.float32(m.n_classes - 1) - 1.0).astype(np.float32))
        assert len(np.unique(idx)) >= 2
    wav = m.generate(torch.from_numpy(mels), True, target, overlap, True, seed=seed)
    ref = wr.finish(smp.astype(np.float64), True, target, overlap, mode == 'RAW', m.n_classes,
                    (T - 1) * 6, 6)
    assert wav.dtype == np.float64 and wav.shape == ref.shape == ((T - 1) * 6,)
    np.testing.assert_allclose(wav, ref, rtol=0, atol=1e-12)


def test_bits_10_is_refused_before_any_launch():
    cfg = C.small_config((2, 3), 10)
    m = C.build_model(cfg, C.state_dict((2, 3), 10, 'RAW', 1), DEV)
    assert m.n_classes == 1024
    mels = torch.zeros(1, 80, 9) - 4.0
    with pytest.raises(_lib.FtmiError, match='ftmi_wavernn failed with status 1003'):
        m.forward(torch.zeros(1, 30), mels)
    with pytest.raises(_lib.FtmiError, match='ftmi_wavernn failed with status 1003'):
        m.generate_samples(mels, True, 20, 5, seed=1)
    torch.cuda.synchronize()
    assert int(ops.status_word(torch.device(DEV)).item()) == 0


# ---------------------------------------------------------------------------------------
# ftmi_wr_stretch_conv

def _crop(kind, W, s):
    return {'full': (0, W * s), 'first': (0, 1), 'last': (W * s - 1, 1),
            'indent': (s, W * s - 2 * s), 'odd': (1, W * s - 1)}[kind]


STRETCH = [(1, (1, 1, 80), 'full'), (1, (3, 5, 80), 'indent'), (2, (3, 5, 80), 'full'),
           (2, (2, 7, 33), 'first'), (3, (2, 7, 33), 'last'), (3, (3, 5, 80), 'odd'),
           (8, (2, 7, 33), 'indent'), (8, (1, 1, 80), 'last'), (8, (3, 5, 80), 'full'),
           (2, (1, 1, 80), 'odd'), (3, (1, 1, 80), 'first')]


def test_stretch_conv_table_covers_every_value():
    assert {s for s, _, _ in STRETCH} == {1, 2, 3, 8}
    assert {shape for _, shape, _ in STRETCH} == {(1, 1, 80), (3, 5, 80), (2, 7, 33)}
    assert {k for _, _, k in STRETCH} == {'full', 'first', 'last', 'indent', 'odd'}
    for s, (_, W, _), kind in STRETCH:
        c0, wo = _crop(kind, W, s)
        assert c0 >= 0 and wo >= 1 and c0 + wo <= W * s


@pytest.mark.parametrize('s,shape,kind', STRETCH)
def test_stretch_conv_matches_fp64(s, shape, kind):
    B, W, Cn = shape
    crop0, W_out = _crop(kind, W, s)
    taps = 2 * s + 1
    rng = np.random.Generator(np.random.PCG64([s, B, W, Cn]))
    x = rng.uniform(-1, 1, (B, W, Cn)).astype(np.float32)
    x[:, :, 0] = 0.0  # a channel of zeros: its outputs are exactly zero
    w = rng.uniform(-1, 1, taps).astype(np.float32)
    assert not np.allclose(w, w[::-1])
    got = ops.wr_stretch_conv(torch.from_numpy(x).to(DEV), s, torch.from_numpy(w).to(DEV),
                              W_out=None if kind == 'full' else W_out, crop0=crop0).cpu().numpy()

    def ref(xa, wa):
        v = wr.stretch2d(torch.from_numpy(xa).double().transpose(1, 2).unsqueeze(1), s, 1)
        y = F.conv2d(v, torch.from_numpy(wa).double().view(1, 1, 1, taps), padding=(0, s))
        return y.squeeze(1).transpose(1, 2)[:, crop0:crop0 + W_out].numpy()

    want, mag = ref(x, w), ref(np.abs(x), np.abs(w))
    bound = (taps + 2) * 2.0 ** -24 * mag
    err = np.abs(got - want)
    ratio = float((err[mag > 0] / bound[mag > 0]).max())
    print(f'WR stretch s={s} shape={shape} crop={kind} max_err={err.max():.3e} max_err_over_bound={ratio:.3f}')
    assert got.shape == (B, W_out, Cn)
    assert np.all(got[mag == 0] == 0.0) and np.all(got[:, :, 0] == 0.0)
    assert np.all(err <= bound), ratio


def test_stretch_conv_refuses_a_crop_past_the_end():
    x = torch.zeros(2, 5, 80, device=DEV)
    w = torch.ones(7, device=DEV)
    with pytest.raises(_lib.FtmiError, match='status 1002'):
        ops.wr_stretch_conv(x, 3, w, W_out=15, crop0=1)
    with pytest.raises(ValueError):
        ops.wr_stretch_conv(x, 3, torch.ones(5, device=DEV))
    torch.cuda.synchronize()


def test_upsample_with_trained_like_taps_matches_reference():
    """The reference's UpsampleNetwork on non-uniform smoothers (factors [2, 3]): tap order and
    layer order show.  Tolerance of test_gpu_wavernn.py::test_upsample_matches_reference."""
    g = load_golden('wr_upsample_taps')
    cfg = C.small_config((2, 3), 9)
    sd = C.state_dict((2, 3), 9, 'RAW', 0)
    sd['upsample.up_layers.1.weight'] = torch.from_numpy(g['w1'])
    sd['upsample.up_layers.3.weight'] = torch.from_numpy(g['w3'])
    m = C.build_model(cfg, sd, DEV)
    up, aux = m.upsample_forward(torch.from_numpy(g['mels']).to(DEV))
    for got, ref in ((up, g['up']), (aux, g['aux'])):
        np.testing.assert_allclose(got.cpu().numpy(), ref, rtol=1e-5, atol=2e-6 * np.abs(ref).max())


# ---------------------------------------------------------------------------------------
# ftmi_wr_unfold

def _samples(rng, B, L, mu_law, nc):
    """fp32 sample values: exact class values 2 i / (NC - 1) - 1 (mu-law) or N(0, 1), with
    -1, +1 and 0 planted."""
    if mu_law:
        i = rng.integers(0, nc, (B, L)).astype(np.float32)
        y = (2.0 * i / np.float32(nc - 1) - np.float32(1.0)).astype(np.float32)
    else:
        y = rng.normal(0.0, 1.0, (B, L)).astype(np.float32)
    flat = y.reshape(-1)
    for k, v in enumerate((-1.0, 1.0, 0.0)):
        flat[(k * 5) % flat.size] = v
    return y


MU = [(False, 512), (True, 2), (True, 16), (True, 256), (True, 512)]


@pytest.mark.parametrize('B,target,overlap', [(1, 5, 1), (3, 1, 1), (3, 1, 3), (5, 4, 3), (2, 7, 10)])
def test_unfold_matches_oracle_tail(B, target, overlap):
    stride, L = target + overlap, target + 2 * overlap
    full = B * stride + overlap
    waves = sorted({w for w in (full, full - 1, B * stride - 1, (B - 1) * stride + 1, 1) if w >= 1})
    rng = np.random.Generator(np.random.PCG64([B, target, overlap]))
    worst = 0.0
    for mu_law, nc in MU:
        y = _samples(rng, B, L, mu_law, nc)
        yd = torch.from_numpy(y).to(DEV)
        for wave_len in waves:
            for fade in sorted({0, 1, wave_len}):
                got = ops.wr_unfold(yd, target, overlap, True, mu_law, nc, wave_len, fade).cpu().numpy()
                ref = C.finish_ref(y, True, target, overlap, mu_law, nc, wave_len, fade)
                assert got.dtype == np.float64 and got.shape == ref.shape == (wave_len,)
                worst = max(worst, float(np.abs(got - ref).max()))
                np.testing.assert_allclose(got, ref, rtol=0, atol=1e-12,
                                           err_msg=str((mu_law, nc, wave_len, fade)))
    print(f'WR unfold B={B} target={target} overlap={overlap} worst={worst:.3e}')


def test_unfold_unbatched_uses_row_0():
    rng = np.random.Generator(np.random.PCG64(8))
    for mu_law, nc in MU:
        y = _samples(rng, 2, 9, mu_law, nc)
        yd = torch.from_numpy(y).to(DEV)
        for wave_len in (9, 8, 1):
            for fade in sorted({0, 1, wave_len}):
                got = ops.wr_unfold(yd, 5, 2, False, mu_law, nc, wave_len, fade).cpu().numpy()
                ref = C.finish_ref(y, False, 5, 2, mu_law, nc, wave_len, fade)
                np.testing.assert_allclose(got, ref, rtol=0, atol=1e-12)


def test_unfold_reference_has_no_overlap_0():
    with pytest.raises(ValueError):
        wr.xfade_and_unfold(np.zeros((2, 5)), 5, 0)


def test_unfold_shape_errors():
    y = torch.zeros(3, 7, device=DEV)
    for args in ((1, 3, True, False, 512, 16, 0),    # wave_len > B stride + overlap = 15
                 (1, 3, True, False, 512, 10, 11),   # wave_len < fade_len
                 (2, 3, True, False, 512, 10, 0),    # L != target + 2 overlap
                 (1, 3, False, False, 512, 8, 0)):   # unbatched: wave_len > L
        with pytest.raises(_lib.FtmiError, match='status 1002'):
            ops.wr_unfold(y, *args)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------
# one instance (FTMI_WR_NI=1): <16,1>, <32,1>

_CHILD = r'''
import json, sys
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np, torch
import wr_cases as C
for B in (9, 17, 32):
    c = C.Case('b1', B=B)
    got, status = C.gpu_logits(c, C.build_model(c.cfg, c.sd, 'cuda'))
    l64 = C.run_oracle(c, torch.float64)
    d = float(np.abs(C.run_oracle(c, torch.float32) - l64).max())
    finite = bool(np.isfinite(got).all())
    err = float(np.abs(got - l64).max()) if finite else -1.0
    print('WRNI1 ' + json.dumps(dict(B=B, shape=list(got.shape), finite=finite, status=status,
                                     err=err, drift=d, bound=C.bound_from(d))), flush=True)
'''


def test_one_instance_launches():
    env = dict(os.environ, FTMI_WR_NI='1')
    script = _CHILD.format(root=str(ROOT), tests=str(ROOT / 'tests'))
    r = subprocess.run([sys.executable, '-c', script], env=env, cwd=str(ROOT), capture_output=True,
                       text=True, timeout=240)
    print(r.stdout)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [json.loads(l[6:]) for l in r.stdout.splitlines() if l.startswith('WRNI1 ')]
    assert [row['B'] for row in rows] == [9, 17, 32]
    for row in rows:
        assert row['shape'] == [row['B'], 30, 512] and row['finite'] and row['status'] == 0
        assert 1e-4 <= row['bound'] <= 5e-4
        assert 0 <= row['err'] <= row['bound'], row
