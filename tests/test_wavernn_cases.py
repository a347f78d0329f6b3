"""CPU side of the WaveRNN launch-shape tests (tests/test_gpu_wavernn_cases.py), on the oracle
alone (tests/wr_cases.py): the table reaches the launches it claims, its folds cannot be
mistaken for one another, and the defects those tests exist to catch — planted in the oracle's
inputs only — each move the named case's logits by more than 10 bounds (or change a draw)."""
import numpy as np
import pytest
import torch

import wr_cases as C
from forwardtacotron_amd.wavernn import WaveRNN
from oracle import wr_torch_cpu as wr

NAMES = list(C.CASES)
FOLDS = [n for n in NAMES if C.CASES[n].get('fold')]


def test_small_configs_are_accepted():
    """The oracle and WaveRNN.from_config both take factors [1], [3], [2, 3] and bits 1, 4, 8, 9."""
    for factors in ([1], [3], [2, 3]):
        for bits in (1, 4, 8, 9):
            cfg = C.small_config(factors, bits)
            hop = int(np.prod(factors))
            m = WaveRNN.from_config(cfg)
            assert m.n_classes == 2 ** bits and m.hop_length == hop
            assert m.fc3.weight.shape == (2 ** bits, 512)
            assert [l.weight.numel() for l in m.upsample.up_layers[1::2]] == [2 * s + 1 for s in factors]
    for factors in ([1], [3], [2, 3]):
        sd = C.state_dict(factors, 9, 'RAW', 5)
        hop = int(np.prod(factors))
        up, aux = wr.upsample(sd, torch.zeros(1, 80, 6) - 4.0, C.model_cfg(C.small_config(factors, 9)))
        assert up.shape == (1, 2 * hop, 80) and aux.shape == (1, 2 * hop, 128)
        taps = sd['upsample.up_layers.1.weight'].flatten()
        assert not torch.allclose(taps, taps.flip(0))  # non-uniform, not symmetric


def test_table_reaches_the_launch_shapes():
    seen = set()
    for n in NAMES:
        c = C.case(n)
        got = C.launches(c.B)
        assert got == C.LAUNCHES[n], (n, got)
        seen |= {(nbv, ni) for nbv, ni, _, _ in got}
    assert seen == {(8, 1), (8, 2), (16, 2)}
    assert any(f0 > 0 for n in NAMES for _, _, f0, _ in C.LAUNCHES[n])
    # the uneven splits between the two instances, and the table's shapes
    assert C.instance_split(3, 2) == [2, 1] and C.instance_split(17, 2) == [9, 8]
    assert C.instance_split(32, 2) == [16, 16] and C.instance_split(16, 2) == [8, 8]
    shape = {n: (C.case(n).B, C.case(n).L, C.case(n).NC, C.case(n).hop) for n in NAMES}
    assert shape == {
        'b1': (1, 30, 512, 6), 'b3': (3, 30, 512, 6), 'b16': (16, 30, 512, 6),
        'b17': (17, 30, 512, 6), 'b32': (32, 30, 512, 6), 'b33': (33, 30, 512, 6),
        'b35': (35, 30, 512, 6), 'nc256': (3, 30, 256, 6), 'nc16': (5, 30, 16, 6),
        'nc2': (3, 3, 2, 3), 'l1': (2, 1, 512, 1), 'l2': (2, 2, 512, 1), 'mol3': (3, 30, 30, 6),
        'mol17': (17, 30, 30, 6), 'hop256': (3, 512, 512, 256), 'fold42': (42, 4, 512, 6),
        'fold2': (2, 30, 512, 6)}
    # the one-instance launches of the FTMI_WR_NI=1 test
    assert [C.launches(b, 1) for b in (9, 17, 32)] == [[(16, 1, 0, 9)], [(32, 1, 0, 17)], [(32, 1, 0, 32)]]


def test_fold_cases_pad_and_every_long_case_crosses_a_frame():
    assert sorted(FOLDS) == ['fold2', 'fold42']
    for n in FOLDS:
        c = C.case(n)
        assert c.padded_positions() == 1, (n, c.padded_positions())
        # wr.conditioning agrees on the fold count and zero-fills exactly that position
        m, aux, _ = wr.conditioning(c.sd, c.mcfg, c.mels, True, *c.fold)
        assert m.shape == (c.B, c.L, 80) and aux.shape == (c.B, c.L, 128)
        padded = torch.from_numpy(c.positions() >= c.total_len)
        assert bool((m[padded] == 0).all()) and bool((aux[padded] == 0).all())
        assert bool((m[~padded].abs().sum(-1) > 0).all())
    for n in NAMES:
        c = C.case(n)
        if c.L > c.hop:
            g = np.minimum(c.positions(), (c.total_len if c.fold else c.L) - 1) // c.hop
            assert (g.max(axis=1) > g.min(axis=1)).all(), n
    assert len(set((C.case('b1').positions()[0] // 6).tolist())) == 5  # 5 frames: 4 changes + start


@pytest.mark.parametrize('name', NAMES)
def test_bound_and_distinguishable_folds(name):
    c, l64 = C.case(name), C.oracle(name)
    d, b = C.drift(name), C.bound(name)
    assert l64.shape == (c.B, c.L, c.NC) and np.isfinite(l64).all()
    assert 0 < d < 5e-5, d  # fp32 rounding of the reference arithmetic, nothing else
    assert b <= C.existing_bar(l64), (b, C.existing_bar(l64))
    for i in range(c.B):
        for j in range(i):
            assert np.abs(l64[i] - l64[j]).max() > 10 * b, (name, i, j)


# defect -> the named case that must catch it
CAUGHT_BY = {
    'frame_shift': 'b1', 'mel_mod32': 'b33', 'pad_nonzero': 'fold42', 'taps0_reversed': 'b3',
    'taps1_reversed': 'b3', 'smoothers_swapped': 'b3', 'x_zero': 'b1', 'a1_zero': 'b3',
    'a2_zero': 'b3', 'a3_zero': 'b3', 'a4_zero': 'b3', 'inactive_class_finite': 'nc16',
}


def test_every_defect_is_listed():
    assert sorted(CAUGHT_BY) == sorted(C.DEFECTS)
    assert sorted(C.DEFECTS) == ['a1_zero', 'a2_zero', 'a3_zero', 'a4_zero', 'frame_shift',
                                 'inactive_class_finite', 'mel_mod32', 'pad_nonzero',
                                 'smoothers_swapped', 'taps0_reversed', 'taps1_reversed', 'x_zero']


@pytest.mark.parametrize('defect', sorted(d for d in CAUGHT_BY if d != 'inactive_class_finite'))
def test_planted_defect_is_caught(defect):
    name = CAUGHT_BY[defect]
    good, bad = C.oracle(name), C.oracle(name, torch.float64, defect)
    ratio = float(np.abs(bad - good).max()) / C.bound(name)
    assert ratio > 10, (defect, name, ratio)
    if defect == 'mel_mod32':  # only item 32 reads another item's mels
        assert np.array_equal(bad[:32], good[:32])
    if defect == 'pad_nonzero':  # only the last fold has a padded position
        assert np.array_equal(bad[:-1], good[:-1])


def test_inactive_classes_would_change_a_draw():
    """nc16: 496 of the 512 fc3 rows are past n_classes.  Were their partials finite instead of
    -inf, the restated Gumbel argmax would pick them."""
    l64 = C.oracle('nc16')
    good = C.gumbel_draws(l64, 7)
    assert good.max() < 16 and np.array_equal(good, C.gumbel_draws(l64, 7, slots=16))
    bad = C.gumbel_draws(l64, 7, slots=512, fill=0.0)
    assert (bad != good).any() and bad.max() >= 16


def test_relu_sees_both_signs():
    p1, p2, logits = C.preactivations('b3')
    np.testing.assert_allclose(logits, C.oracle('b3'), rtol=0, atol=1e-12)
    for p in (p1, p2):
        assert 0.2 < (p > 0).mean() < 0.8 and p.min() < -0.1 and p.max() > 0.1


def test_oracle_runs_in_fp64_and_fp32_is_unchanged():
    """The oracle's states follow the weights' dtype; on fp32 weights the outputs are fp32."""
    c = C.case('l2')
    sd32 = c.sd
    out = wr.forward(sd32, c.mcfg, c.x, c.mels)
    assert out.dtype == torch.float32
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd32.items()}
    assert wr.forward(sd64, c.mcfg, c.x.double(), c.mels.double()).dtype == torch.float64
    # forward and generate(forced=...) agree once the input is shifted by a step: the shift
    # wr_cases gives the kernel's xin in the fold cases
    mg = c.mels.double()  # generate pads by `pad` frames a side: 6 samples at hop 1
    xg = torch.from_numpy(np.random.Generator(np.random.PCG64(3)).uniform(-1, 1, (c.B, 6)))
    tr = []
    wr.generate(sd64, c.mcfg, mg, batched=False, forced=xg, trace=tr, steps=6)
    xf = torch.nn.functional.pad(xg, (1, 0))[:, :-1]
    want = wr.forward(sd64, c.mcfg, xf, wr.pad_tensor(mg.transpose(1, 2), c.pad).transpose(1, 2))
    np.testing.assert_allclose(torch.stack(tr, 1).numpy(), want.numpy(), rtol=0, atol=1e-12)
