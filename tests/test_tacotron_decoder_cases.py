"""CPU side of the decoder-level Tacotron tests (tests/test_gpu_tacotron_decoder.py), on the
oracle alone (tests/taco_decoder_cases.py): the preconditions that make the cases worth
running — bounds small enough to say something, peaked attention that reaches tokens >= 256,
a stop rule one value decides — and the defects those tests exist to catch, planted in the
oracle only, each breaking an asserted quantity of a named case by more than 10 bounds or
changing its frame count."""
import numpy as np
import pytest
import torch

import taco_decoder_cases as C

NAMES = list(C.CASES)
STOPS = [n for n in NAMES if 'want' in C.CASES[n]]


def test_table_reaches_the_unexercised_code():
    """The shapes the issue names: both token passes, every live-row slot, n_live below and
    off a multiple of 256, T at and under the window, both modes at r = 20."""
    c = C.CASES
    shapes = {(v['mode'], v['B'], v['T'], v['r']) for v in c.values()}
    assert shapes >= {('forced', 2, 512, 20), ('forced', 2, 257, 7), ('forced', 2, 256, 13),
                      ('forced', 1, 255, 3), ('forced', 2, 300, 3), ('forced', 1, 1, 3),
                      ('forced', 2, 2, 1), ('forced', 1, 31, 2), ('free', 1, 512, 1),
                      ('free', 1, 384, 20), ('free', 1, 40, 10), ('free', 1, 40, 11),
                      ('free', 1, 40, 20), ('free', 1, 40, 3)}
    assert c['forced_t255_r3']['frames'] % 3 != 0
    assert c['forced_t512_r20']['peaks'] == (511, 256) and c['forced_t257_r7']['peaks'] == (256, 0)


@pytest.mark.parametrize('name', NAMES)
def test_preconditions(name):
    case, o = C.case(name), C.oracle(name)
    bm, ba = C.bounds(name)
    assert bm <= 2e-3 and ba <= 1e-4, (bm, ba)
    attn, mel = o['attn'], o['mel']
    assert attn.shape == (case.B, o['steps'], case.T) and mel.shape == (case.B, o['steps'] * case.r, 80)
    if case.mode == 'forced':
        assert o['steps'] == case.n == -(-case.frames // case.r)
    if case.T > 1:
        assert attn.max(-1).mean() >= 0.3
    if case.T >= 257:
        assert (attn.argmax(-1) >= 256).any()
    assert 1.0 <= np.abs(mel).mean() <= 10.0
    # the GPU test's argmax check has something to check
    assert C.decided_steps(attn, ba).mean() >= 0.8
    peaks = case.cfg['peaks']
    if peaks is not None:
        top = np.sort(attn[:, 0], -1)
        assert (attn[:, 0].argmax(-1) == np.array(peaks)).all()
        assert ((top[:, -1] - top[:, -2]) > 10 * ba).all()


def test_place_peak_moves_the_step0_argmax_exactly():
    """Step 0 sees cum = att = 0: a roll along T rolls the weights (to fp64 rounding)."""
    g = torch.Generator().manual_seed(5)
    enc = torch.tanh(torch.randn(2, 300, 256, generator=g))
    ep = torch.nn.functional.linear(enc, C.decoder_sd()['encoder_proj.weight'])
    a0 = C.step0_attention(enc, ep)
    e2, p2 = C.place_peak(enc, ep, (299, 7))
    a1 = C.step0_attention(e2, p2)
    for b, p in enumerate((299, 7)):
        sh = p - int(a0[b].argmax())
        assert int(a1[b].argmax()) == p
        assert torch.allclose(a1[b], torch.roll(a0[b], sh), rtol=0, atol=1e-12)


@pytest.mark.parametrize('name', STOPS)
def test_stop_cases(name):
    case = C.case(name)
    frames, rows = case.cfg['want']
    for dt in (torch.float64, torch.float32):
        o = C.oracle(name, dt)
        assert o['mel'].shape[1] == frames and o['attn'].shape[1] == rows == o['steps']
        assert rows * case.r < case.frames  # the rule ended the run, not the step limit
    if name == 'stop_loud_r3':
        fig = C.loud_conditions(name)
        assert fig['alone'] >= 1 and fig['steps'] >= 7
        assert fig['others_margin'] >= 1e-2 and fig['row_margin'] >= 1e-2
        a = (C.N_MELS - 1) * case.r + case.r - 2  # the scaled value's live row
        assert a == C.N_MELS * case.r - 2 and a % 256 >= 200  # a high workgroup


def broken(name, defect):
    """(frame count changed, worst err / bound over mel and attn) of a defect on a case."""
    good, bad = C.oracle(name), C.oracle(name, torch.float64, defect)
    if bad['steps'] != good['steps']:
        return True, float('inf')
    bm, ba = C.bounds(name)
    return False, max(float(np.abs(bad['mel'] - good['mel']).max()) / bm,
                      float(np.abs(bad['attn'] - good['attn']).max()) / ba)


# defect -> the named cases that must catch it, and how
CAUGHT_BY = {
    'a': (['forced_t512_r20', 'forced_t257_r7', 'free_t512_r1'], 'bound'),
    'b': (['forced_t512_r20', 'forced_t300_r3', 'forced_t2_r1', 'forced_t31_r2'], 'bound'),
    'c': (['forced_t300_r3', 'forced_t2_r1'], 'bound'),
    'd': (['forced_t300_r3', 'forced_t257_r7', 'free_t512_r1'], 'bound'),
    'e': (['free_t384_r20'], 'bound'),
    'f': (['forced_t512_r20', 'free_t384_r20'], 'bound'),
    'g': (['stop_loud_r3'], 'frames'),
    'h': (['stop_r10'], 'frames'),
}


def test_every_defect_is_listed():
    assert sorted(CAUGHT_BY) == sorted(C.DEFECTS)


@pytest.mark.parametrize('defect', sorted(CAUGHT_BY))
def test_planted_defect_is_caught(defect):
    names, how = CAUGHT_BY[defect]
    for name in names:
        changed, ratio = broken(name, defect)
        if how == 'frames':
            assert changed, (defect, name)
        else:
            assert not changed and ratio > 10, (defect, name, ratio)


def test_stop_defects_change_the_frame_count_as_reasoned():
    """g: the scaled value sits in frame r - 2, so a scan of the last frame alone stops at the
    first step with t > 10 (s = 4: 15 frames instead of 21).  h: t = 10 at s = 1 of r = 10
    (20 frames instead of 30)."""
    assert C.oracle('stop_loud_r3', torch.float64, 'g')['mel'].shape[1] == 15
    assert C.oracle('stop_r10', torch.float64, 'h')['mel'].shape[1] == 20
    # and neither touches a case where every value decides the same way and t = 10 never occurs
    assert C.oracle('stop_r11', torch.float64, 'g')['steps'] == C.oracle('stop_r11')['steps']
    assert C.oracle('stop_r11', torch.float64, 'h')['steps'] == C.oracle('stop_r11')['steps']


def test_oracle_loops_restate_taco_torch_cpu():
    """With no defect the free-running loop is taco_torch_cpu.generate's (same step function,
    same rule): the frame fed back and the stop step agree bit for bit on a short run."""
    import taco_torch_cpu as TC
    case = C.case('stop_r10')
    sd = case.sd(torch.float64)
    enc, ep = case.enc.double(), case.enc_proj.double()
    st = TC.DecoderState(sd, enc)
    last, mels = torch.zeros(1, 80, dtype=torch.float64), []
    with torch.no_grad():
        for t in range(0, case.frames, case.r):
            fr, _ = TC.decoder_step(sd, st, enc, ep, mels[-1][:, :, -1] if t > 0 else last, case.r)
            mels.append(fr)
            if bool((fr < case.thr).all()) and t > 10:
                break
    want = torch.cat(mels, 2).transpose(1, 2).numpy()
    assert np.array_equal(want, C.oracle('stop_r10')['mel'])
