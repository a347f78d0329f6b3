"""The Tacotron decoder launch (csrc/tacotron.hip, `Decoder.launch`) on its own inputs against
the fp64 CPU oracle (tests/taco_decoder_cases.py): 257..512 tokens (a workgroup's second
token), r up to 20 (1600 live mel_proj rows), the attention peak on tokens 0 / 255 / 256 /
T-1 and on the location window's edges, T = 1, 2, 31, and the device-side stop rule where one
value of the step's r frames decides it.

Both sides receive the same fp32 enc / enc_proj, so no encoder or postnet error enters.
Bounds: max(1e-4, 10 drift) for mel, max(1e-5, 10 drift) for attn, drift = the oracle's own
fp32-vs-fp64 difference on the case (tests/test_tacotron_decoder_cases.py asserts they are
<= 2e-3 / 1e-4 and that the planted defects break them)."""
import numpy as np
import pytest
import torch

import taco_decoder_cases as C

pytestmark = pytest.mark.gpu

NAMES = list(C.CASES)


@pytest.fixture(scope='module')
def decoders():
    """{loud key: Decoder on the device}: the synthetic `decoder.*` tensors, and the copy with
    the scaled mel_proj row for the case that has one."""
    from forwardtacotron_amd.tacotron import Decoder
    out = {}
    for loud in {C.case(n).loud for n in NAMES}:
        d = Decoder(80, 256, 512)
        d.load_state_dict({k[len('decoder.'):]: v for k, v in C.decoder_sd(torch.float32, loud).items()
                           if k.startswith('decoder.')})
        out[loud] = d.to('cuda').eval()
    return out


def launch(decoders, name):
    """-> (mel (B, n r, 80), attn (B, n, T), steps word, status word) as numpy / ints."""
    from forwardtacotron_amd import ops
    case = C.case(name)
    dec = decoders[case.loud]
    enc, ep = case.enc.cuda(), case.enc_proj.cuda()
    st = ops.status_word('cuda')
    st.zero_()
    if case.mode == 'forced':
        # case.prenet_in: the teacher frames sliced as Tacotron._forward slices them
        mel, attn, n = dec.launch(enc, ep, case.r, case.frames, 0.0, case.prenet_in.cuda().contiguous())
    else:
        mel, attn, n = dec.launch(enc, ep, case.r, case.frames, case.thr)
    torch.cuda.synchronize()
    assert mel.shape == (case.B, case.n * case.r, 80) and attn.shape == (case.B, case.n, case.T)
    return mel.cpu().numpy(), attn.cpu().numpy(), int(n.item()), int(st.item())


@pytest.mark.parametrize('name', NAMES)
def test_case(decoders, name):
    case, o = C.case(name), C.oracle(name)
    mel, attn, steps, status = launch(decoders, name)
    assert status == 0
    want = o['steps']
    if case.mode == 'forced':
        assert want == -(-case.frames // case.r)
    assert steps == want
    if 'want' in case.cfg:
        assert (steps * case.r, steps) == case.cfg['want']
    assert not mel[:, want * case.r:].any() and not attn[:, want:].any()
    mel, attn = mel[:, :want * case.r], attn[:, :want]
    bm, ba = C.bounds(name)
    dm, da = C.drift(name)
    em, ea = float(np.abs(mel - o['mel']).max()), float(np.abs(attn - o['attn']).max())
    print(f'{name}: mel {em:.3e} / {bm:.3e} (drift {dm:.2e})  attn {ea:.3e} / {ba:.3e} '
          f'(drift {da:.2e})  steps {steps}')
    assert np.isfinite(mel).all() and np.isfinite(attn).all()
    assert em <= bm and ea <= ba
    sure = C.decided_steps(o['attn'], ba)
    assert sure.mean() >= 0.8
    assert (attn.argmax(-1)[sure] == o['attn'].argmax(-1)[sure]).all()
    assert np.abs(attn.astype(np.float64).sum(-1) - 1.0).max() <= 1e-5


def test_repeat_launch_is_bit_identical(decoders):
    """Every sum in a fixed order, and the per-stream workspace reused across launches of
    other shapes: the same case before and after a T = 1 launch gives the same bits."""
    a = launch(decoders, 'forced_t512_r20')
    b = launch(decoders, 'forced_t1_r3')
    c = launch(decoders, 'forced_t512_r20')
    assert a[2:] == c[2:] == (4, 0) and b[2:] == (4, 0)
    assert np.array_equal(a[0].view(np.int32), c[0].view(np.int32))
    assert np.array_equal(a[1].view(np.int32), c[1].view(np.int32))


def test_workspace_bytes():
    from forwardtacotron_amd import _lib
    f = _lib.load().ftmi_tacotron_decoder_workspace_bytes
    assert f(3, 40) == 0 and f(1, 0) == 0 and f(1, 513) == 0 and f(0, 40) == 0
    for name in NAMES:
        c = C.CASES[name]
        assert f(c['B'], c['T']) > 0, name
