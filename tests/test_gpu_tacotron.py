"""Tacotron on the HIP path (forwardtacotron_amd/tacotron.py, csrc/tacotron.hip: the decoder
loop as one persistent launch) against the reference goldens.

Bounds, read from goldens_tacotron.json: |d mel|, |d linear| <= max(1e-4, 10 drift64) and
|d attn| <= max(1e-5, 10 drift64), drift64 = the reference's own fp32-vs-fp64 difference on
the case: the HIP path differs from the fp32 reference by summation order, expf and the f16x3
encoder / postnet, each a perturbation of fp32-rounding size, and drift64 measures the
feedback's amplification of such perturbations."""
import json

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu

META = json.loads((GOLDEN / 'goldens_tacotron.json').read_text())['cases']


@pytest.fixture(scope='module')
def model():
    from forwardtacotron_amd.synthetic import default_config, synthetic_array
    from forwardtacotron_amd.tacotron import Tacotron
    keys = json.loads((GOLDEN / 'tacotron_state_dict_keys.json').read_text())
    m = Tacotron.from_config(default_config())
    m.load_state_dict({k: torch.from_numpy(synthetic_array(k, shape, dt, 0, 'tacotron'))
                       for k, shape, dt in keys})
    return m.to('cuda').eval()


def run(model, name):
    info, g = META[name], load_golden(f'taco_{name}')
    model.r = info['r']
    x = torch.from_numpy(g['x']).cuda()
    if info['mode'] == 'generate':
        model.stop_threshold = model.stop_threshold.new_tensor(info['stop_threshold'])
        out = model.generate(x, steps=info['steps'])
    else:
        model.eval()
        out = [o.cpu().numpy() for o in model(x, torch.from_numpy(g['m']).cuda())]
    return info, g, out


def check(info, g, out, argmax=False):
    mel, lin, attn = out
    assert mel.shape == g['mel'].shape and lin.shape == g['linear'].shape and attn.shape == g['attn'].shape
    d = info['drift64']
    bm, bl, ba = max(1e-4, 10 * d['mel']), max(1e-4, 10 * d['linear']), max(1e-5, 10 * d['attn'])
    em, el, ea = (float(np.abs(a - b).max()) for a, b in ((mel, g['mel']), (lin, g['linear']), (attn, g['attn'])))
    print(f'mel {em:.3e} / {bm:.3e}  linear {el:.3e} / {bl:.3e}  attn {ea:.3e} / {ba:.3e}')
    assert em <= bm and el <= bl and ea <= ba
    if argmax:
        ref = g['attn'].reshape(-1, attn.shape[-1])
        top = np.sort(ref, -1)
        sure = (top[:, -1] - top[:, -2]) > 10 * ba
        assert sure.mean() >= 0.8
        assert (attn.reshape(ref.shape).argmax(-1)[sure] == ref.argmax(-1)[sure]).all()


@pytest.mark.parametrize('name', ['gen_t7', 'gen_t45_r2', 'gen_t70', 'gen_t45_r5'])
def test_generate(model, name):
    info, g, out = run(model, name)
    assert model.training  # generate leaves the module in training mode, like the reference
    check(info, g, out, argmax=name == 'gen_t70')


@pytest.mark.parametrize('r,frames,rows', [(1, 12, 12), (2, 14, 7), (5, 20, 4)])
def test_unconditional_stop(model, r, frames, rows):
    """stop_threshold = +1e9: the device-side rule ends at the first step with t > 10."""
    info, g, out = run(model, f'stop_r{r}')
    assert out[0].shape == (80, frames) and out[2].shape == (rows, 20)
    check(info, g, out)


def test_value_dependent_stop(model):
    """A threshold the per-step maxima clear by >= 1e-2 up to the stop (asserted on the
    reference): the frame count must be the reference's."""
    info, g, out = run(model, 'stop_value')
    assert info['frames'] > 20 and out[0].shape[1] == info['frames']
    check(info, g, out)


@pytest.mark.parametrize('name', ['fwd_b3', 'fwd_b2'])
def test_forward(model, name):
    info, g, out = run(model, name)
    check(info, g, out, argmax=name == 'fwd_b3')


def test_guard_refuses_when_not_resident(model):
    """With the CUs the residency check may count lowered, the decoder call returns
    FTMI_E_UNSUPPORTED before its memset or its launch (status word clean)."""
    from forwardtacotron_amd import _lib, ops
    g = load_golden('taco_gen_t7')
    x = torch.from_numpy(g['x']).cuda()
    model.r = 1
    enc, enc_proj = model._encode(x)
    lib = _lib.load()
    st = ops.status_word('cuda')
    st.zero_()
    prev = lib.ftmi_set_resident_cu_limit(8)
    try:
        with pytest.raises(_lib.FtmiError, match='status 1003'):
            model.decoder.launch(enc, enc_proj, 1, 12, -11.0)
        torch.cuda.synchronize()
        assert int(st.item()) == 0
    finally:
        lib.ftmi_set_resident_cu_limit(prev)
    mel, attn, n = model.decoder.launch(enc, enc_proj, 1, 12, -11.0)
    torch.cuda.synchronize()
    assert int(n.item()) == 12 and torch.isfinite(mel).all() and int(st.item()) == 0


def test_token_limit(model):
    from forwardtacotron_amd import _lib, ops
    x = torch.ones(1, ops.TACO_MAX_TOKENS + 1, dtype=torch.long, device='cuda')
    with pytest.raises(_lib.FtmiError, match='UNSUPPORTED'):
        model.generate(x, steps=4)


def test_forward_in_training_mode(model):
    """Like ForwardTacotron.forward here: a call in training mode advances `step` and still
    computes the inference result (no dropout, no zoneout)."""
    info, g = META['fwd_b2'], load_golden('taco_fwd_b2')
    model.r = info['r']
    model.train()
    before = model.get_step()
    out = [o.cpu().numpy() for o in model(torch.from_numpy(g['x']).cuda(), torch.from_numpy(g['m']).cuda())]
    model.eval()
    assert model.get_step() == before + 1
    check(info, g, out)


def test_cli_writes_the_persistent_launch_mel(tmp_path):
    """gen_tacotron end to end (synthetic weights, token input): the melgan branch saves the
    postnet output of Tacotron.generate under the reference's name."""
    from forwardtacotron_amd import gen_tacotron
    written = gen_tacotron.main(['--synthetic', '--input_tokens', '12,40,7', '--steps', '60',
                                 '--out', str(tmp_path), 'melgan'])
    assert [p.name for p in written] == ['1_taco_0k_melgan.mel']
    m = torch.load(written[0], weights_only=True)
    assert m.shape == (1, 80, 60) and torch.isfinite(m).all() and float(m.abs().mean()) > 0.1
