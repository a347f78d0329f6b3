"""The torch-CPU restatement of the Tacotron path (tests/taco_torch_cpu.py) against the
reference goldens (tests/golden/taco_*.npz): every case within max(1e-4 | 1e-5, 10 drift64),
drift64 = the reference's own fp32-vs-fp64 difference recorded with the golden."""
import json

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden
from taco_torch_cpu import forward, generate, to_torch

META = json.loads((GOLDEN / 'goldens_tacotron.json').read_text())
CASES = sorted(META['cases'])


def taco_sd():
    from forwardtacotron_amd.synthetic import synthetic_array
    keys = json.loads((GOLDEN / 'tacotron_state_dict_keys.json').read_text())
    return {k: synthetic_array(k, shape, dt, 0, 'tacotron') for k, shape, dt in keys}


@pytest.fixture(scope='module')
def sd():
    return to_torch(taco_sd())


def bounds(info):
    d = info['drift64']
    return (max(1e-4, 10 * d['mel']), max(1e-4, 10 * d['linear']), max(1e-5, 10 * d['attn']))


def run_case(sd, info, g):
    x = torch.from_numpy(g['x'])
    with torch.no_grad():
        if info['mode'] == 'generate':
            out = generate(sd, x, info['steps'], info['r'], info['stop_threshold'])
        else:
            out = forward(sd, x, torch.from_numpy(g['m']), info['r'])
    return [o.numpy() for o in out]


@pytest.mark.parametrize('name', CASES)
def test_restatement_matches_golden(sd, name):
    info, g = META['cases'][name], load_golden(f'taco_{name}')
    mel, lin, attn = run_case(sd, info, g)
    assert mel.shape == g['mel'].shape and attn.shape == g['attn'].shape  # the stop step too
    bm, bl, ba = bounds(info)
    assert np.abs(mel - g['mel']).max() <= bm
    assert np.abs(lin - g['linear']).max() <= bl
    assert np.abs(attn - g['attn']).max() <= ba


def test_recipe_conditions_recorded():
    """The goldens script asserted the recipe's conditions on the reference; the recorded
    figures are the ones the synthetic module documents."""
    from forwardtacotron_amd import synthetic
    c = META['cases']
    for st in (c['gen_t70'], META['recipe_t45_200']):
        assert st['peak'] >= 0.3 and st['visited'] >= 4 and 1 <= st['mel_abs'] <= 10
    assert c['gen_t70']['decided'] >= 0.8 and c['fwd_b3']['decided'] >= 0.8
    assert c['stop_value']['frames'] > 20 and c['stop_value']['margin'] >= 1e-2
    assert [c[f'stop_r{r}']['frames'] for r in (1, 2, 5)] == [12, 14, 20]
    assert synthetic.TACO_MEASURED['peak'] == (round(c['gen_t70']['peak'], 3),
                                               round(META['recipe_t45_200']['peak'], 3))
