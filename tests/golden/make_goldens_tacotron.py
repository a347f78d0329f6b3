"""Tacotron goldens from the reference model (models/tacotron.py).

Build container only (imports the reference, absent on the GPU box):

    FT_REFERENCE=<reference checkout> python tests/golden/make_goldens_tacotron.py

Weights: forwardtacotron_amd.synthetic recipe (seed 0, model='tacotron') loaded into the
reference `models.tacotron.Tacotron`; the fixtures keep only inputs / outputs (taco_*.npz),
the key / shape list (tacotron_state_dict_keys.json) and goldens_tacotron.json.

Every case also runs the reference in float64 and records drift64 = max |fp32 - fp64| for
mel, linear and attn: the feedback amplification of fp32-rounding-size perturbations, from
which tests/test_gpu_tacotron.py takes its bounds (max(1e-4 | 1e-5, 10 drift64)).

Asserted here, on the reference alone:
  - the recipe's gains (synthetic.TACO_ATTN_GAIN / TACO_MEL_GAIN): at T = 70 / 60 steps and
    T = 45, r = 2 / 200 steps the mean peak attention weight is >= 0.3, the argmax visits >= 4
    positions and mean |mel| lies in [1, 10];
  - the unconditional-stop frame counts 12 / 14 / 20 and attention rows 12 / 7 / 4 (r = 1, 2, 5);
  - the value-dependent stop: a threshold for which the reference stops at a step >= 20 and
    every step's largest frame value up to the stop is >= 1e-2 away from it;
  - cases gen_t70 and fwd_b3: the reference's top-two attention weights differ by more than
    ten times the attention bound on >= 80 % of the steps.
"""
import json
import os
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent
sys.path.insert(0, str(REPO))
if os.environ.get('FT_REFERENCE'):  # else the reference is expected on PYTHONPATH
    sys.path.insert(0, os.environ['FT_REFERENCE'])

from models.tacotron import Tacotron  # noqa: E402  (reference)

from forwardtacotron_amd.synthetic import default_config, load_synthetic, synthetic_tokens  # noqa: E402

MEL_BOUND, ATTN_BOUND = 1e-4, 1e-5


def make_model(dtype=torch.float32):
    torch.manual_seed(0)
    m = Tacotron.from_config(default_config())
    load_synthetic(m, 0, 'tacotron')
    return m.double() if dtype == torch.float64 else m


def run_generate(model, x, r, steps, thr):
    model.r = r
    model.stop_threshold = model.stop_threshold.new_tensor(thr)
    with torch.no_grad():
        mel, lin, attn = model.generate(torch.from_numpy(x), steps=steps)
    model.eval()
    return mel, lin, attn


def run_forward(model, x, m, r):
    model.r = r
    model.eval()
    with torch.no_grad():
        mel, lin, attn = model(torch.from_numpy(x), torch.from_numpy(m).to(model.post_proj.weight.dtype))
    return mel.numpy(), lin.numpy(), attn.numpy()


def both(fn):
    """fn(model) in fp32 and in fp64 -> (fp32 outputs, drift64)."""
    out32 = fn(make_model())
    torch.set_default_dtype(torch.float64)  # the reference allocates its zero states with it
    try:
        out64 = fn(make_model(torch.float64))
    finally:
        torch.set_default_dtype(torch.float32)
    assert all(a.shape == b.shape for a, b in zip(out32, out64)), 'fp64 run took another length'
    drift = {k: float(np.abs(a.astype(np.float64) - b).max())
             for k, a, b in zip(('mel', 'linear', 'attn'), out32, out64)}
    return [np.asarray(a, dtype=np.float32) for a in out32], drift


def attn_stats(attn, mel):
    a = attn.reshape(-1, attn.shape[-1])
    return {'peak': float(a.max(-1).mean()), 'visited': int(len(set(a.argmax(-1).tolist()))),
            'mel_abs': float(np.abs(mel).mean())}


def decided_fraction(attn, drift_attn):
    """Share of steps whose top-two weights differ by more than ten attention bounds."""
    bound = max(ATTN_BOUND, 10 * drift_attn)
    a = np.sort(attn.reshape(-1, attn.shape[-1]), -1)
    return float(((a[:, -1] - a[:, -2]) > 10 * bound).mean())


def main():
    meta = {'torch': torch.__version__, 'weights': 'synthetic seed 0, model tacotron', 'cases': {}}
    ref = make_model()
    keys = [[k, list(v.shape), str(v.dtype).replace('torch.', '')] for k, v in ref.state_dict().items()]
    (HERE / 'tacotron_state_dict_keys.json').write_text(json.dumps(keys, indent=0))
    have = {k: tuple(s) for k, s, _ in keys}
    assert have['decoder.mel_proj.weight'] == (1600, 512) and have['decoder.attn_net.conv.weight'] == (32, 2, 31)
    assert {'step', 'stop_threshold', 'decoder.r'} <= set(have)

    def save(name, arrays, info, drift):
        np.savez_compressed(HERE / f'taco_{name}.npz', **arrays)
        info['drift64'] = drift
        meta['cases'][name] = info
        print(name, info)

    # -- free-running generate (models/tacotron.py:272-331) ---------------------------------
    gen_cases = [('gen_t7', 7, 1, 12), ('gen_t45_r2', 45, 2, 40), ('gen_t70', 70, 1, 60),
                 ('gen_t45_r5', 45, 5, 100)]
    for i, (name, T, r, steps) in enumerate(gen_cases):
        x = synthetic_tokens(1, T, seed=100 + i)
        (mel, lin, attn), drift = both(lambda m: run_generate(m, x, r, steps, -11.0))
        info = {'mode': 'generate', 'T': T, 'r': r, 'steps': steps, 'stop_threshold': -11.0,
                'frames': int(mel.shape[1]), **attn_stats(attn, mel)}
        if name == 'gen_t70':
            info['decided'] = decided_fraction(attn, drift['attn'])
            assert info['decided'] >= 0.8, info
            assert info['peak'] >= 0.3 and info['visited'] >= 4 and 1 <= info['mel_abs'] <= 10, info
        save(name, {'x': x, 'mel': mel, 'linear': lin, 'attn': attn}, info, drift)

    # the recipe's second measuring point (not a fixture): T = 45, r = 2, 200 steps
    x = synthetic_tokens(1, 45, seed=101)
    mel, lin, attn = run_generate(make_model(), x, 2, 200, -11.0)
    st = attn_stats(attn, mel)
    meta['recipe_t45_200'] = st
    print('recipe T=45 r=2 200 steps', st)
    assert st['peak'] >= 0.3 and st['visited'] >= 4 and 1 <= st['mel_abs'] <= 10, st

    # -- unconditional stop: the first step with t > 10 ends the loop -----------------------
    x = synthetic_tokens(1, 20, seed=110)
    for r, frames, rows in ((1, 12, 12), (2, 14, 7), (5, 20, 4)):
        (mel, lin, attn), drift = both(lambda m: run_generate(m, x, r, 400, 1e9))
        assert mel.shape[1] == frames and attn.shape[0] == rows, (r, mel.shape, attn.shape)
        save(f'stop_r{r}', {'x': x, 'mel': mel, 'linear': lin, 'attn': attn},
             {'mode': 'generate', 'T': 20, 'r': r, 'steps': 400, 'stop_threshold': 1e9,
              'frames': frames}, drift)

    # -- value-dependent stop ------------------------------------------------------------
    # the first token seed whose trace of per-step maxima has a new minimum at a step >= 20
    # that clears every earlier step by the margin
    thr = stop = None
    for seed in range(120, 160):
        x = synthetic_tokens(1, 30, seed=seed)
        mel, _, _ = run_generate(make_model(), x, 1, 80, -1e9)
        tops = mel.max(0)  # r = 1: the step's largest value
        for s in range(20, len(tops)):
            # stop at s: tops[s] < thr; no earlier stop: tops[t] >= thr for 10 < t < s
            lo, hi = tops[s] + 1e-2, tops[11:s].min() - 1e-2
            if lo > hi:
                continue
            cand = 0.5 * (lo + hi)
            if np.abs(tops[:s + 1] - cand).min() >= 1e-2:
                thr, stop = float(np.float32(cand)), s
                break
        if thr is not None:
            break
    assert thr is not None, 'no threshold with a 1e-2 margin: change the token seed'
    (mel, lin, attn), drift = both(lambda m: run_generate(m, x, 1, 80, thr))
    assert mel.shape[1] == stop + 1 and stop >= 20, (mel.shape, stop)
    margin = float(np.abs(mel.max(0) - thr).min())
    assert margin >= 1e-2, margin
    save('stop_value', {'x': x, 'mel': mel, 'linear': lin, 'attn': attn},
         {'mode': 'generate', 'T': 30, 'r': 1, 'steps': 80, 'stop_threshold': thr, 'token_seed': seed,
          'frames': stop + 1, 'margin': margin}, drift)

    # -- teacher-forced forward (models/tacotron.py:216-270) --------------------------------
    rng = np.random.Generator(np.random.PCG64(77))
    for name, lens, r, F in (('fwd_b3', (45, 20, 7), 2, 37), ('fwd_b2', (33, 21), 1, 30)):
        x = synthetic_tokens(len(lens), max(lens), seed=130 + r, lengths=lens)
        m = (rng.normal(0.0, 3.0, (len(lens), 80, F)) - 4.0).astype(np.float32)
        (mel, lin, attn), drift = both(lambda mod: run_forward(mod, x, m, r))
        info = {'mode': 'forward', 'T': max(lens), 'lengths': list(lens), 'r': r, 'F': F,
                'frames': int(mel.shape[2]), **attn_stats(attn, mel)}
        if name == 'fwd_b3':
            assert mel.shape[2] == 38
            info['decided'] = decided_fraction(attn, drift['attn'])
            assert info['decided'] >= 0.8, info
        save(name, {'x': x, 'm': m, 'mel': mel, 'linear': lin, 'attn': attn}, info, drift)

    (HERE / 'goldens_tacotron.json').write_text(json.dumps(meta, indent=1))


if __name__ == '__main__':
    main()
