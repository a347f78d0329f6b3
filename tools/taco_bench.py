"""Tacotron generation timing: B = 1, T = 120 synthetic tokens, 800 frames, stop disabled
(stop_threshold = -1e9), r in {1, 2}.  Encoder, decoder launch and postnet are timed with
events; the torch-CPU restatement (tests/taco_torch_cpu.py) runs on 16 threads in the same
process as the CPU figure.  Prints one JSON line per r and writes it to
profiles/taco_bench_r{r}.json.

    python tools/taco_bench.py [--iters 5] [--no-cpu] [--out profiles]
"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / 'tests'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from forwardtacotron_amd.synthetic import default_config, load_synthetic, synthetic_tokens  # noqa: E402
from forwardtacotron_amd.tacotron import Tacotron  # noqa: E402

T, FRAMES = 120, 800


def gpu_leg(model, x, r, iters):
    model.r = r
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    rows = []
    for it in range(iters + 2):
        e = [ev() for _ in range(4)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e[0].record()
        enc, enc_proj = model._encode(x)
        e[1].record()
        mel, attn, n = model.decoder.launch(enc, enc_proj, r, FRAMES, -1e9)
        e[2].record()
        steps = int(n.item())
        linear = model._post(mel)
        e[3].record()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        assert steps == (FRAMES + r - 1) // r and torch.isfinite(linear).all()
        if it >= 2:  # two warm-up utterances (weight packing, allocator)
            rows.append([e[i].elapsed_time(e[i + 1]) for i in range(3)] + [wall])
    enc_ms, dec_ms, post_ms, wall_ms = np.median(np.asarray(rows), 0)
    return {'encoder_ms': float(enc_ms), 'decoder_ms': float(dec_ms), 'postnet_ms': float(post_ms),
            'ms_per_utterance': float(wall_ms), 'decoder_steps': steps,
            'us_per_decoder_step': float(dec_ms * 1e3 / steps)}


def cpu_leg(model, x, r):
    from taco_torch_cpu import generate, to_torch
    torch.set_num_threads(16)
    sd = to_torch({k: v.detach().cpu() for k, v in model.state_dict().items()})
    with torch.no_grad():
        generate(sd, x.cpu(), 40, r, -1e9)  # warm-up
        t0 = time.perf_counter()
        mel, _, attn = generate(sd, x.cpu(), FRAMES, r, -1e9)
        dt = time.perf_counter() - t0
    return {'cpu_threads': 16, 'cpu_ms_per_utterance': dt * 1e3,
            'cpu_us_per_decoder_step_all_in': dt * 1e6 / attn.shape[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--no-cpu', action='store_true')
    ap.add_argument('--out', default=str(ROOT / 'profiles'))
    a = ap.parse_args()
    model = load_synthetic(Tacotron.from_config(default_config()), 0, 'tacotron').cuda().eval()
    model.stop_threshold = model.stop_threshold.new_tensor(-1e9)
    x = torch.from_numpy(synthetic_tokens(1, T, seed=5)).cuda()
    for r in (1, 2):
        row = {'workload': f'tacotron generate B=1 T={T} frames={FRAMES} r={r} stop disabled',
               'device': torch.cuda.get_device_name(0)}
        row.update(gpu_leg(model, x, r, a.iters))
        if not a.no_cpu:
            row.update(cpu_leg(model, x, r))
            row['speedup_vs_cpu'] = row['cpu_ms_per_utterance'] / row['ms_per_utterance']
        line = json.dumps(row)
        print(line)
        Path(a.out).mkdir(parents=True, exist_ok=True)
        (Path(a.out) / f'taco_bench_r{r}.json').write_text(line + '\n')


if __name__ == '__main__':
    main()
