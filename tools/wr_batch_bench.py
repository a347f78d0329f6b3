"""Vocoding a list of utterances: one WaveRNN.generate call per utterance (each its own launch)
against one WaveRNN.generate_batch call (the folds of all utterances in shared launches of 32).

16 synthetic mels (N(0, 1) - 4) of 200-800 frames, evenly spread, in a shuffled order; the default
config (hop 256, 9 bits RAW, mu-law), synthetic weights, target 11000, overlap 550, the same
seed per utterance on both sides, in the same run.  After one warm-up call of each kind (weight
packing, code loading), each side runs `--repeats` times; a side's figure is its fastest run.

  total_ms          host wall time of the calls, synchronised (upsampling, cond GEMM, sample
                    loop, tail, device-to-host copies)
  loop_ms           device time of generate_samples / generate_samples_batch alone (events)
  us_per_step       one by one: per utterance, loop_ms / L at its fold count (one launch each);
                    packed: loop_ms / (launches * L), the average over its launches (all of 32
                    folds but the last)
  samples_per_s     wave samples returned / total time

Prints one JSON line and writes it to profiles/wr_batch_bench.json.

    python tools/wr_batch_bench.py [--out profiles] [--name wr_batch_bench.json] [--repeats 2]
"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

ITEMS, T_MIN, T_MAX = 16, 200, 800
TARGET, OVERLAP = 11000, 550


def mels():
    rng = np.random.Generator(np.random.PCG64(1600))
    lengths = np.linspace(T_MIN, T_MAX, ITEMS).round().astype(int)
    rng.shuffle(lengths)
    return [torch.from_numpy((rng.normal(0.0, 1.0, (1, 80, int(T))) - 4.0).astype(np.float32)) for T in lengths]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def device_ms(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--name', default='wr_batch_bench.json')
    ap.add_argument('--out', default=str(ROOT / 'profiles'))
    ap.add_argument('--repeats', type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('wr_batch_bench needs a HIP device (no CPU fallback)')
    from forwardtacotron_amd.gen_forward import synthetic_wavernn
    voc, cfg = synthetic_wavernn()
    voc = voc.to('cuda')
    mu_law = bool(cfg['dsp']['mu_law'])
    ms = [m.cuda() for m in mels()]
    seeds = [9000 + i for i in range(len(ms))]
    lengths = [m.size(-1) for m in ms]
    plan = voc.pack_plan(lengths, True, TARGET, OVERLAP)
    folds = plan.items[:, 1].tolist()
    L = plan.L
    short = sorted(range(len(ms)), key=lambda i: lengths[i])[:2]

    def one_by_one():
        return [voc.generate(m, True, TARGET, OVERLAP, mu_law, seed=s) for m, s in zip(ms, seeds)]

    def packed():
        return voc.generate_batch(ms, True, TARGET, OVERLAP, mu_law, seeds=seeds)

    voc.generate(ms[short[0]], True, TARGET, OVERLAP, mu_law, seed=1)
    voc.generate_batch([ms[i] for i in short], True, TARGET, OVERLAP, mu_law, seeds=[1, 2])
    runs = {'one_by_one': [], 'packed': []}
    waves = {}
    for _ in range(max(1, a.repeats)):
        for name, fn in (('one_by_one', one_by_one), ('packed', packed)):
            waves[name], t = timed(fn)
            runs[name].append(t)
    n_samples = int(sum(w.size for w in waves['packed']))
    assert [w.shape for w in waves['packed']] == [w.shape for w in waves['one_by_one']]
    assert all(w.shape == ((T - 1) * voc.hop_length,) for w, T in zip(waves['packed'], lengths))
    assert all(np.isfinite(w).all() for w in waves['packed'])
    # the sample loops alone
    loop_each = [device_ms(lambda m=m, s=s: voc.generate_samples(m, True, TARGET, OVERLAP, seed=s))
                 for m, s in zip(ms, seeds)]
    loop_packed = device_ms(lambda: voc.generate_samples_batch(ms, True, TARGET, OVERLAP, seeds=seeds))
    from forwardtacotron_amd import ops
    launches_each = [len(ops.wavernn_route(f)) for f in folds]
    t1, tp = min(runs['one_by_one']), min(runs['packed'])
    row = {
        'workload': f'{len(ms)} synthetic mels of {T_MIN}-{T_MAX} frames, default config (hop '
                    f'{voc.hop_length}, {voc.n_classes} classes), target {TARGET}, overlap {OVERLAP}',
        'device': torch.cuda.get_device_name(0), 'frames': lengths, 'folds': folds, 'L': L,
        'wave_samples': n_samples,
        'one_by_one': {'total_ms': t1, 'runs_ms': runs['one_by_one'], 'launches': int(sum(launches_each)),
                       'folds_per_launch': folds, 'loop_ms': loop_each,
                       'us_per_step': [t * 1e3 / (n * L) for t, n in zip(loop_each, launches_each)],
                       'samples_per_s': n_samples / (t1 * 1e-3)},
        'packed': {'total_ms': tp, 'runs_ms': runs['packed'], 'launches': len(plan.launches),
                   'folds_per_launch': [b for _, _, _, b in plan.launches], 'loop_ms': loop_packed,
                   'us_per_step': loop_packed * 1e3 / (len(plan.launches) * L),
                   'samples_per_s': n_samples / (tp * 1e-3)},
        'speedup_total': t1 / tp, 'speedup_loop': float(sum(loop_each)) / loop_packed,
    }
    line = json.dumps(row)
    print(line)
    Path(a.out).mkdir(parents=True, exist_ok=True)
    (Path(a.out) / a.name).write_text(line + '\n')


if __name__ == '__main__':
    main()
