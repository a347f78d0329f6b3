"""Synthesising a list of sentences: the loop of ForwardTacotron.generate(x_i[None]) (what the
CLI does without --batch) against ForwardTacotron.generate_batch (the sentences in shared
launches, each one's result that of the sentence alone).

Workload: the token recipe of BASELINE config c3 (synthetic.synthetic_tokens(64, 200, seed=0,
min_len=50): 64 sentences of 50-200 tokens, fixed seed), synthetic weights, alpha = 1.  Six
sides, timed in the same run:

  loop      generate(x_i[None]) for every sentence, one after the other.  The rounds show
            generate() the same 64 shapes again and again, so it captures each one's phoneme
            phase as a graph and drops it again (phase_graph keeps 8): the cost of a caller
            that cycles through more shapes than the cache holds
  loop_eager  the same loop with the phase graph off (forward_tacotron.GRAPH = False): what
            the CLI's one-off sentence lengths get, since a shape seen once stays eager
  padded   generate() on the zero-padded (64, 200) batch — other results (the items see
            the padding and each other), shown for its cost only
  masked    generate_masked(x, x_len) on the same padded batch: the length-aware pass alone,
            its results left in the padded tensors
  batch     generate_batch(xs) as one chunk: that pass plus the host-side padding and the
            320 per-item copies into tensors of their own
  batch16   generate_batch(xs, max_batch=16)

After two warm-up passes of every side (weight packs, code loading, the loop's per-shape
graphs), `--rounds` rounds run the sides alternately; within a round a side runs `inner`
times back to back (loop: once — it is 64 calls already) between two device synchronises,
and its time is the host wall time over `inner`.  Per side: every round's ms, their min,
median and max (the spread), and valid mel frames (the frames the 64 sentences have when
synthesised alone) per second at the median.  The batch results are also compared with the
loop's on the spot (frame counts equal, max |mel_post| difference).

Prints one JSON line and writes it to profiles/gen_batch_bench.json.

    python tools/gen_batch_bench.py [--out profiles] [--name gen_batch_bench.json] [--rounds 7]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

ITEMS, T_MAX, T_MIN, SEED = 64, 200, 50, 0


def timed(fn, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3 / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--name', default='gen_batch_bench.json')
    ap.add_argument('--out', default=str(ROOT / 'profiles'))
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--inner', type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('gen_batch_bench needs a HIP device (no CPU fallback)')
    from forwardtacotron_amd.gen_forward import synthetic_tts_model
    from forwardtacotron_amd.synthetic import synthetic_tokens
    model, _ = synthetic_tts_model()
    model = model.to('cuda').eval()
    x = synthetic_tokens(ITEMS, T_MAX, seed=SEED, min_len=T_MIN)
    lengths = (x != 0).sum(1).tolist()
    xs = [torch.from_numpy(x[b, :L]).cuda() for b, L in enumerate(lengths)]
    xp = torch.from_numpy(x).cuda()
    lens_t = torch.tensor(lengths)
    from forwardtacotron_amd import forward_tacotron as ft

    def loop_eager():
        ft.GRAPH = False
        try:
            return [model.generate(s[None]) for s in xs]
        finally:
            ft.GRAPH = True

    sides = {
        'loop': (lambda: [model.generate(s[None]) for s in xs], 1),
        'loop_eager': (loop_eager, 1),
        'padded': (lambda: model.generate(xp), a.inner),
        'masked': (lambda: model.generate_masked(xp, lens_t), a.inner),
        'batch': (lambda: model.generate_batch(xs), a.inner),
        'batch16': (lambda: model.generate_batch(xs, max_batch=16), a.inner),
    }
    for _ in range(2):
        for fn, _n in sides.values():
            fn()
    torch.cuda.synchronize()
    # results must not change: the batch against the loop, item by item (the loop's dictionaries
    # alias buffers the next call reuses, so each is compared right after its call)
    outs = model.generate_batch(xs)
    frames, worst = [], 0.0
    for s, o in zip(xs, outs):
        ref = model.generate(s[None])['mel_post']
        assert ref.shape == o['mel_post'].shape, (ref.shape, o['mel_post'].shape)
        frames.append(int(ref.shape[2]))
        worst = max(worst, float((ref - o['mel_post']).abs().max()))
    valid = int(sum(frames))
    runs = {k: [] for k in sides}
    for _ in range(max(1, a.rounds)):
        for name, (fn, inner) in sides.items():
            runs[name].append(timed(fn, inner)[1])
    row = {
        'workload': f'{ITEMS} sentences of {min(lengths)}-{max(lengths)} tokens '
                    f'(synthetic_tokens({ITEMS}, {T_MAX}, seed={SEED}, min_len={T_MIN})), synthetic '
                    'weights, alpha 1.0',
        'device': torch.cuda.get_device_name(0), 'rounds': a.rounds, 'inner': a.inner,
        'tokens': int(sum(lengths)), 'valid_frames': valid,
        'padded_frames': int(ITEMS * model.generate(xp)['mel'].shape[2]),
        'batch_vs_loop_max_abs_mel_post': worst,
    }
    for name, ms in runs.items():
        med = statistics.median(ms)
        row[name] = {'runs_ms': ms, 'min_ms': min(ms), 'median_ms': med, 'max_ms': max(ms),
                     'valid_frames_per_s': valid / (med * 1e-3)}
    best_loop = min(row['loop']['median_ms'], row['loop_eager']['median_ms'])
    row['speedup_batch_over_loop'] = best_loop / row['batch']['median_ms']
    row['speedup_batch16_over_loop'] = best_loop / row['batch16']['median_ms']
    row['batch_over_padded'] = row['batch']['median_ms'] / row['padded']['median_ms']
    row['masked_over_padded'] = row['masked']['median_ms'] / row['padded']['median_ms']
    line = json.dumps(row)
    print(line)
    Path(a.out).mkdir(parents=True, exist_ok=True)
    (Path(a.out) / a.name).write_text(line + '\n')
    # required: the batch beats the loop in valid frames per second
    for loop in ('loop', 'loop_eager'):
        assert row['batch']['valid_frames_per_s'] > row[loop]['valid_frames_per_s']
        assert row['batch16']['valid_frames_per_s'] > row[loop]['valid_frames_per_s']


if __name__ == '__main__':
    main()
