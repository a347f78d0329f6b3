"""Alignment timing: Dijkstra durations, peak-count durations and attention scores per item
at (mel_len, x_len) = (800, 120) for B = 1 and B = 16 and at (1250, 512) for B = 1, events
around 50 launches after 5 warm-up launches, next to the teacher-forced Tacotron pass
model(x, m) at the same shape (synthetic weights, r = 1; median of 3 after one warm-up), whose
attention the extraction reads.  Prints one JSON line and writes it to
profiles/align_bench.json.

    python tools/align_bench.py [--no-model] [--no-check] [--out profiles] [--name align_bench.json]
    python tools/align_bench.py --cpu-reference <reference checkout>   # host only, no GPU:
        the reference's functions on this host's CPU, one item per call -> align_bench_cpu.json
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

import align_cases as ac  # noqa: E402

SHAPES = ((800, 120, 1), (800, 120, 16), (1250, 512, 1))
LAUNCHES, WARMUP = 50, 5


def inputs(R, C, B):
    """(B, R + 1, C) soft alignments (the collate's one padding frame), mel_len = R."""
    att = np.stack([np.concatenate([ac.soft(R, C, 0.5, 300 + b), np.full((1, C), 1.0 / C, np.float32)])
                    for b in range(B)])
    return att, [R] * B, [C] * B


def timed(fn):
    for _ in range(WARMUP):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(LAUNCHES):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / LAUNCHES  # us per launch


def gpu_leg(with_model, check=True):
    from forwardtacotron_amd import ops
    rows = []
    model = None
    if with_model:
        from forwardtacotron_amd.synthetic import default_config, load_synthetic, synthetic_tokens
        from forwardtacotron_amd.tacotron import Tacotron
        model = load_synthetic(Tacotron.from_config(default_config()), 0, 'tacotron').cuda().eval()
    for R, C, B in SHAPES:
        att_np, ml, xl = inputs(R, C, B)
        att = torch.from_numpy(att_np).cuda()
        mlt = torch.tensor(ml, dtype=torch.int32).cuda()
        xlt = torch.tensor(xl, dtype=torch.int32).cuda()
        dur, cost = ops.align_dijkstra(att, mlt, xlt, want_cost=True)
        assert not check or dur.sum(1).cpu().tolist() == ml
        if check and R * C <= 100000:  # the loop restatement is slow beyond
            want = ac.durations_dp(att_np[0], R, C)
            assert np.array_equal(dur[0].cpu().numpy(), want[0]) and float(cost[0]) == want[1]
        row = {'mel_len': R, 'x_len': C, 'B': B,
               'dijkstra_us_per_item': timed(lambda: ops.align_dijkstra(att, mlt, xlt)) / B,
               'count_us_per_item': timed(lambda: ops.align_count(att, mlt, xlt)) / B,
               'score_us_per_item': timed(lambda: ops.attention_score(att, mlt, 1)) / B}
        if model is not None:
            x = torch.from_numpy(synthetic_tokens(B, C, seed=7)).cuda()
            m = torch.randn(B, 80, R + 1, device='cuda') * 3.0 - 4.0
            ts = []
            with torch.no_grad():
                for it in range(4):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    model(x, m)
                    torch.cuda.synchronize()
                    ts.append((time.perf_counter() - t0) * 1e3)
            row['forward_ms_per_item'] = float(np.median(ts[1:])) / B
            row['dijkstra_share_of_forward'] = row['dijkstra_us_per_item'] * 1e-3 / row['forward_ms_per_item']
        rows.append(row)
    return {'workload': 'alignment extraction per item', 'device': torch.cuda.get_device_name(0),
            'launches': LAUNCHES, 'shapes': rows}


def cpu_leg(ref):
    sys.path.insert(0, ref)
    from utils.duration_extraction import extract_durations_per_count, extract_durations_with_dijkstra
    from utils.metrics import attention_score
    rows = []
    for R, C, B in SHAPES:
        if B != 1:
            continue
        att, ml, xl = inputs(R, C, 1)
        seq = np.zeros(C, np.int64)
        t = []
        for fn in (lambda: extract_durations_with_dijkstra(seq, att[0], R),
                   lambda: extract_durations_per_count(seq, att[0], R),
                   lambda: attention_score(torch.from_numpy(att), torch.tensor(ml), r=1)):
            fn()
            t0 = time.perf_counter()
            for _ in range(3):
                fn()
            t.append((time.perf_counter() - t0) / 3 * 1e6)
        rows.append({'mel_len': R, 'x_len': C, 'B': 1, 'dijkstra_us_per_item': t[0],
                     'count_us_per_item': t[1], 'score_us_per_item': t[2]})
    return {'workload': 'alignment extraction per item, reference functions on the host CPU',
            'torch_threads': torch.get_num_threads(), 'shapes': rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--no-model', action='store_true')
    ap.add_argument('--cpu-reference', default=None)
    ap.add_argument('--no-check', action='store_true',
                    help='skip the result checks (a timing-experiment library named by FTMI_LIB)')
    ap.add_argument('--name', default='align_bench.json')
    ap.add_argument('--out', default=str(ROOT / 'profiles'))
    a = ap.parse_args()
    row = cpu_leg(a.cpu_reference) if a.cpu_reference else gpu_leg(not a.no_model, not a.no_check)
    line = json.dumps(row)
    print(line)
    Path(a.out).mkdir(parents=True, exist_ok=True)
    name = 'align_bench_cpu.json' if a.cpu_reference else a.name
    (Path(a.out) / name).write_text(line + '\n')


if __name__ == '__main__':
    main()
