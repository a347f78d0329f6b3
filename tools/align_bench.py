"""Alignment timing: Dijkstra durations, peak-count durations and attention scores per item
at (mel_len, x_len) = (800, 120) for B = 1 and B = 16 and at (1250, 512) for B = 1, events
around 50 launches after 5 warm-up launches, next to the teacher-forced Tacotron pass
model(x, m) at the same shape (synthetic weights, r = 1; median of 3 after one warm-up), whose
attention the extraction reads.  Prints one JSON line and writes it to
profiles/align_bench.json.

--features times the step after it instead: phoneme-level pitch and energy
(ops.phoneme_features, one launch per batch) per item at the same shapes, with the durations
of the Dijkstra launch on the same attention, next to that launch and the teacher-forced pass,
plus the data set's moments and normalisation at 13,100 x 120 phoneme pitches
-> profiles/align_features_bench.json.

    python tools/align_bench.py [--features] [--no-model] [--no-check] [--out profiles] [--name align_bench.json]
    python tools/align_bench.py [--features] --cpu-reference <reference checkout>   # host only, no GPU:
        the reference's functions on this host's CPU, one item per call -> align_bench_cpu.json
        (--features: its extract_pitch_energy over a one-item data set -> align_features_bench_cpu.json)
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


def load_model():
    from forwardtacotron_amd.synthetic import default_config, load_synthetic
    from forwardtacotron_amd.tacotron import Tacotron
    return load_synthetic(Tacotron.from_config(default_config()), 0, 'tacotron').cuda().eval()


def forward_ms_per_item(model, R, C, B):
    """The teacher-forced pass model(x, m): median of 3 after one warm-up."""
    from forwardtacotron_amd.synthetic import synthetic_tokens
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
    return float(np.median(ts[1:])) / B


def feature_inputs(R, B, seed=400):
    """(mel (B, 80, R + 1) N(-4, 2), pitch (B, R): 60-560 Hz, 30 % zeros)."""
    g = np.random.Generator(np.random.PCG64(seed))
    mel = g.normal(-4.0, 2.0, (B, 80, R + 1)).astype(np.float32)
    pitch = g.uniform(60.0, 560.0, (B, R)).astype(np.float32)
    pitch[g.random((B, R)) < 0.3] = 0.0
    return mel, pitch


def features_leg(with_model, check=True):
    import feature_cases as fc
    from forwardtacotron_amd import ops
    model = load_model() if with_model else None
    rows = []
    for R, C, B in SHAPES:
        att_np, ml, xl = inputs(R, C, B)
        att = torch.from_numpy(att_np).cuda()
        mlt = torch.tensor(ml, dtype=torch.int32).cuda()
        xlt = torch.tensor(xl, dtype=torch.int32).cuda()
        mel_np, pitch_np = feature_inputs(R, B)
        mel, pitch = torch.from_numpy(mel_np).cuda(), torch.from_numpy(pitch_np).cuda()
        dur, _ = ops.align_dijkstra(att, mlt, xlt)
        pc, ec, dsum = ops.phoneme_features(mel, mlt, dur, xlt, pitch, mlt, 400.0)
        if check:
            assert dsum.cpu().tolist() == ml
            p64, e64 = fc.features(mel_np[0], R, dur[0].cpu().numpy(), C, pitch_np[0], R, 400.0)
            for got, want in ((pc[0], p64), (ec[0], e64)):
                got = got.cpu().numpy().astype(np.float64)
                assert np.array_equal(got == 0, want == 0)
                assert (np.abs(got - want) <= 2.0 ** -23 * np.abs(want)).all()
        row = {'mel_len': R, 'x_len': C, 'B': B,
               'features_us_per_item': timed(lambda: ops.phoneme_features(mel, mlt, dur, xlt, pitch, mlt, 400.0)) / B,
               'energy_only_us_per_item': timed(lambda: ops.phoneme_features(mel, mlt, dur, xlt)) / B,
               'dijkstra_us_per_item': timed(lambda: ops.align_dijkstra(att, mlt, xlt)) / B}
        row['features_share_of_dijkstra'] = row['features_us_per_item'] / row['dijkstra_us_per_item']
        if model is not None:
            row['forward_ms_per_item'] = forward_ms_per_item(model, R, C, B)
            row['features_share_of_forward'] = row['features_us_per_item'] * 1e-3 / row['forward_ms_per_item']
        rows.append(row)
    n = 13100 * 120  # an LJSpeech-sized data set's phoneme pitches
    g = np.random.Generator(np.random.PCG64(401))
    v = g.uniform(60.0, 400.0, n).astype(np.float32)
    v[g.random(n) < 0.3] = 0.0
    dev = torch.from_numpy(v).cuda()
    cnt, mean, std = ops.nonzero_moments(dev).tolist()
    assert not check or (cnt == np.count_nonzero(v) and abs(mean - v[v != 0].astype(np.float64).mean()) < 1e-9 * mean)
    norm = {'values': n, 'moments_us': timed(lambda: ops.nonzero_moments(dev)),
            'normalize_us': timed(lambda: ops.normalize_nonzero(dev, 0.0, 1.0))}  # mean 0, std 1: the values stay
    return {'workload': 'phoneme pitch / energy extraction per item', 'device': torch.cuda.get_device_name(0),
            'launches': LAUNCHES, 'shapes': rows, 'normalisation': norm}


def features_cpu_leg(ref):
    """The reference's extract_pitch_energy on this host's CPU over a data set of one item
    (its three np.load and two np.save calls included), median of 3 after one warm-up."""
    import tempfile

    import feature_cases as fc
    sys.path.insert(0, str(ROOT / 'tests' / 'golden'))
    import make_goldens_features as mg
    rows = []
    for R, C, B in SHAPES:
        if B != 1:
            continue
        mel, pitch = feature_inputs(R, 1)
        case = {'mel': mel[0], 'mel_len': R, 'dur': np.array(fc.split(R, C, 402), np.int32), 'x_len': C,
                'pitch': pitch[0], 'pitch_len': R}
        with tempfile.TemporaryDirectory() as tmp:
            paths = mg.write_dataset(Path(tmp), {'utt': case})
            fn, _ = mg.reference_functions(Path(ref), paths)
            ts = []
            for _ in range(4):
                t0 = time.perf_counter()
                fn(paths.phon_pitch, paths.phon_energy, 400.0)
                ts.append((time.perf_counter() - t0) * 1e6)
        rows.append({'mel_len': R, 'x_len': C, 'B': 1, 'features_us_per_item': float(np.median(ts[1:]))})
    return {'workload': 'phoneme pitch / energy extraction per item, reference function on the host CPU',
            'shapes': rows}


def gpu_leg(with_model, check=True):
    from forwardtacotron_amd import ops
    rows = []
    model = load_model() if with_model else None
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
            row['forward_ms_per_item'] = forward_ms_per_item(model, R, C, B)
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
    ap.add_argument('--features', action='store_true',
                    help='time the phoneme pitch / energy step -> align_features_bench.json')
    ap.add_argument('--cpu-reference', default=None)
    ap.add_argument('--no-check', action='store_true',
                    help='skip the result checks (a timing-experiment library named by FTMI_LIB)')
    ap.add_argument('--name', default='align_bench.json')
    ap.add_argument('--out', default=str(ROOT / 'profiles'))
    a = ap.parse_args()
    if a.features:
        row = features_cpu_leg(a.cpu_reference) if a.cpu_reference else features_leg(not a.no_model, not a.no_check)
    else:
        row = cpu_leg(a.cpu_reference) if a.cpu_reference else gpu_leg(not a.no_model, not a.no_check)
    line = json.dumps(row)
    print(line)
    Path(a.out).mkdir(parents=True, exist_ok=True)
    name = a.name
    if a.features and name == 'align_bench.json':
        name = 'align_features_bench.json'
    if a.cpu_reference:
        name = name.replace('.json', '_cpu.json')
    (Path(a.out) / name).write_text(line + '\n')


if __name__ == '__main__':
    main()
