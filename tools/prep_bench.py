"""Audio-preparation timing: 64 synthetic items of 6-10 s at 22,050 Hz (noise floor plus a ramped
tone burst, unequal lengths) through dsp.trim_bounds alone and through the whole
DSP.prepare_batch (trim, peak, scaled rows, labels, log-mel), device events around 20 calls after
3 warm-up calls, and in the same run the numpy restatement of the same steps
(tests/prep_cases.py, and oracle/dsp_oracle.py for the log-mel) on this host's CPU, one item
after the other.

Bytes: every sample counted as read once per kernel that reads it and every output as written
once (row length, the padding included: the kernels skip it, so this over-counts a little):
  trim_bounds    frame_power 4 B L read + 4 B F written; trim_bounds 4 B F read + 8 B written
  prepare_batch  the above + peak_abs 4 B L read + prepare 4 B L read, 4 B L + 8 B L written
                 + mel 4 B L read, 4 n_mels B F_mel written
The fraction of HBM bandwidth is those bytes over the measured time over 8 TB/s (spec peak).

Prints one JSON line and writes it to profiles/prep_bench.json.

    python tools/prep_bench.py [--out profiles] [--name prep_bench.json] [--cpu-items 8]
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

import prep_cases as pc  # noqa: E402

SR, ITEMS, CALLS, WARMUP = 22050, 64, 20, 3
HBM_PEAK = 8.0e12  # B/s, spec


def items():
    g = np.random.RandomState(700)
    out = []
    for i in range(ITEMS):
        n = int(g.randint(6 * SR, 10 * SR + 1))
        lo = int(g.randint(SR // 4, SR))
        hi = n - int(g.randint(SR // 4, SR))
        out.append(pc.item(n, 1000 + i, lo, hi, amp=float(g.uniform(0.2, 1.4)), ramp=2000))
    return out


def timed(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(CALLS):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / CALLS  # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--name', default='prep_bench.json')
    ap.add_argument('--out', default=str(ROOT / 'profiles'))
    ap.add_argument('--cpu-items', type=int, default=8,
                    help='items the host restatement is timed on (per-item figure)')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('prep_bench needs a HIP device (no CPU fallback)')
    from forwardtacotron_amd import dsp as D
    from forwardtacotron_amd.dsp import DSP
    cfg = json.loads((ROOT / 'tests' / 'golden' / 'dsp_config.json').read_text())
    dsp = DSP.from_config(cfg)
    sig = items()
    B, L = len(sig), max(len(v) for v in sig)
    rows = np.zeros((B, L), np.float32)
    for b, v in enumerate(sig):
        rows[b, :len(v)] = v
    y = torch.from_numpy(rows).cuda()
    lengths = torch.tensor([len(v) for v in sig], dtype=torch.int32).cuda()
    top_db, fl, hop = dsp.trim_silence_top_db, dsp.TRIM_FRAME_LENGTH, dsp.TRIM_HOP_LENGTH

    # results first: the device against the restatement on the items the host leg times
    p = dsp.prepare_batch(y, lengths)
    torch.cuda.synchronize()
    bounds = p.bounds.cpu().tolist()
    n_cpu = max(1, min(a.cpu_items, B))
    t_trim = t_prep = 0.0
    for b in range(n_cpu):
        t0 = time.perf_counter()
        se = pc.trim_bounds_np(sig[b], top_db, fl, hop, np.float32)
        t1 = time.perf_counter()
        s, e, peak, w, q = pc.prepare_np(sig[b], top_db, dsp.should_peak_norm, ('mu', dsp.bits))
        mel = _mel_np(dsp, w)
        t2 = time.perf_counter()
        t_trim += t1 - t0
        t_prep += t2 - t1
        assert tuple(bounds[b]) == tuple(se) == (s, e), (b, bounds[b], se, (s, e))
        n = e - s
        assert np.array_equal(p.wav[b, :n].cpu().numpy(), w)
        assert np.array_equal(p.quant[b, :n].cpu().numpy(), q)
        got = p.mel[b, :, :mel.shape[1]].cpu().numpy()
        assert np.abs(got - mel).max() < 1e-3, np.abs(got - mel).max()

    F = 1 + L // hop
    F_mel = 1 + L // dsp.hop_length
    bytes_trim = 4.0 * B * L + 4.0 * B * F + 4.0 * B * F + 8.0 * B
    bytes_prep = bytes_trim + 4.0 * B * L + (4.0 + 4.0 + 8.0) * B * L + 4.0 * B * L \
        + 4.0 * dsp.n_mels * B * F_mel
    us_power = timed(lambda: D.frame_power(y, lengths, fl, hop))
    us_trim = timed(lambda: D.trim_bounds(y, lengths, top_db, fl, hop))
    us_prep = timed(lambda: dsp.prepare_batch(y, lengths))
    audio_s = float(sum(len(v) for v in sig)) / SR
    row = {
        'workload': f'audio preparation, {B} items of 6-10 s at {SR} Hz (rows of {L} samples)',
        'device': torch.cuda.get_device_name(0), 'calls': CALLS, 'audio_seconds': audio_s,
        'frame_power': {'us_per_batch': us_power, 'us_per_item': us_power / B,
                        'bytes': 4.0 * B * L + 4.0 * B * F,
                        'hbm_fraction': (4.0 * B * L + 4.0 * B * F) / (us_power * 1e-6) / HBM_PEAK},
        'trim_bounds': {'us_per_batch': us_trim, 'us_per_item': us_trim / B, 'bytes': bytes_trim,
                        'GB_per_s': bytes_trim / us_trim * 1e-3,
                        'hbm_fraction': bytes_trim / (us_trim * 1e-6) / HBM_PEAK},
        'prepare_batch': {'us_per_batch': us_prep, 'us_per_item': us_prep / B, 'bytes': bytes_prep,
                          'GB_per_s': bytes_prep / us_prep * 1e-3,
                          'hbm_fraction': bytes_prep / (us_prep * 1e-6) / HBM_PEAK,
                          'audio_seconds_per_second': audio_s / (us_prep * 1e-6)},
        'host_numpy': {'items_timed': n_cpu, 'trim_bounds_us_per_item': t_trim / n_cpu * 1e6,
                       'prepare_us_per_item': t_prep / n_cpu * 1e6,  # its own trim included
                       'note': 'numpy restatement, one item after the other, one process'},
    }
    line = json.dumps(row)
    print(line)
    Path(a.out).mkdir(parents=True, exist_ok=True)
    (Path(a.out) / a.name).write_text(line + '\n')


def _mel_np(dsp, w):
    """The host's log-mel of one item: the reference's arithmetic as oracle/dsp_oracle.py has it."""
    from oracle import dsp_oracle
    return dsp_oracle.wav_to_mel(w, dsp.sample_rate, dsp.n_fft, dsp.hop_length, dsp.win_length,
                                 dsp.n_mels, dsp.fmin, dsp.fmax)


if __name__ == '__main__':
    main()
