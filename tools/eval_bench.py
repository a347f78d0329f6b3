"""Validation-loss timing: masked L1 at (64, 80, 1400), cross-entropy at (32 * 1375, 512) and
the mixture-of-logistics loss at (32 * 1375, 30), events around 50 launches after 5 warm-up
launches, each next to the teacher-forced pass that produces its input (synthetic weights;
median of 3 after one warm-up): ForwardTacotron.forward at B = 64, 200 tokens, 1400 frames, and
WaveRNN.forward in RAW and MOL mode at B = 32 and five hops of samples (1280 with the default
hop of 256; the reference trains on 5 * 275 = 1375).  The share of the forward pass is taken
with the loss timed on that pass's own output.  Prints one JSON line and writes it to
profiles/eval_bench.json.

    python tools/eval_bench.py [--no-model] [--no-check] [--out profiles] [--name eval_bench.json]
    python tools/eval_bench.py --cpu-reference <reference checkout>   # host only, no GPU: the
        reference's own loss functions on this host's CPU -> eval_bench_cpu.json
"""
import argparse
import json
import platform
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / 'tests'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import eval_cases as ec  # noqa: E402

L1_SHAPE, VOC_ROWS, RAW_C, MOL_C = (64, 80, 1400), 32 * 1375, 512, 30
LAUNCHES, WARMUP = 50, 5


def inputs():
    """numpy inputs at the three shapes: mel-like operands with lengths 700..1400, logits N(0, 2)
    with uniform labels, mixture parameters like the tests' typical case."""
    g = np.random.Generator(np.random.PCG64(500))
    x = g.normal(-4.0, 2.0, L1_SHAPE).astype(np.float32)
    t = (x + g.normal(0.0, 0.5, L1_SHAPE)).astype(np.float32)
    lens = g.integers(700, 1401, L1_SHAPE[0])
    logits = g.normal(0.0, 2.0, (VOC_ROWS, RAW_C)).astype(np.float32)
    labels = g.integers(0, RAW_C, VOC_ROWS)
    K = MOL_C // 3
    y_hat = np.concatenate([g.normal(0.0, 1.0, (VOC_ROWS, K)), g.uniform(-1.2, 1.2, (VOC_ROWS, K)),
                            g.uniform(-7.0, -1.0, (VOC_ROWS, K))], 1).astype(np.float32)
    y = g.uniform(-1.0, 1.0, VOC_ROWS).astype(np.float32)
    return x, t, lens, logits, labels, y_hat, y


def timed(fn):
    for _ in range(WARMUP):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(LAUNCHES):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / LAUNCHES  # us per call


def forward_ms(fn):
    """Median wall time of 3 calls after one warm-up; returns (ms, the last output)."""
    ts, out = [], None
    with torch.no_grad():
        for _ in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts[1:])), out


def tts_forward():
    from forwardtacotron_amd.forward_tacotron import ForwardTacotron
    from forwardtacotron_amd.synthetic import default_config, load_synthetic, synthetic_tokens
    B, _, F = L1_SHAPE
    T = 200
    model = load_synthetic(ForwardTacotron.from_config(default_config())).cuda().eval()
    g = np.random.Generator(np.random.PCG64(501))
    batch = {'x': torch.from_numpy(synthetic_tokens(B, T, seed=7, min_len=T)).cuda(),
             'mel': torch.from_numpy(g.normal(-4.0, 2.0, (B, 80, F)).astype(np.float32)).cuda(),
             'mel_len': torch.full((B,), F - 1).cuda(), 'x_len': torch.full((B,), T).cuda(),
             'dur': torch.full((B, T), float(F // T)).cuda(),
             'pitch': torch.from_numpy(g.normal(0, 1, (B, T)).astype(np.float32)).cuda(),
             'energy': torch.from_numpy(g.normal(0, 1, (B, T)).astype(np.float32)).cuda()}
    ms, pred = forward_ms(lambda: model(batch))
    return ms, pred, batch


def voc_forward(mode):
    from forwardtacotron_amd.synthetic import default_config, load_synthetic
    from forwardtacotron_amd.wavernn import WaveRNN
    cfg = default_config()
    cfg['vocoder']['model']['mode'] = mode
    model = load_synthetic(WaveRNN.from_config(cfg), kind='wavernn').cuda().eval()
    g = np.random.Generator(np.random.PCG64(502))
    B, L = 32, 5 * model.hop_length
    mel = torch.from_numpy(g.normal(-4.0, 2.0, (B, 80, 5 + 2 * model.pad)).astype(np.float32)).cuda()
    x = torch.from_numpy(g.uniform(-1, 1, (B, L)).astype(np.float32)).cuda()
    ms, y_hat = forward_ms(lambda: model(x, mel))
    if mode == 'RAW':
        y = torch.from_numpy(g.integers(0, model.n_classes, (B, L))).cuda()
    else:
        y = torch.from_numpy(g.uniform(-1, 1, (B, L)).astype(np.float32)).cuda()
    return ms, y_hat, y


def gpu_leg(with_model, check=True):
    from forwardtacotron_amd import ops
    x_np, t_np, lens_np, logits_np, labels_np, y_hat_np, y_np = inputs()
    x, t = torch.from_numpy(x_np).cuda(), torch.from_numpy(t_np).cuda()
    xt = x.transpose(1, 2).contiguous().transpose(1, 2)  # the layout of pred['mel']
    lens = torch.from_numpy(lens_np).int().cuda()
    logits, labels = torch.from_numpy(logits_np).cuda(), torch.from_numpy(labels_np).int().cuda()
    y_hat, y = torch.from_numpy(y_hat_np).cuda(), torch.from_numpy(y_np).cuda()
    lsm = float(np.log(1e-14))
    if check:
        eps = 2.0 ** -23
        for got, want in ((ops.l1_loss(xt, t, lens), ec.masked_l1(x_np, t_np, lens_np)),
                          (ops.cross_entropy(logits, labels)[0], ec.cross_entropy(logits_np, labels_np)),
                          (ops.mol_loss(y_hat, y, 65536, lsm)[0],
                           float(ec.mol(y_hat_np[None], y_np[None, :, None])[0].mean()))):
            assert abs(float(got) - want) <= eps * abs(want), (float(got), want)
    rows = {
        'masked_l1': {'shape': list(L1_SHAPE),
                      'loss_us': timed(lambda: ops.l1_loss(xt, t, lens)),
                      'loss_us_both_frame_major': timed(lambda: ops.l1_loss(x, t, lens)),
                      'bytes': 8.0 * x.numel() * float(lens_np.sum()) / (L1_SHAPE[0] * L1_SHAPE[2])},
        'cross_entropy': {'shape': [VOC_ROWS, RAW_C],
                          'loss_us': timed(lambda: ops.cross_entropy(logits, labels)),
                          'bytes': 4.0 * logits.numel()},
        'mol': {'shape': [VOC_ROWS, MOL_C], 'loss_us': timed(lambda: ops.mol_loss(y_hat, y, 65536, lsm)),
                'bytes': 4.0 * y_hat.numel()},
    }
    for r in rows.values():
        r['GB_per_s'] = r['bytes'] / r['loss_us'] * 1e-3
    if with_model:
        from forwardtacotron_amd import evaluate as ev
        ms, pred, batch = tts_forward()
        r = rows['masked_l1']
        r['forward'] = 'ForwardTacotron.forward B=64 T=200 frames=1400'
        r['forward_ms'] = ms
        # the four losses of one evaluate_forward step on that pass's output; mel counts twice
        r['loss_us_on_forward_output'] = timed(lambda: ev.masked_l1(pred['mel'], batch['mel'], batch['mel_len']))
        r['share_of_forward'] = 2 * r['loss_us_on_forward_output'] * 1e-3 / ms
        for mode, key in (('RAW', 'cross_entropy'), ('MOL', 'mol')):
            ms, out, tgt = voc_forward(mode)
            B, L, C = out.shape
            r = rows[key]
            r['forward'] = f'WaveRNN.forward {mode} B={B} L={L}'
            r['forward_ms'] = ms
            if mode == 'RAW':
                flat, lab = out.view(B * L, C), tgt.view(-1).int()
                r['loss_us_on_forward_output'] = timed(lambda: ops.cross_entropy(flat, lab))
            else:
                flat, smp = out.view(B * L, C), tgt.view(-1)
                r['loss_us_on_forward_output'] = timed(lambda: ops.mol_loss(flat, smp, 65536, lsm))
            r['share_of_forward'] = r['loss_us_on_forward_output'] * 1e-3 / ms
    return {'workload': 'validation losses', 'device': torch.cuda.get_device_name(0), 'launches': LAUNCHES,
            'losses': rows}


def cpu_leg(ref):
    sys.path.insert(0, ref)
    import torch.nn.functional as F
    from trainer.common import MaskedL1
    from utils.distribution import discretized_mix_logistic_loss
    x, t, lens, logits, labels, y_hat, y = (torch.from_numpy(v) for v in inputs())
    masked = MaskedL1()
    rows = {}
    with torch.no_grad():
        for key, fn in (('masked_l1', lambda: masked(x, t, lens)),
                        ('cross_entropy', lambda: F.cross_entropy(logits, labels)),
                        ('mol', lambda: discretized_mix_logistic_loss(y_hat[None], y[None, :, None]))):
            fn()
            t0 = time.perf_counter()
            for _ in range(3):
                fn()
            rows[key] = {'loss_us': (time.perf_counter() - t0) / 3 * 1e6}
    return {'workload': 'validation losses, reference functions on the host CPU (another machine than '
                        'the GPU figures: not a like-for-like comparison)',
            'host': platform.processor() or platform.machine(), 'torch_threads': torch.get_num_threads(),
            'losses': rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--no-model', action='store_true')
    ap.add_argument('--cpu-reference', default=None)
    ap.add_argument('--no-check', action='store_true',
                    help='skip the result checks (a timing-experiment library named by FTMI_LIB)')
    ap.add_argument('--name', default='eval_bench.json')
    ap.add_argument('--out', default=str(ROOT / 'profiles'))
    a = ap.parse_args()
    row = cpu_leg(a.cpu_reference) if a.cpu_reference else gpu_leg(not a.no_model, not a.no_check)
    line = json.dumps(row)
    print(line)
    Path(a.out).mkdir(parents=True, exist_ok=True)
    name = a.name.replace('.json', '_cpu.json') if a.cpu_reference else a.name
    (Path(a.out) / name).write_text(line + '\n')


if __name__ == '__main__':
    main()
