"""Inputs and a plain float64 restatement for the validation-loss tests (tests/test_eval_cases.py,
tests/test_gpu_eval.py, tests/golden/make_goldens_eval.py).

Every input is regenerated from a fixed PCG64 seed; tests/golden/goldens_eval.npz keeps a sha256
of each case's input bytes next to what the reference computed from it, and a mismatch fails.

The restatement (`masked_l1`, `l1`, `cross_entropy`, `mol`) is the specification of
include/ftmi.h in numpy float64.  `mol` also returns, per (sample, component) pair, which of
the four branches was taken and the float64 cdf_delta, for the conditions that
tests/test_eval_cases.py asserts on the case set itself.
"""
import hashlib

import numpy as np


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def sha(case) -> str:
    h = hashlib.sha256()
    for k in sorted(case):
        v = case[k]
        if isinstance(v, np.ndarray):
            h.update(k.encode() + b'\0' + str(v.dtype).encode() + str(v.shape).encode())
            h.update(np.ascontiguousarray(v).tobytes())
        else:
            h.update(f'{k}={v!r}'.encode())
        h.update(b'\0')
    return h.hexdigest()


# ---- L1 -------------------------------------------------------------------------------------

def _l1_case(seed, shape, lens, wide=False, pad=None):
    """x, target fp32 (B, C, L).  wide: magnitudes 10^U(-3, 3) with random signs.  pad: the value
    that both tensors hold at the frames t >= lens[b] (None: ordinary values)."""
    g = _rng(seed)
    if wide:
        x = (10.0 ** g.uniform(-3, 3, shape) * g.choice([-1.0, 1.0], shape)).astype(np.float32)
        t = (10.0 ** g.uniform(-3, 3, shape) * g.choice([-1.0, 1.0], shape)).astype(np.float32)
    else:
        x = g.normal(-4.0, 2.0, shape).astype(np.float32)
        t = (x + g.normal(0.0, 0.5, shape)).astype(np.float32)
    c = {'x': x, 'target': t}
    if lens is not None:
        c['lens'] = np.asarray(lens, np.int64)
        if pad is not None:
            for b, n in enumerate(lens):
                x[b, :, max(n, 0):] = pad
                t[b, :, max(n, 0):] = pad
    return c


def l1_cases():
    """name -> {'x', 'target', optional 'lens'}."""
    return {
        'one': _l1_case(1, (1, 1, 1), [1]),
        'mel_3x80x37': _l1_case(2, (3, 80, 37), [37, 1, 20]),
        'c1_rows': _l1_case(3, (4, 1, 11), [11, 3, 7, 1]),
        'lens_zero': _l1_case(4, (3, 5, 9), [0, 9, 4]),
        'lens_over': _l1_case(5, (2, 7, 10), [25, 3]),
        'lens_all_zero': _l1_case(6, (2, 3, 5), [0, 0]),
        'big_wide': _l1_case(7, (8, 80, 1500), [1500, 1, 0, 777, 1499, 64, 65, 2000], wide=True),
        'pad_1e30': _l1_case(8, (2, 4, 40), [33, 5], pad=np.float32(1e30)),
        'plain': _l1_case(9, (3, 80, 37), None),
        'plain_c1': _l1_case(10, (2, 1, 70), None),
    }


def nan_padding(case):
    """The device-only variant: NaN at every frame t >= lens[b] of both tensors."""
    x, t = case['x'].copy(), case['target'].copy()
    for b, n in enumerate(case['lens']):
        x[b, :, max(int(n), 0):] = np.nan
        t[b, :, max(int(n), 0):] = np.nan
    return {'x': x, 'target': t, 'lens': case['lens']}


def masked_l1(x, target, lens):
    B, C, L = x.shape
    total, count = 0.0, 0
    for b in range(B):
        n = min(max(int(lens[b]), 0), L)
        total += float(np.abs(x[b, :, :n].astype(np.float64) - target[b, :, :n].astype(np.float64)).sum())
        count += n
    return total / (C * count) if count else float('nan')


def l1(x, target):
    return float(np.abs(x.astype(np.float64) - target.astype(np.float64)).sum() / x.size)


def run_l1(c):
    return masked_l1(c['x'], c['target'], c['lens']) if 'lens' in c else l1(c['x'], c['target'])


# ---- cross-entropy --------------------------------------------------------------------------

def _ce_case(seed, rows, C, scale=1.0, pick=None, batch=None):
    g = _rng(seed)
    logits = (g.normal(0.0, 2.0, (rows, C)) * scale).astype(np.float32)
    if pick == 'argmax':
        target = logits.argmax(1).astype(np.int64)
    elif pick == 'argmin':
        target = logits.argmin(1).astype(np.int64)
    else:
        target = g.integers(0, C, rows).astype(np.int64)
    c = {'logits': logits, 'target': target}
    if batch:
        c['batch'] = batch  # logits are handed over as (B, C, L), target as (B, L)
    return c


def ce_cases():
    """name -> {'logits' (rows, C), 'target' (rows,), optional 'batch'}."""
    return {
        'c2_r1': _ce_case(21, 1, 2),
        'c30_r63': _ce_case(22, 63, 30),
        'c512_r65': _ce_case(23, 65, 512),
        'c513_r1400': _ce_case(24, 1400, 513, batch=2),
        'c1024_r65': _ce_case(25, 65, 1024),
        'c512_r1400': _ce_case(26, 1400, 512, batch=2),
        'scaled300': _ce_case(27, 63, 512, scale=300.0),
        'argmax': _ce_case(28, 65, 30, pick='argmax'),
        'argmin': _ce_case(29, 63, 513, pick='argmin'),
    }


def ce_rejected():
    """One label equal to C and one equal to -1."""
    c = _ce_case(30, 65, 30)
    c['target'][7], c['target'][40] = 30, -1
    return c


def cross_entropy(logits, target):
    x = logits.astype(np.float64)
    m = x.max(1)
    lse = m + np.log(np.exp(x - m[:, None]).sum(1))
    return float((lse - x[np.arange(len(x)), target]).mean())


# ---- discretized mixture of logistics -------------------------------------------------------

HI, LO = np.float32(0.999), np.float32(-0.999)


def _mol_case(seed, B, L, K, edge=False, num_classes=65536, log_scale_min=None, reduce=True):
    g = _rng(seed)
    logit = g.normal(0.0, 1.0, (B, L, K))
    mean = g.uniform(-1.2, 1.2, (B, L, K))
    y = g.uniform(-1.0, 1.0, (B, L))
    if edge:
        ls = g.uniform(-14.0, 1.0, (B, L, K))
        ls[0, 3, 0] = ls[B - 1, L - 2, K - 1] = -40.0  # below the clamp
        flat = y.reshape(-1)
        n = flat.size
        flat[n // 8:n // 8 + max(n // 80, 1)] = -1.0  # runs of the two clipping values
        flat[n // 2:n // 2 + max(n // 80, 1)] = 1.0
        flat = flat.astype(np.float32)
        tail = [HI, np.nextafter(HI, np.float32(2)), np.nextafter(HI, np.float32(0)),
                LO, np.nextafter(LO, np.float32(-2)), np.nextafter(LO, np.float32(0))]
        flat[n - 6:] = tail
        y = flat.reshape(B, L)
    else:
        ls = g.uniform(-7.0, -1.0, (B, L, K))
        clip = g.random((B, L))
        y = np.where(clip < 0.03, -1.0, np.where(clip > 0.97, 1.0, y))
    c = {'y_hat': np.concatenate([logit, mean, ls], -1).astype(np.float32),
         'y': y.astype(np.float32)[..., None], 'num_classes': int(num_classes), 'reduce': bool(reduce)}
    if log_scale_min is not None:
        c['log_scale_min'] = float(log_scale_min)
    return c


def mol_cases():
    """name -> {'y_hat' (B, L, 3 K), 'y' (B, L, 1), 'num_classes', 'reduce', optional
    'log_scale_min'}."""
    return {
        'typical_k1': _mol_case(41, 1, 65, 1),
        'typical_k10': _mol_case(42, 2, 150, 10),
        'typical_k11': _mol_case(43, 2, 129, 11),
        'edge_k10': _mol_case(44, 3, 257, 10, edge=True),
        'edge_k11': _mol_case(45, 1, 130, 11, edge=True),
        'classes256': _mol_case(46, 1, 100, 10, num_classes=256, log_scale_min=-7.0),
        'edge_min9': _mol_case(47, 2, 64, 10, edge=True, log_scale_min=-9.0),
        'per_sample_k10': _mol_case(48, 2, 70, 10, edge=True, reduce=False),
        'per_sample_k1': _mol_case(49, 1, 129, 1, reduce=False),
    }


def _softplus(v):
    with np.errstate(over='ignore'):
        return np.where(v > 20.0, v, np.log1p(np.exp(np.minimum(v, 20.0))))


def _sigmoid(v):
    with np.errstate(over='ignore'):
        return 1.0 / (1.0 + np.exp(-v))


def mol(y_hat, y, num_classes=65536, log_scale_min=None):
    """(values (B, L) float64, branch (B, L, K) in 0..3, cdf_delta (B, L, K)).  The values are
    -log_sum_exp(log_probs): the reduce=False result before its unsqueeze; their mean is the loss."""
    if log_scale_min is None:
        log_scale_min = float(np.log(1e-14))
    K = y_hat.shape[-1] // 3
    h = y_hat.astype(np.float64)
    logit, mean, ls = h[..., :K], h[..., K:2 * K], np.maximum(h[..., 2 * K:], log_scale_min)
    yf = np.broadcast_to(y.astype(np.float32), mean.shape)  # the tests on y are fp32 compares
    centered = yf.astype(np.float64) - mean
    inv = np.exp(-ls)
    half = 1.0 / (num_classes - 1)
    plus_in, min_in, mid_in = inv * (centered + half), inv * (centered - half), inv * centered
    log_cdf_plus = plus_in - _softplus(plus_in)
    log_one_minus_cdf_min = -_softplus(min_in)
    cdf_delta = _sigmoid(plus_in) - _sigmoid(min_in)
    log_pdf_mid = mid_in - ls - 2.0 * _softplus(mid_in)
    mid = log_pdf_mid - np.log((num_classes - 1) / 2)
    inner = np.where(cdf_delta > 1e-5, np.log(np.maximum(cdf_delta, 1e-12)), mid)
    branch = np.where(yf < LO, 0, np.where(yf > HI, 1, np.where(cdf_delta > 1e-5, 2, 3)))
    lp = np.where(yf < LO, log_cdf_plus, np.where(yf > HI, log_one_minus_cdf_min, inner))
    lm = logit.max(-1, keepdims=True)
    lp = lp + (logit - (lm + np.log(np.exp(logit - lm).sum(-1, keepdims=True))))
    pm = lp.max(-1)
    lse = pm + np.log(np.exp(lp - pm[..., None]).sum(-1))
    return -lse, branch, cdf_delta


def run_mol(c):
    """The loss of a case: a float for reduce=True, else the (B, L, 1) float64 values."""
    v, _, _ = mol(c['y_hat'], c['y'], c['num_classes'], c.get('log_scale_min'))
    return float(v.mean()) if c['reduce'] else v[..., None]
