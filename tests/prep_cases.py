"""The silence trim and audio preparation restated in numpy (librosa 0.7.2 effects.trim as
utils/dsp.py:112-113 calls it, then preprocess.py:51-91 without the pitch track), and the case
table tests/test_prep_cases.py (CPU) and tests/test_gpu_prep.py (device) share.

Signals are deterministic: low-level uniform noise plus tone bursts with linear ramps, so a
frame's level is far from the threshold except on the ramps, and test_prep_cases.py asserts
that no frame of any case sits within 0.01 dB of it (then float32, float64 and the device must
give the same bounds).
"""
from collections import namedtuple
from functools import lru_cache

import numpy as np

PLANT = 1e3  # planted past each item's length: any read beyond the item moves every level


# --- the restatement ---------------------------------------------------------------------------

def frame_power_np(y, frame_length, hop, dtype=np.float64, pad_mode='reflect'):
    """power[f] = mean(frame ** 2) over the centred, padded frames; dtype float32 is what
    librosa computes (feature.rms: float32 mean over the frame axis, sqrt, and the caller
    squares again), float64 is the exact target."""
    y = np.asarray(y, dtype=dtype)
    yp = np.pad(y, frame_length // 2, mode=pad_mode)
    F = 1 + len(y) // hop
    idx = np.arange(frame_length)[:, None] + hop * np.arange(F)[None, :]
    frames = yp[idx]  # (frame_length, F), librosa util.frame's layout
    power = np.mean(np.abs(frames) ** 2, axis=0)
    if dtype == np.float32:
        power = np.sqrt(power) ** 2
        assert power.dtype == np.float32
    return power


def frame_db_np(power, ref=None):
    """librosa core.power_to_db(power, ref=np.max, amin=1e-10, top_db=None) in power's dtype."""
    amin = power.dtype.type(1e-10)
    ref = np.max(power) if ref is None else power.dtype.type(ref)
    return (10 * np.log10(np.maximum(amin, power)) - 10 * np.log10(np.maximum(amin, ref)))


def trim_bounds_np(y, top_db, frame_length=2048, hop=512, dtype=np.float64, pad_mode='reflect',
                   ref=None, clip_end=True, centre_start=False):
    """(start, end) of librosa effects.trim; the keyword defects exist for test_prep_cases."""
    L = len(y)
    db = frame_db_np(frame_power_np(y, frame_length, hop, dtype, pad_mode), ref)
    nz = np.flatnonzero(db > -top_db)
    if nz.size == 0:
        return 0, 0
    start = int(nz[0]) * hop + (frame_length // 2 if centre_start else 0)
    end = (int(nz[-1]) + 1) * hop
    return start, (min(L, end) if clip_end else end)


def labels_np(x, mode):
    """int64 labels of float32 samples x; mode: ('mu', bits) | ('raw', bits) | ('mol', 16)."""
    kind, bits = mode
    x = np.asarray(x, dtype=np.float32)
    if kind == 'mu':
        return mu_law_prefloor(x, bits)[1].astype(np.int64)
    m = 2 ** bits - 1
    v = (x + 1.) * m / 2
    assert v.dtype == np.float32
    return v.clip(0, m).astype(np.int64)


def mu_law_prefloor(x, bits):
    """(value before the floor, floor) of DSP.encode_mu_law(float64(x), 2 ** bits)."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    mu = 2 ** bits - 1
    fx = np.sign(x) * np.log(1 + mu * np.abs(x)) / np.log(1 + mu)
    pre = (fx + 1) / 2 * mu + 0.5
    return pre, np.floor(pre)


def prepare_np(y, top_db, peak_norm, mode, trim=True, frame_length=2048, hop=512):
    """One item through Preprocessor._convert_file's order: trim, peak rule, labels.  Returns
    (start, end, peak float32, prepared float32 samples, int64 labels).  An all-zero item is
    left unscaled (the reference divides by zero there)."""
    y = np.asarray(y, dtype=np.float32)
    s, e = trim_bounds_np(y, top_db, frame_length, hop) if trim else (0, len(y))
    w = y[s:e].copy()
    peak = np.abs(w).max() if w.size else np.float32(0)
    if (peak_norm or peak > 1.0) and peak > 0:
        w /= peak
    return s, e, np.float32(peak), w, labels_np(w, mode)


# --- deterministic signals ---------------------------------------------------------------------

def noise(n, seed, level):
    return (np.random.RandomState(seed).uniform(-1, 1, n) * level).astype(np.float32)


def burst(n, lo, hi, amp, ramp, period=37.0):
    """A tone over [lo, hi) with linear ramps of `ramp` samples at both ends, zero elsewhere."""
    t = np.arange(n)
    env = np.clip(np.minimum(t - lo, hi - 1 - t) / max(ramp, 1), 0, 1)
    return (amp * env * np.sin(2 * np.pi * t / period)).astype(np.float32)


def item(n, seed, lo, hi, amp=0.5, ramp=64, level=1e-4):
    return noise(n, seed, level) + burst(n, lo, hi, amp, ramp)


Case = namedtuple('Case', ['name', 'frame_length', 'hop', 'top_db', 'stride', 'items', 'named'])
# items: list of float32 arrays (unequal lengths); the device rows are (B, stride) with PLANT past
# each item.  named: indices of the items that must trim non-trivially (start > 0, end < L).


def _case(name, fl, hop, top_db, items, named=(), extra_stride=0):
    L = max(len(v) for v in items)
    return Case(name, fl, hop, top_db, L + extra_stride, [np.asarray(v, np.float32) for v in items],
                tuple(named))


@lru_cache(maxsize=None)
def cases():
    c = []
    # the reference's framing, one item per length of the list (700 is shorter than the pad)
    c.append(_case('ref-700', 2048, 512, 30, [item(700, 1, 520, 690, ramp=16)]))
    c.append(_case('ref-1025', 2048, 512, 30, [item(1025, 2, 530, 1000, ramp=16)]))
    c.append(_case('ref-2047', 2048, 512, 30, [item(2047, 3, 1100, 1500, ramp=32)]))
    c.append(_case('ref-12345', 2048, 512, 60, [item(12345, 4, 4000, 8000)], named=(0,)))
    c.append(_case('ref-30000', 2048, 512, 60, [item(30000, 5, 9000, 21000)], named=(0,),
                   extra_stride=77))
    # B = 3, unequal lengths, a stride beyond L: loud at sample 0; last frame non-silent with
    # L % hop != 0; an ordinary one
    c.append(_case('ref-b3', 2048, 512, 30,
                   [item(12345, 6, 0, 5000), item(9001, 7, 4000, 9001, ramp=8),
                    item(30000, 8, 7000, 20000)], named=(2,), extra_stride=5))
    # B = 5: a quiet item beside a loud one (the batch's level must not reach it), an all-zero
    # item, a peak above 1, a short one
    c.append(_case('ref-b5', 2048, 512, 30,
                   [item(30000, 9, 8000, 22000, amp=0.9),
                    item(30000, 10, 10000, 18000, amp=0.002, level=2e-6),
                    np.zeros(12345, np.float32),
                    item(12345, 11, 3000, 9000, amp=1.7),
                    item(1025, 12, 530, 1000, ramp=16)], named=(0, 1, 3), extra_stride=3))
    c.append(_case('ref-top10', 2048, 512, 10, [item(30000, 13, 9000, 21000, ramp=2000)],
                   named=(0,)))
    # a small frame whose hop divides it
    c.append(_case('small-b3', 256, 64, 30,
                   [item(2047, 14, 700, 1500, ramp=8), item(700, 15, 200, 450, ramp=8),
                    item(1025, 16, 0, 600, ramp=8)], named=(0, 1), extra_stride=9))
    c.append(_case('small-top60', 256, 64, 60, [item(12345, 17, 5000, 9000, ramp=16)], named=(0,)))
    c.append(_case('small-top10', 256, 64, 10, [item(2047, 18, 600, 1400, ramp=300)], named=(0,)))
    # a hop that does not divide the frame
    c.append(_case('odd-b3', 2048, 300, 30,
                   [item(12345, 19, 4000, 8000), item(30000, 20, 11000, 30000, ramp=8),
                    item(2047, 21, 1100, 1500, ramp=32)], named=(0,), extra_stride=1))
    c.append(_case('odd-top60', 2048, 300, 60, [item(30000, 22, 9000, 21000)], named=(0,)))
    c.append(_case('odd-700', 2048, 300, 10, [item(700, 23, 320, 690, ramp=16)]))
    # loud at sample 0 and decided by the padding: the reflected copy of the first 700 samples
    # lifts frame 0 to about -8.5 dB under the later burst; zero padding leaves it near -11.5 dB
    c.append(_case('ref-edge-start', 2048, 512, 10,
                   [noise(12345, 24, 1e-4) + burst(12345, 0, 700, 0.4545, 8)
                    + burst(12345, 5000, 9000, 1.0, 64)]))
    return tuple(c)


# planted defect -> (case, item) whose bounds it must change (tests/test_prep_cases.py)
DEFECTS = {
    'zero_pad': ('ref-edge-start', 0),
    'batch_reference': ('ref-b5', 1),
    'lengths_ignored': ('ref-b3', 1),
    'end_not_clipped': ('ref-b3', 1),
    'centre_start': ('ref-12345', 0),
}


def rows(case):
    """(B, stride) float32 rows with PLANT past each item's samples, and the int32 lengths
    (a PrepCase has no stride of its own: 7 past its longest item)."""
    stride = getattr(case, 'stride', None) or max(len(v) for v in case.items) + 7
    y = np.full((len(case.items), stride), PLANT, dtype=np.float32)
    for b, v in enumerate(case.items):
        y[b, :len(v)] = v
    return y, np.array([len(v) for v in case.items], dtype=np.int32)


@lru_cache(maxsize=None)
def expected_bounds(name, dtype_name):
    case = next(c for c in cases() if c.name == name)
    dt = np.float32 if dtype_name == 'float32' else np.float64
    return tuple(trim_bounds_np(v, case.top_db, case.frame_length, case.hop, dt) for v in case.items)


# --- preparation cases (the reference's 2048 / 512 trim; B = 3 rows of unequal length) ------------

PrepCase = namedtuple('PrepCase', ['name', 'peak_norm', 'mode', 'top_db', 'trim', 'items'])

LABEL_MODES = (('mu', 9), ('raw', 10), ('mol', 16))


def _plant_labels(v, lo):
    """-1, 0 and +1 inside the burst (they survive the trim; |x| <= 1 keeps the peak rule's
    verdict when the burst's own peak is 1 or more)."""
    v = v.copy()
    v[lo + 300:lo + 303] = (-1.0, 0.0, 1.0)
    return v


@lru_cache(maxsize=None)
def prep_cases():
    c = []
    loud = item(12345, 31, 3000, 9000, amp=1.7)    # peak above 1: scaled whatever peak_norm says
    unit = _plant_labels(item(9001, 32, 2500, 7000, amp=0.6), 2500)  # peak exactly 1
    quiet = item(12345, 33, 4000, 8000, amp=0.3)   # peak below 1: scaled only under peak_norm
    zero = np.zeros(3000, np.float32)              # left unscaled
    for mode in LABEL_MODES:
        c.append(PrepCase(f'{mode[0]}{mode[1]}-norm-off', False, mode, 60, True,
                          (loud, unit, quiet, zero)))
        c.append(PrepCase(f'{mode[0]}{mode[1]}-norm-on', True, mode, 30, True, (quiet, unit, zero)))
    c.append(PrepCase('mu9-no-trim', False, ('mu', 9), 60, False,
                      (item(9001, 34, 2500, 7000, amp=1.2), unit)))
    return tuple(c)
