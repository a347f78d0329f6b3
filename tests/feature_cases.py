"""Inputs and a plain float64 restatement for the phoneme pitch / energy tests
(tests/test_feature_cases.py, tests/test_gpu_features.py, tests/golden/make_goldens_features.py).

Every input is regenerated from a fixed seed; tests/golden/goldens_features.npz keeps a sha256
of each case's input bytes next to what the reference computed from it, and a mismatch fails.

A case is one utterance: `mel` (n_mels, rows) fp32 log-mel, N(-4, 2), whose frames from
`mel_len` on are NaN; `dur` [T] int32 whose first `x_len` entries sum to mel_len and whose later
entries are non-zero decoys; `pitch` [P] fp32, 60-560 Hz with about 30 % zeros, whose entries
from `pitch_len` on are 50 Hz decoys (inside the kept range, outside the data's).  The
reference sees dur[:x_len], mel[:, :mel_len] and pitch[:pitch_len] as its three files.

The restatement (`features`, `normalize`) is the specification of include/ftmi.h in loops; its
`defect` argument plants one named mistake.
"""
import hashlib

import numpy as np

PITCH_MAX = 400.0  # exactly representable in fp32
PAD_FRAMES, PAD_TOKENS, PAD_PITCH = 3, 2, 4
CHUNK = 2048       # frames per LDS pass of the kernel (csrc/align.hip PF_CHUNK)
DEFECTS = ('all_tokens', 'le_max', 'pitch_by_frames', 'ignore_pitch_len', 'read_pad_frames')


# ---- inputs ---------------------------------------------------------------------------------

def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def split(total, parts, seed, zero_share=0.15):
    """`parts` non-negative durations that sum to `total`, some of them 0."""
    g = _rng(seed)
    w = g.random(parts) + 0.05
    w[g.random(parts) < zero_share] = 0.0
    if not w.any():
        w[0] = 1.0
    d = np.floor(w / w.sum() * total).astype(np.int64)
    live = np.flatnonzero(w)
    for k in range(int(total - d.sum())):
        d[live[k % len(live)]] += 1
    assert d.sum() == total and (d >= 0).all()
    return d.tolist()


def make(name, dur, seed, n_mels=80, T=None, mel_len=None, pitch_len=None, pitch=None, ld_bin=None):
    """dur: the first x_len durations.  mel_len: sum(dur) unless the case says otherwise (never:
    the reference asserts it).  pitch: {frame: value} overrides of the generated series."""
    g = _rng(seed)
    x_len = len(dur)
    L = int(sum(dur)) if mel_len is None else mel_len
    T = x_len + PAD_TOKENS if T is None else T
    PL = L if pitch_len is None else pitch_len
    rows, P = L + PAD_FRAMES, max(PL, L) + PAD_PITCH
    mel = np.full((n_mels, rows), np.nan, np.float32)
    mel[:, :L] = g.normal(-4.0, 2.0, (n_mels, L)).astype(np.float32)
    d = np.full(T, 2, np.int32)
    d[:x_len] = dur
    p = g.uniform(60.0, 560.0, P).astype(np.float32)
    p[g.random(P) < 0.3] = 0.0
    for t, v in (pitch or {}).items():
        p[t] = v
    p[PL:] = 50.0
    c = {'name': name, 'mel': mel, 'mel_len': L, 'dur': d, 'x_len': x_len, 'pitch': p, 'pitch_len': PL}
    if ld_bin:
        c['ld_bin'] = ld_bin
    return c


def feature_cases():
    """name -> case.  The smallest shapes at which each mechanism can break."""
    below = float(np.nextafter(np.float32(PITCH_MAX), np.float32(0.0)))
    cs = [
        make('t1', [1], 1, T=1),
        make('zero_runs', [0, 0, 3, 0, 0, 0, 2, 1, 0, 4, 0, 0], 2),
        make('tokens_beyond_frames', [1, 0, 0, 1], 3, T=4, pitch={0: 120.0, 1: 180.0}),
        make('x_len_decoys', [2, 3, 0, 4, 1, 2], 4, T=9),
        make('strided', [3, 1, 4, 1, 5, 9, 2, 6], 5, n_mels=13, ld_bin=47),
        make('pitch_cut_inside', [4, 4, 4, 4], 6, pitch_len=10,
             pitch={8: 100.0, 9: 200.0, 10: 300.0, 11: 390.0}),
        make('pitch_cut_before', [4, 4, 4, 4], 7, pitch_len=12),
        make('pitch_longer', [5, 2, 6], 8, pitch_len=20),
        make('unvoiced_token', [3, 4, 3], 9, pitch={3: 0.0, 4: 0.0, 5: 0.0, 6: 0.0}),
        make('above_max_token', [3, 4, 3], 10, pitch={3: 400.0, 4: 401.0, 5: 480.0, 6: 559.0}),
        make('at_max', [2, 2, 3], 11, pitch={0: PITCH_MAX, 1: 100.0, 2: below, 3: 100.0}),
        make('t64', split(150, 64, 12), 12, T=64),
        make('t65', split(150, 65, 13), 13, T=65),
        make('t512', split(700, 510, 14), 14, n_mels=13, T=512),
        make('long_token', [3, 1300, 2], 15, n_mels=13),
        make('mels13', split(90, 17, 16), 16, n_mels=13),
    ]
    for k, L in enumerate((CHUNK - 1, CHUNK, CHUNK + 1)):
        cs.append(make(f'frames_{L}', split(L, 40, 20 + k), 20 + k, n_mels=13))
    return {c['name']: c for c in cs}


BATCH_ITEMS = ('zero_runs', 't1', 'x_len_decoys', 'pitch_cut_inside', 'at_max')  # n_mels 80 each


def batch_case(cases):
    """Five items padded into one batch: (mel (5, 80, rows), mel_len, dur (5, T), x_len,
    pitch (5, P), pitch_len), the padding as in the single cases (NaN frames, decoy durations,
    50 Hz pitch).  Item k is the single case BATCH_ITEMS[k]."""
    cs = [cases[n] for n in BATCH_ITEMS]
    rows = max(c['mel'].shape[1] for c in cs)
    T = max(len(c['dur']) for c in cs)
    P = max(len(c['pitch']) for c in cs)
    mel = np.full((len(cs), 80, rows), np.nan, np.float32)
    dur = np.full((len(cs), T), 2, np.int32)
    pitch = np.full((len(cs), P), 50.0, np.float32)
    for k, c in enumerate(cs):
        mel[k, :, :c['mel'].shape[1]] = c['mel']
        dur[k, :len(c['dur'])] = c['dur']
        pitch[k, :len(c['pitch'])] = c['pitch']
    return {'mel': mel, 'mel_len': [c['mel_len'] for c in cs], 'dur': dur,
            'x_len': [c['x_len'] for c in cs], 'pitch': pitch,
            'pitch_len': [c['pitch_len'] for c in cs]}


def strided(case):
    """The case's mel in a buffer with bin stride ld_bin (NaN in the gap)."""
    m = case['mel']
    buf = np.full((m.shape[0], case.get('ld_bin', m.shape[1])), np.nan, np.float32)
    buf[:, :m.shape[1]] = m
    return buf


def sha(case):
    h = hashlib.sha256()
    for k in ('mel', 'dur', 'pitch'):
        h.update(np.ascontiguousarray(case[k]).tobytes())
    h.update(repr((case['mel_len'], case['x_len'], case['pitch_len'])).encode())
    return h.hexdigest()


# ---- the restatement ---------------------------------------------------------------------

def features(mel, mel_len, dur, x_len, pitch, pitch_len, pitch_max_freq=PITCH_MAX, defect=None):
    """-> (pitch_char, energy_char), float64 [T]: the means before their one fp32 rounding."""
    n_mels, rows = mel.shape
    T = len(dur)
    L = rows if defect == 'read_pad_frames' else mel_len
    C = T if defect == 'read_pad_frames' else x_len
    PL = len(pitch) if defect == 'ignore_pitch_len' else pitch_len
    fmax = np.float32(pitch_max_freq)
    s = np.zeros(L)
    for k in range(n_mels):  # k ascending; one frame per lane
        e = np.exp(mel[k, :L].astype(np.float64))
        s = s + e * e
    energy = np.sqrt(s)
    cum = [0]
    for i in range(C):
        cum.append(cum[-1] + max(int(dur[i]), 0))
    pitch_char, energy_char = np.zeros(T), np.zeros(T)
    for i in range(C if defect == 'all_tokens' else min(C, mel_len)):
        a, b = min(cum[i], L), min(cum[i + 1], L)
        es = ps = 0.0
        pc = 0
        for t in range(a, b):
            es += float(energy[t])
            if t < PL:
                v = np.float32(pitch[t])
                if v != np.float32(0.0) and (v <= fmax if defect == 'le_max' else v < fmax):
                    ps += float(v)
                    pc += 1
        if b > a:
            energy_char[i] = es / (b - a)
        if defect == 'pitch_by_frames':
            pc = b - a if pc else 0
        if pc:
            pitch_char[i] = ps / pc
    return pitch_char, energy_char


def run(case, defect=None):
    return features(case['mel'], case['mel_len'], case['dur'], case['x_len'], case['pitch'],
                    case['pitch_len'], PITCH_MAX, defect)


def moments(values):
    """values: float64 arrays -> (count, mean, population std) of their non-zero entries."""
    nz = np.concatenate([np.asarray(v, np.float64).ravel() for v in values])
    nz = nz[nz != 0.0]
    mean = nz.sum() / len(nz)
    return len(nz), float(mean), float(np.sqrt(((nz - mean) ** 2).sum() / len(nz)))


def normalize(values):
    """-> ([normalised float64 arrays], mean, std): (v - mean) / std where v != 0."""
    _, mean, std = moments(values)
    return [np.where(v != 0.0, (v - mean) / std, 0.0) for v in values], mean, std
