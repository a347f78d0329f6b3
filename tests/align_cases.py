"""Inputs and a plain numpy restatement for the alignment tests (tests/test_align_cases.py,
tests/test_gpu_align.py, tests/golden/make_goldens_align.py).

Every input is regenerated from a fixed seed; tests/golden/goldens_align.npz keeps a sha256
of each input's bytes next to what the reference computed from it, and a mismatch fails.

Shapes are (mel_len, x_len).  An input has rows >= mel_len and T >= x_len; the padding rows
and columns hold decoys that change the result if they are read: padding columns carry the
largest values of their row, padding rows a sharp peak of their own.

The restatement (`durations_dp`, `durations_count`, `scores`) is the specification of
include/ftmi.h in loops; its `defect` argument plants one named mistake.
"""
import hashlib

import numpy as np

PAD_ROWS, PAD_COLS = 3, 2
DIAG, UP, LEFT = 0, 1, 2


# ---- inputs ---------------------------------------------------------------------------------

def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def soft(R, C, sharp, seed, floor=0.05):
    """A soft monotone alignment: softmax(-sharp (j - c_t)^2) around a jittered straight line,
    mixed with a random floor so that no two paths cost the same."""
    g = _rng(seed)
    c = np.linspace(0.0, C - 1.0, R) + g.normal(0.0, 0.4, R) if R > 1 else np.zeros(1)
    j = np.arange(C)[None, :]
    z = -sharp * (j - c[:, None]) ** 2
    p = np.exp(z - z.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    n = g.random((R, C)) + 0.05
    n /= n.sum(1, keepdims=True)
    return ((1.0 - floor) * p + floor * n).astype(np.float32)


def one_hot(peaks, C):
    a = np.zeros((len(peaks), C), np.float32)
    a[np.arange(len(peaks)), peaks] = 1.0
    return a


def ones_path(moves, seed):
    """att == 1.0 exactly on a staircase path ('D' diagonal, 'V' down, 'H' right; no V next to
    an H, so no other all-ones path exists), a random background in (0.05, 0.5) elsewhere."""
    i = j = 0
    cells = [(0, 0)]
    for m in moves:
        i, j = i + (m in 'DV'), j + (m in 'DH')
        cells.append((i, j))
    a = (_rng(seed).random((i + 1, j + 1)) * 0.45 + 0.05).astype(np.float32)
    for c in cells:
        a[c] = 1.0
    return a


def embed(core, rows=None, T=None, seed=0):
    """core in the top-left corner of a (rows, T) input full of decoys."""
    R, C = core.shape
    rows = R + PAD_ROWS if rows is None else rows
    T = C + PAD_COLS if T is None else T
    g = _rng(1000 + seed)
    a = (g.random((rows, T)) * 0.01).astype(np.float32)
    a[:, C:] = (0.97 + 0.02 * g.random((rows, T - C))).astype(np.float32)  # beats every real column
    a[R:, :C] = (g.random((rows - R, C)) * 0.01).astype(np.float32)
    for t in range(R, rows):  # padding rows peak at a column of their own
        a[t, (3 * t + 1) % C] = 0.96
    a[:R, :C] = core
    return a


def _case(name, core, tied=False, **kw):
    R, C = core.shape
    return {'name': name, 'att': embed(core, seed=len(name) + R + C, **kw), 'mel_len': R, 'x_len': C,
            'tied': tied}


def duration_cases():
    """name -> case; a case is {'att' (rows, T) fp32, 'mel_len', 'x_len', 'tied', 'ld_row'?}."""
    cs = []
    for k, (R, C) in enumerate([(1, 1), (1, 5), (7, 1), (3, 9)]):
        cs.append(_case(f'deg_{R}x{C}', soft(R, C, 0.5, 10 + k)))
    for tag, sharp in (('soft05', 0.5), ('soft5', 5.0)):
        for k, (R, C) in enumerate([(37, 11), (40, 63), (40, 64), (40, 65), (40, 129)]):
            cs.append(_case(f'{tag}_{R}x{C}', soft(R, C, sharp, 20 + k + int(10 * sharp))))
    c = _case('long_600x130', soft(600, 130, 0.5, 40), rows=640, T=132)
    c['ld_row'] = 136
    cs.append(c)
    cs.append(_case('wide_40x512', soft(40, 512, 0.5, 41), T=512))
    cs.append(_case('onehot_advance', one_hot(list(range(8)), 8)))
    cs.append(_case('onehot_stay', one_hot([t // 3 for t in range(12)], 4)))
    cs.append(_case('onehot_skip', one_hot([0, 1, 3, 3], 4), tied=True))
    cs.append(_case('ones_path', ones_path('DVDHDVVDHD', 42)))
    mono = soft(30, 12, 2.0, 43)
    cs.append(_case('nonmono_30x12', mono[_rng(44).permutation(30)]))
    # extract_durations_per_count semantics
    far = [2, 3, 14, 14, 14, 15, 15, 16, 17, 17, 18, 18]
    cs.append(_case('count_jump11', peaked(far, 20, 50)))
    cs.append(_case('count_jump10', peaked([2, 3, 13, 13, 14, 15, 15, 16, 17, 17, 18, 18], 20, 51)))
    cs.append(_case('count_beyond', peaked([0, 1, 1, 2, 3, 3, 4, 5], 6, 52)))
    tie = peaked([0, 1, 2, 4, 4, 5, 6, 7, 8], 9, 53)
    tie[3, 7] = tie[3, 4]  # an exact two-way tie in row 3: the first index (4) counts
    cs.append(_case('count_tie', tie))
    cs.append(_case('count_short', peaked([0, 0, 1, 2, 2, 3, 4, 5, 5, 5], 9, 54)))
    return {c['name']: c for c in cs}


def peaked(peaks, C, seed):
    """Rows with a clear peak (0.6) over a random background below 0.3."""
    a = (_rng(seed).random((len(peaks), C)) * 0.3).astype(np.float32)
    a[np.arange(len(peaks)), peaks] = 0.6
    return a


BATCH_ITEMS = ('soft05_37x11', 'deg_7x1', 'soft5_40x65', 'deg_3x9', 'nonmono_30x12')


def batch_case(cases):
    """Five items in one (5, rows, T) input; item 0 is the single-item case soft05_37x11."""
    cores = [cases[n]['att'][:cases[n]['mel_len'], :cases[n]['x_len']] for n in BATCH_ITEMS]
    rows = max(c.shape[0] for c in cores) + PAD_ROWS
    T = max(c.shape[1] for c in cores) + PAD_COLS
    att = np.stack([embed(c, rows, T, seed=70 + k) for k, c in enumerate(cores)])
    return {'att': att, 'mel_len': [c.shape[0] for c in cores], 'x_len': [c.shape[1] for c in cores]}


SCORE_R = (1, 2, 3)
SCORE_MEL_LENS = {1: [50, 37, 23], 2: [101, 37, 23], 3: [152, 37, 23]}  # item 0: mel_len // r == rows


def score_case():
    """B = 3, rows = 50, T = 20: soft alignments whose peak sometimes jumps, every row in play
    for some r (the rows past an item's mel_len // r are decoys for that r)."""
    g = _rng(60)
    att = np.stack([soft(50, 20, 1.5, 61 + b) for b in range(3)])
    for b in range(3):
        for t in g.choice(np.arange(2, 50), 9, replace=False):  # jumps of 2..6 tokens
            att[b, t] = np.roll(att[b, t], int(g.integers(2, 7)))
    return att


def strided(case):
    """The case's input in a buffer with row stride ld_row (decoys in the gap)."""
    a = case['att']
    ld = case.get('ld_row', a.shape[1])
    buf = np.full((a.shape[0], ld), 0.99, np.float32)
    buf[:, :a.shape[1]] = a
    return buf


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ---- the restatement ---------------------------------------------------------------------

def durations_dp(att, mel_len, x_len, defect=None):
    """-> (dur int32 [T], cost float64, unique).  unique: at every step of the backtracked path
    the best predecessor is strictly smaller than the second best."""
    rows, T = att.shape
    R = rows if defect == 'read_pad_rows' else mel_len
    C = T if defect == 'ignore_x_len' else x_len
    w = (np.float32(1.0) - att[:R, :C].astype(np.float32)).astype(np.float64)
    inf = np.inf
    D = np.full((R, C), inf)
    D[0, 0] = 0.0
    choice = np.zeros((R, C), np.int8)
    for i in range(R):
        for j in range(C):
            if i == j == 0:
                continue
            cand = [D[i - 1, j - 1] if i and j and defect != 'no_diag' else inf,
                    D[i - 1, j] if i else inf, D[i, j - 1] if j else inf]
            k = int(np.argmin(cand))  # first of diagonal, up, left
            src = [(i - 1, j - 1), (i - 1, j), (i, j - 1)][k]
            D[i, j] = (w[src] if defect == 'src_weight' else w[i, j]) + cand[k]
            choice[i, j] = k
    dur = np.zeros(T, np.int32)
    i, j, unique = R - 1, C - 1, True
    col = {i: j}
    while (i, j) != (0, 0):
        cand = sorted([D[i - 1, j - 1] if i and j and defect != 'no_diag' else inf,
                       D[i - 1, j] if i else inf, D[i, j - 1] if j else inf])
        unique = unique and cand[0] < cand[1]
        k = choice[i, j]
        i, j = [(i - 1, j - 1), (i - 1, j), (i, j - 1)][k]
        if defect == 'first_col' or i not in col:
            col[i] = j
    for j in col.values():
        dur[j] += 1
    return dur, float(D[R - 1, C - 1]), unique


def durations_count(att, mel_len, x_len, defect=None):
    rows, T = att.shape
    C = T if defect == 'ignore_x_len' else x_len
    a = att[:, :C]
    arg = (C - 1 - np.argmax(a[:, ::-1], 1)) if defect == 'last_argmax' else np.argmax(a, 1)
    raw = arg.copy()
    for t in range(1, rows):
        if abs(int(arg[t]) - int((raw if defect == 'unrepaired' else arg)[t - 1])) > 10:
            arg[t] = arg[t - 1]
    n = rows if defect == 'read_pad_rows' else mel_len
    dur = np.zeros(T, np.int32)
    cnt = np.bincount(arg[:n], minlength=1)
    dur[:len(cnt)] = cnt
    return dur


def scores(att, mel_lens, r, defect=None):
    """-> (loc, sharp) float64 [B]: exact count / (L - 1) and the fp64 sum / rows."""
    B, rows, T = att.shape
    loc, sharp = np.zeros(B), np.zeros(B)
    for b in range(B):
        L = mel_lens[b] // r
        n = min(rows, L)
        arg = np.argmax(att[b], 1)
        top = att[b].max(1).astype(np.float64)
        m = rows if defect == 'loc_over_rows' else n
        cnt = sum(abs(int(arg[t]) - int(arg[t - 1])) <= r for t in range(1, m))
        loc[b] = cnt / (L - 1) if L != 1 else np.nan
        sharp[b] = top[:n].sum() / (mel_lens[b] if defect == 'sharp_by_mel_len' else rows)
    return loc, sharp
