"""Cases for the sequence-side kernels (csrc/seq.hip above the length-aware batches: embedding,
the duration kernels, lr_index, length_regulate, series_proj_add, rowdot; csrc/transformer.hip:
embedding_posenc, lr_posenc) — test infrastructure only, no tests in here.

One plain numpy restatement per operation, written from the reference model's arithmetic
(nn.Embedding, generate()'s fill-2 rule, LengthRegulator, the pitch / energy Conv1d(1, C, 3),
SeriesPredictor's Linear(C, 1) / alpha, PositionalEncoding), deterministic inputs from
np.random.Generator(PCG64(seed)) with the seed in the table, and the case tables: the smallest
shapes that reach each branch of each kernel (the branch is named beside the case).

`defect=` plants one of DEFECTS in a restatement (tests/test_seq_cases.py: each must be rejected
by the comparison the device test uses, on a named case of its table).

Guarded buffers: an operand sits inside a flat buffer filled with a sentinel, GUARD elements
before and after it, at a chosen element offset and row stride; the device result is compared by
bits over the whole buffer, so a write into the stride gap, the lead-in or a guard shows.
"""
from __future__ import annotations

import numpy as np

from oracle import ft_oracle as O

# ---------------------------------------------------------------- guarded buffers
SENTINEL = np.float32(-777.25)
INT_SENTINEL = -77725
GUARD = 64  # elements of sentinel before and after the operand (a multiple of 4: 16-byte aligned)


def sentinel_of(dtype):
    return SENTINEL if np.dtype(dtype) == np.float32 else np.dtype(dtype).type(INT_SENTINEL)


def guarded(values, stride=None, offset=0):
    """(flat buffer, span): `values` (..., C) laid out as rows of `stride` >= C elements that
    start `offset` elements after the leading guard; everything else is the sentinel.
    buf[span] holds the rows * stride elements of the operand."""
    values = np.asarray(values)
    C = values.shape[-1]
    stride = C if stride is None else stride
    rows = values.size // C
    buf = np.full(GUARD + offset + rows * stride + GUARD, sentinel_of(values.dtype), values.dtype)
    span = slice(GUARD + offset, GUARD + offset + rows * stride)
    buf[span].reshape(rows, stride)[:, :C] = values.reshape(rows, C)
    return buf, span


def operand(buf, span, shape, stride=None):
    """The (..., C) operand of a guarded buffer (a numpy view or a torch view alike)."""
    C = shape[-1]
    stride = C if stride is None else stride
    rows = (span.stop - span.start) // stride
    return buf[span].reshape(rows, stride)[:, :C].reshape(shape)


def bits(a):
    """Bit-for-bit comparison key: fp32 as int32 words (NaN payloads, -0.0), integers as is."""
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def bound_ratio(got, ref, rtol, atol):
    """Worst |err| / bound under tests/test_gpu_kernels.close: bound = atol * max(1, rms(ref))
    + rtol * |ref|.  <= 1 exactly when close() passes."""
    ref = np.asarray(ref, np.float64)
    scale = max(1.0, float(np.sqrt(np.mean(np.square(ref)))))
    err = np.abs(np.asarray(got, np.float64) - ref)
    return float(np.max(err / (atol * scale + rtol * np.abs(ref))))


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


DEFECTS = {
    'fill_lt0': 'the fill-2 rule decided on sum < 0',
    'floor': 'truncation toward zero replaced by floor',
    'round': 'truncation toward zero replaced by round',
    'first1024': 'the sum taken over the first 1024 elements only',
    'ext32': 'ext_sum read as a 32-bit word',
    'own_sum': "the decision taken on the tensor's own sum although ext_sum is given",
    'inclusive_scan': 'offsets hold the inclusive scan',
    'carry64': 'the carry dropped at a 64-column boundary',
    'first_equal': 'lr_index chooses the first of equal offsets',
    'minus1_row0': 'index -1 mapped to row 0',
    'clamp': 'an id outside the table clamped to the edge row',
    'wrap32': 'an id wrapped modulo 2^32',
    'cross_item': 'a series neighbour read across the item boundary',
    'block0_weights': "column block 1 uses block 0's weights",
    'bias_after_div': 'rowdot adds the bias after the division',
    'flat_row': 'posenc indexed by the flat row instead of by t',
}


# ---------------------------------------------------------------- embedding
# (rows, dim, ids shape, seed).  dim 4: one float4 per row; (7, 260): dim4 = 65 is no power of
# two and n * dim4 = 650 threads is no multiple of the 256-thread workgroup.
EMBED = [
    (135, 4, (1, 1), 11),
    (135, 64, (3, 17), 12),
    (7, 260, (2, 5), 13),
]


def outside_ids(rows):
    return [-1, rows, 2 ** 32, 2 ** 32 + 1, -2 ** 40]


def embed_table(rows, dim, seed):
    return _rng(seed).normal(0.0, 1.0, (rows, dim)).astype(np.float32)


def embed_id_sets(rows, shape, seed):
    """{name: ids}: 'clean' holds in-table ids only, 0 and rows - 1 among them; every other set
    holds ids outside the table (-1, rows, 2^32, 2^32 + 1, -2^40) next to 0 and rows - 1.  A
    (1, 1) shape holds one id, so it gets one set per value."""
    n = int(np.prod(shape))
    special = [0, rows - 1] + outside_ids(rows)
    if n < len(special):
        sets = {'clean': np.zeros(shape, np.int64), 'clean_last': np.full(shape, rows - 1, np.int64)}
        for v in outside_ids(rows):
            sets[f'id={v}'] = np.full(shape, v, np.int64)
        return sets
    rng = _rng(seed)
    clean = rng.integers(0, rows, n).astype(np.int64)
    clean[0], clean[-1] = 0, rows - 1
    planted = clean.copy()
    pos = rng.permutation(np.arange(1, n - 1))[:len(outside_ids(rows))]
    planted[pos] = outside_ids(rows)
    return {'clean': clean.reshape(shape), 'planted': planted.reshape(shape)}


def embedding_ref(ids, table, defect=None):
    """nn.Embedding on ids inside the table, a zero row for any other id; also whether any id
    was outside the table."""
    ids = np.asarray(ids, np.int64)
    rows = table.shape[0]
    if defect == 'wrap32':
        ids = ids & np.int64(0xFFFFFFFF)
    ok = (ids >= 0) & (ids < rows)
    if defect == 'clamp':
        ids, ok = np.clip(ids, 0, rows - 1), np.ones_like(ok)
    if defect == 'minus1_row0':
        ids, ok = np.where(ids == -1, 0, ids), ok | (ids == -1)
    out = np.zeros(ids.shape + (table.shape[1],), table.dtype)
    out[ok] = table[ids[ok]]
    return out, bool((~ok).any())


# ---------------------------------------------------------------- duration kernels
# (B, T, seed): T across the 64-lane scan chunks (63, 64, 65, 129, 130), B across the 16 waves
# of the one workgroup (17 and 20 rows: rows 16.. are a wave's second row).
DUR = [(1, 1, 21), (1, 63, 22), (2, 64, 23), (3, 65, 24), (17, 129, 25), (20, 130, 26)]
KNOWN = (0.49999997, 1.5, 2.5, -0.75)  # counts 1 (fp32 0.49999997 + 0.5 = 1.0), 2, 3, 0 (clipped)


def dur_tensor(B, T, seed):
    dur = _rng(seed).uniform(-1.0, 6.0, (B, T)).astype(np.float32)
    if T >= 2 * len(KNOWN):
        for b in range(B):  # a different place in every row, never across the row's end
            p = (7 * b) % (T - len(KNOWN) + 1)
            dur[b, p:p + len(KNOWN)] = np.array(KNOWN, np.float32)
    return dur


# flat position of the one 1.25 in a (20, 130) tensor of values in (-0.99, 0.99): thread 0, the
# last thread of wave 15, the first element of the second pass of 1024, the last element (third
# pass).  With a -1.5 planted elsewhere the truncated sum is 0 (fill), without it 1 (no fill).
FILL_SHAPE, FILL_SEED = (20, 130), 31
FILL = [(p, neg) for p in (0, 1023, 1024, 2599) for neg in (True, False)]


def fill_tensor(p, neg):
    n = FILL_SHAPE[0] * FILL_SHAPE[1]
    dur = _rng(FILL_SEED).uniform(-0.99, 0.99, n).astype(np.float32)
    dur[p] = np.float32(1.25)
    if neg:
        dur[(p + n // 2) % n] = np.float32(-1.5)
    return dur.reshape(FILL_SHAPE)


EXT_SUMS = (-3, 0, 1, 2 ** 32)


def global_tensors():
    """{name: dur}: the (3, 65) DUR tensor (own sum > 0) and one whose own sum is <= 0."""
    low = _rng(41).uniform(-0.99, 0.99, (3, 65)).astype(np.float32)
    low[1, 7] = np.float32(-2.5)
    return {'dur_3x65': dur_tensor(3, 65, 24), 'own_sum_le_0': low}


TRUNC = [(1, 51), (1023, 52), (1025, 53), (2600, 54)]  # (n, seed)


def trunc_tensor(n, seed):
    """uniform(-1, 6) with -0.9 (floor differs), -1.5 and 2.5 (round differs), 3.0e9 twice and
    -3.0e9 once (the sum leaves int32); the last element is a 3.0e9, so a lost tail shows."""
    v = _rng(seed).uniform(-1.0, 6.0, n).astype(np.float32)
    v[n - 1] = np.float32(3.0e9)
    if n >= 8:
        v[0], v[1], v[2], v[3], v[n // 2] = -0.9, -1.5, 3.0e9, 2.5, -3.0e9
    return v


def trunc_sum_ref(dur, defect=None):
    dur = np.asarray(dur, np.float32).reshape(-1)
    if defect == 'first1024':
        dur = dur[:1024]
    f = {'floor': np.floor, 'round': np.round}.get(defect, np.trunc)
    return int(f(dur).astype(np.int64).sum())


def exclusive_offsets(counts, defect=None):
    """(B, T + 1) int32: offsets[b, t] = sum(counts[b, :t])."""
    counts = np.asarray(counts, np.int64)
    B, T = counts.shape
    off = np.zeros((B, T + 1), np.int64)
    off[:, 1:] = np.cumsum(counts, axis=1)
    if defect == 'inclusive_scan':
        off[:, :T] = off[:, 1:]
    if defect == 'carry64':  # every 64-column chunk starts again at 0
        for t0 in range(64, T, 64):
            off[:, t0:] -= off[:, t0:t0 + 1].copy()
    return off.astype(np.int32)


def duration_counts_ref(dur, apply_fill, fill=2.0, ext_sum=None, defect=None):
    """generate()'s fill-2 rule (decided on ext_sum if given, else on the tensor's own truncated
    sum: fill when it is <= 0), then the LengthRegulator clip and counts.  Returns (dur after the
    call, offsets (B, T + 1) int32, totals (B,) int32, flag)."""
    dur = np.array(dur, np.float32)
    flag = 0
    if apply_fill:
        if ext_sum is not None and defect != 'own_sum':
            s = int(ext_sum)
            if defect == 'ext32':
                s = int(np.array(s, np.int64).astype(np.int32))
        else:
            s = trunc_sum_ref(dur, defect)
        if (s < 0) if defect == 'fill_lt0' else (s <= 0):
            dur[:] = np.float32(fill)
            flag = 1
    dur[dur < 0] = np.float32(0)
    off = exclusive_offsets(O.duration_counts(dur), defect)
    return dur, off, off[:, -1].copy(), flag


# ---------------------------------------------------------------- LengthRegulator
def _lr300():
    return _rng(61).integers(0, 5, (2, 300)).astype(np.int64)


# name -> count rows (B, T): zero-count runs at both ends; T = 1; a row whose total is 0 beside a
# row that has frames; T = 300 with totals beyond 512 frames (three index blocks of 256)
LR = {
    'zero_runs': np.array([[0, 0, 3, 0, 2, 0, 0]], np.int64),
    't1': np.array([[5]], np.int64),
    'empty_row': np.array([[0, 0, 0, 0], [1, 0, 2, 0]], np.int64),
    't300': _lr300(),
}


def lr_tmels(counts):
    """T_mel: the largest total, 5 beyond it (-1 in every row), 3 below it (the sharded crop), 1, 0."""
    m = int(np.asarray(counts).sum(axis=1).max())
    return sorted({m, m + 5, max(m - 3, 0), 1, 0}, reverse=True)


def lr_index_ref(offsets, T_mel, defect=None):
    """repeat_interleave(arange(T), counts) per row, -1 past the row's total, cropped to T_mel."""
    offsets = np.asarray(offsets)
    B, T = offsets.shape[0], offsets.shape[1] - 1
    counts = np.diff(offsets.astype(np.int64), axis=1)
    idx = np.full((B, T_mel), -1, np.int32)
    for b in range(B):
        r = np.repeat(np.arange(T), counts[b])[:T_mel]
        if defect == 'first_equal':  # the first t whose offset equals the chosen one
            r = np.searchsorted(offsets[b, :T], offsets[b, :T][r], side='left')
        idx[b, :len(r)] = r
    return idx


def length_regulate_ref(x, index, defect=None):
    """y[b, f] = x[b, index[b, f]], a zero row where index is -1."""
    B = x.shape[0]
    rows = x[np.arange(B)[:, None], np.maximum(index, 0)]
    if defect == 'minus1_row0':
        return rows
    return np.where(index[..., None] >= 0, rows, np.float32(0)).astype(np.float32)


def scaled_pe(pe, scale, rows, width):
    return (np.float32(scale) * pe[:rows, :width].astype(np.float32)).astype(np.float32)


def lr_posenc_ref(x, index, pe, scale, defect=None):
    """LengthRegulator + PositionalEncoding: v + s * pe[t], product and sum rounded to fp32
    one after the other."""
    B, T_mel = index.shape
    v = length_regulate_ref(x, index, defect)
    if defect == 'flat_row':
        return v + scaled_pe(pe, scale, B * T_mel, x.shape[2]).reshape(B, T_mel, -1)
    return v + scaled_pe(pe, scale, T_mel, x.shape[2])[None]


def embedding_posenc_ref(ids, table, pe, scale, defect=None):
    B, T = ids.shape
    v, outside = embedding_ref(ids, table, defect if defect != 'flat_row' else None)
    if defect == 'flat_row':
        return v + scaled_pe(pe, scale, B * T, table.shape[1]).reshape(B, T, -1), outside
    return v + scaled_pe(pe, scale, T, table.shape[1])[None], outside


GRID_CAP = 8192 * 256  # elements one pass of the capped posenc grids covers

# (name, B, T, T_mel, C, x row stride, seed).  B * T_mel is no multiple of 4 (a partial last
# workgroup of 4 frame rows); C = 260 runs the lane loop (C / 4 = 65 > 64 lanes); stride C + 4 is
# a view into wider rows; 'grid' is 3 * 700 * 1024 = 2.15 M elements, beyond GRID_CAP.
EXPAND_LR = [(f'C{C}_s{S}', 3, 5, 7, C, S, 70 + i)
             for i, (C, S) in enumerate([(4, 4), (4, 8), (256, 256), (256, 260), (260, 260), (260, 264)])]
EXPAND_LR.append(('grid', 3, 8, 700, 1024, 1024, 79))
# lr_posenc also takes widths that are no multiple of 4
EXPAND_LRPE = EXPAND_LR[:-1] + [('C6_s6', 3, 5, 7, 6, 6, 77), ('C6_s10', 3, 5, 7, 6, 10, 78), EXPAND_LR[-1]]
# (name, B, T, rows, dim, seed): ids outside the table among them
EXPAND_EMBPE = [('d6', 2, 5, 9, 6, 81), ('d256', 2, 5, 9, 256, 82), ('grid', 3, 700, 11, 1024, 83)]
PE_SCALE = np.float32(0.7310586)


def expand_inputs(B, T, T_mel, C, seed):
    """x (B, T, C), index (B, T_mel) with repeats, skipped phonemes, a row cropped at T_mel and
    a row that ends before it (-1 tail), pe (B * T_mel, C) (its first T_mel rows are the kernel's)."""
    rng = _rng(seed)
    x = rng.normal(0.0, 1.0, (B, T, C)).astype(np.float32)
    hi = max(2, (2 * T_mel) // T + 1)
    counts = rng.integers(0, hi, (B, T)).astype(np.int64)
    counts[0, 0], counts[0, -1] = 0, 0
    counts[B - 1, T // 2:] = 0  # the last row stays short of T_mel
    counts[B - 1, 0] = max(1, T_mel // 3)
    counts[1, 1] = T_mel  # the second row is cropped
    index = lr_index_ref(exclusive_offsets(counts), T_mel)
    pe = rng.normal(0.0, 1.0, (B * T_mel, C)).astype(np.float32)
    return x, index, pe


def embpe_inputs(B, T, rows, dim, seed):
    rng = _rng(seed)
    table = rng.normal(0.0, 1.0, (rows, dim)).astype(np.float32)
    ids = rng.integers(0, rows, B * T).astype(np.int64)
    ids[0], ids[-1] = 0, rows - 1
    pos = rng.permutation(np.arange(1, B * T - 1))[:len(outside_ids(rows))]
    ids[pos] = outside_ids(rows)
    pe = rng.normal(0.0, 1.0, (B * T, dim)).astype(np.float32)
    return ids.reshape(B, T), table, pe


# ---------------------------------------------------------------- series_proj_add
SP_ROWS, SP_BLOCK_COLS = 32, 1024  # seq.hip: rows per chunk, columns per block (256 threads x 4)
STRENGTHS = (0.7, -1.3)

# name -> (B, T, C, row stride, float offset of x, float offset of wp, vector path?, seed)
SPA = {
    'v_t1': (1, 1, 4, 4, 0, 0, True, 91),             # both neighbours are the zero padding
    'v_2blocks': (3, 33, 2048, 2048, 0, 0, True, 92),  # two column blocks; chunks cross both item ends
    'v_partial': (2, 19, 1028, 1032, 0, 0, True, 93),  # partial second block; stride > C
    's_c6': (3, 5, 6, 6, 0, 0, False, 94),             # scalar: C % 4 != 0
    's_c514': (2, 7, 514, 514, 0, 0, False, 95),       # scalar, more than one pass of 256 threads
    's_stride': (2, 7, 512, 514, 0, 0, False, 96),     # scalar by stride
    's_addr': (2, 7, 512, 512, 1, 0, False, 97),       # scalar by the address of x
    's_wp_addr': (2, 7, 512, 512, 0, 1, False, 98),    # scalar by the address of wp
}


def spa_vector_path(C, stride, x_off, wp_off, we_off=0, bp_off=0, be_off=0):
    """ftmi_series_proj_add's choice, for operands at float offsets from 16-byte aligned bases."""
    return C % 4 == 0 and stride % 4 == 0 and not any(o % 4 for o in (x_off, wp_off, we_off, bp_off, be_off))


def spa_inputs(B, T, C, seed):
    """x, pitch, energy, wp, bp, we, be.  The last value of item b and the first of item b + 1
    are +-8: a neighbour read across an item's end misses by about 8 |w|."""
    rng = _rng(seed)
    x = rng.normal(0.0, 1.0, (B, T, C)).astype(np.float32)
    p = rng.normal(0.0, 1.0, (B, T)).astype(np.float32)
    e = rng.normal(0.0, 1.0, (B, T)).astype(np.float32)
    for b in range(B - 1):
        p[b, T - 1], p[b + 1, 0] = 8.0, -8.0
        e[b, T - 1], e[b + 1, 0] = -8.0, 8.0
    wp = rng.normal(0.0, 0.5, (C, 3)).astype(np.float32)
    we = rng.normal(0.0, 0.5, (C, 3)).astype(np.float32)
    bp = rng.normal(0.0, 0.1, C).astype(np.float32)
    be = rng.normal(0.0, 0.1, C).astype(np.float32)
    return x, p, e, wp, bp, we, be


def _conv_k3(s, w, b, defect):
    """Conv1d(1, C, 3, padding=1) of a (B, T) series, float64: (B, T, C)."""
    B, T = s.shape
    s, w, b = s.astype(np.float64), w.astype(np.float64), b.astype(np.float64)
    if defect == 'cross_item':  # one zero at each end of the whole batch only
        flat = np.concatenate([[0.0], s.reshape(-1), [0.0]])
        left, right = flat[:-2].reshape(B, T), flat[2:].reshape(B, T)
    else:
        sp = np.zeros((B, T + 2))
        sp[:, 1:T + 1] = s
        left, right = sp[:, :T], sp[:, 2:]
    if defect == 'block0_weights':
        col = np.arange(w.shape[0]) % SP_BLOCK_COLS
        w, b = w[col], b[col]
    return left[..., None] * w[:, 0] + s[..., None] * w[:, 1] + right[..., None] * w[:, 2] + b


def series_proj_add_ref(x, pitch, wp, bp, ps, energy, we, be, es, defect=None):
    """x + ps (conv1d_k3(pitch) + bp) + es (conv1d_k3(energy) + be), zero padding per item; float64."""
    return (x.astype(np.float64) + np.float64(ps) * _conv_k3(pitch, wp, bp, defect)
            + np.float64(es) * _conv_k3(energy, we, be, defect))


# ---------------------------------------------------------------- rowdot
ROWDOT_C = (1, 63, 64, 65, 200)   # below a wave, one lane idle, one pass, one lane's second pass, 4 passes
ROWDOT_M = {1: (1, 1), 3: (1, 3), 4: (2, 2), 5: (1, 5), 38: (2, 19)}  # M = B * T -> (B, T)
ROWDOT_ALPHA = (1.0, 1.3, 1000.0)
ROWDOT_BIAS = np.float32(0.3)


def rowdot_inputs(C, M):
    rng = _rng(1000 * C + M)
    return rng.normal(0.0, 1.0, (M, C)).astype(np.float32), rng.normal(0.0, 1.0, C).astype(np.float32)


def rowdot_ref(x, w, bias, alpha, defect=None):
    """Linear(C, 1)(x) / alpha, float64; bias None: no bias."""
    b = 0.0 if bias is None else float(bias)
    d = x.astype(np.float64) @ w.astype(np.float64)
    if defect == 'bias_after_div':
        return d / float(alpha) + b
    return (d + b) / float(alpha)
