"""Host-side (numpy) half of the recurrence tests: a plain reference of ftmi_rnn_bidir over its
own operands, the weight and input patterns, the bound, emulations of subtly wrong kernels and
the table of cases that visits every rnn_gemv_kernel / rnn_bidir_kernel instantiation with
`lengths`, `index`, several passes, T < 3 and weights and inputs off the unit scale.

Not a conftest and not a test module: imported by test_rnn_cases.py (CPU: the reference against
torch.nn.GRU / LSTM, the conditions every case must meet, the defects against the bound, the
routes) and test_gpu_rnn_cases.py (GPU: the kernels against `recur_ref` in float64).

The bound (the idiom of bound B in test_gpu_value_domain.py):
    max |got - ref64| <= F_max  E32_max  + FLOOR
    mean|got - ref64| <= F_mean E32_mean + FLOOR / 8
with E32 the error of the same recurrence in float32 on the host (numpy: exact exp, another
summation order) and FLOOR = 2^-22, four ulps of a value in [0.5, 1): the step tag in the
mantissa LSB of h (at most 1 ulp) and fast_tanh = 2 sigmoid(2x) - 1, which doubles the ulp of
a sigmoid near 0.5 and takes rcpf's ulp on top.  F is one pair per arithmetic path, twice the
worst ratio measured on the MI355X over that path's cases, rounded up to one significant digit
(the measured ratios: profiles/rnn_range.json, table in DESIGN.md section 6); inputs are seeded
and the kernels deterministic, the factor 2 is for compiler and runtime versions.

Patterns that push the recurrence into its chaotic regime say nothing about a kernel (float32
itself is then far from float64), so every case must satisfy E32_max <= E32_CAP on the host;
`outlier` weights and `saturating` inputs therefore run at T <= 4 only."""
import ctypes
import functools
from collections import namedtuple

import numpy as np

FLOOR = 2.0 ** -22
E32_CAP = 1e-5
PAD_VALUE = -11.5129
SPREAD = 0x100  # include/ftmi.h FTMI_RNN_SPREAD
SWITCH_NAMES = ('GEMV', 'GEMV_KSEG', 'XCD_LOCAL', 'PAD', 'U64', 'CSTORE', 'CELLROWS', 'NB', 'U8',
                'PSLEEP')

# (F_max, F_mean) per path: 2 x the worst measured ratio |err| / E32, one significant digit,
# rounded up (MI355X; profiles/rnn_range.json holds every run's ratios).  Worst ratios:
#   f16x3   9.66 (domain-gru128-f16-T3)        2.96 (short-lstm-cr-T1-lengths)
#   bf16x6  2.36 (short-gru256-cst-T1-plain)   3.02 (short-lstm-cr-T1-lengths)
#   f32     2.36 (short-gru256-cst-T1-plain)   3.02 (short-lstm-cr-T1-lengths)
#   gemv    2.82 (form-gemv-lstm-k8-B1-plain)  3.86 (form-gemv-lstm-k8-B1-plain)
# The ratios near 3 belong to T = 1 and B = 1 cases whose E32 is below an ulp and whose error
# lies inside FLOOR; beyond FLOOR no bf16x6 / f32 / gemv run exceeds 1.3 x E32.  The f16x3
# 9.66 is the pre-split h exchange: the f16 tail carries a step tag in its LSB too, so the
# exchanged pair holds h to 2^-21 (csrc/rnn.hip, HSPLIT), which 2^5-scaled W_hh rows make
# visible (the next f16x3 ratio is 4.0, every `unit` and `rows` case is below 3.4).
F = {'f16x3': (20.0, 6.0), 'bf16x6': (5.0, 7.0), 'f32': (5.0, 7.0), 'gemv': (6.0, 8.0)}
PATH_OF_MMA = {2: 'f16x3', 1: 'bf16x6', 0: 'f32'}


# ---------------------------------------------------------------- the reference
def _sigmoid(x):
    return 1 / (1 + np.exp(-x))


def _recur(cell, xp, w_hh, b_hh, dtype, index=None, xp_zero=None, lengths=None, pad_value=0.0,
           defect=None, nbl=16, stats=None):
    """ftmi_rnn_bidir in plain numpy at `dtype`; `defect` plants one of DEFECTS; `stats`
    (a dict) receives the fractions of sigmoid gates above 0.99 / below 0.01 on live frames."""
    G = 4 if cell else 3
    xp = np.asarray(xp).astype(dtype)
    w = np.asarray(w_hh).astype(dtype)
    B, H = xp.shape[0], w.shape[2]
    rows = np.arange(B)
    if defect == 'f':  # a later chunk reads the lengths / index rows of chunk 0
        rows = rows % nbl
    if defect == 'b':
        w = w.astype(np.float16).astype(dtype)
    if index is not None:
        idx = np.asarray(index)[rows]
        T = idx.shape[1]
        xe = xp[np.arange(B)[:, None], np.maximum(idx, 0)]
        if defect != 'e':
            xe = np.where((idx >= 0)[..., None], xe, np.asarray(xp_zero).astype(dtype))
    else:
        xe, T = xp, xp.shape[1]
    lens = np.full(B, T) if lengths is None else np.asarray(lengths)[rows]
    y = np.empty((B, T, 2 * H), dtype)
    hi = lo = n = 0
    with np.errstate(over='ignore'):
        for d in (0, 1):
            wt = np.ascontiguousarray(w[d].T)
            bias = None if b_hh is None else np.asarray(b_hh)[d * G * H:(d + 1) * G * H].astype(dtype)
            h = np.zeros((B, H), dtype)
            c = np.zeros((B, H), dtype)
            for s in range(T):
                t = T - 1 - s if d else s
                live = (t < lens)[:, None]
                gx = xe[:, t, d * G * H:(d + 1) * G * H]
                gs = (h.astype(np.float16).astype(dtype) if defect == 'a' else h) @ wt
                if cell == 0:
                    gs = gs + bias
                    r = _sigmoid(gx[:, :H] + gs[:, :H])
                    z = _sigmoid(gx[:, H:2 * H] + gs[:, H:2 * H])
                    nn = np.tanh(gx[:, 2 * H:] + r * gs[:, 2 * H:])
                    hn = nn + z * (h - nn)
                    gates = (r, z)
                else:
                    g = gx + gs
                    i, f, o = _sigmoid(g[:, :H]), _sigmoid(g[:, H:2 * H]), _sigmoid(g[:, 3 * H:])
                    c = f * c + i * np.tanh(g[:, 2 * H:3 * H])
                    hn = o * np.tanh(c)
                    gates = (i, f, o)
                if stats is not None:
                    for a in gates:
                        hi += np.count_nonzero(a[live[:, 0]] > 0.99)
                        lo += np.count_nonzero(a[live[:, 0]] < 0.01)
                        n += a[live[:, 0]].size
                if defect == 'c' and d == 1:  # the reverse pass runs through the padding
                    h = hn
                else:
                    h = np.where(live, hn, 0).astype(dtype)
                    c = np.where(live, c, 0).astype(dtype)
                out = h if defect == 'd' else np.where(live, h, dtype(pad_value))
                y[:, t, d * H:(d + 1) * H] = out
    if stats is not None:
        stats.update(sat_hi=hi / max(n, 1), sat_lo=lo / max(n, 1))
    return y


def recur_ref(cell, xp, w_hh, b_hh, dtype, index=None, xp_zero=None, lengths=None, pad_value=0.0):
    """The bidirectional GRU (cell 0) / LSTM (cell 1) recurrence over ops.rnn_bidir's operands:
    xp (B, T_src, 2 G H) input projections [forward | reverse], w_hh (2, G H, H), b_hh (2 G H)
    or None (LSTM), PyTorch's gate order (r z n / i f g o).  index (B, T): frame -> source row,
    -1 reads xp_zero; frames t >= lengths[b] give pad_value and the reverse direction starts at
    lengths[b] - 1 (pack_padded_sequence / pad_packed_sequence).  -> (B, T, 2 H) at `dtype`."""
    return _recur(cell, xp, w_hh, b_hh, dtype, index, xp_zero, lengths, pad_value)


# Host emulations of a subtly wrong kernel, in recur_ref's calling convention (f takes `nbl`,
# the live sequences per group of the form it emulates):
#  a  h reduced to its f16 head in W_hh h          b  W_hh reduced to its f16 head
#  c  the reverse direction starts at T - 1        d  padded frames carry h, not pad_value
#  e  index == -1 reads source row 0, not xp_zero  f  chunk c > 0 reads chunk 0's lengths / index
DEFECTS = {k: functools.partial(_recur, defect=k) for k in 'abcdef'}


def errors(got, ref64):
    d = np.abs(np.asarray(got, np.float64) - ref64)
    return float(d.max()), float(d.mean())


def bound(ref64, ref32, path):
    """((max bound, mean bound), (E32 max, E32 mean)) of one case on one path."""
    e_max, e_mean = errors(ref32, ref64)
    f_max, f_mean = F[path]
    return (f_max * e_max + FLOOR, f_mean * e_mean + FLOOR / 8), (e_max, e_mean)


# ---------------------------------------------------------------- patterns
def unit_scales(pattern, H):
    """The scale of each hidden unit, applied to all of its gate rows in both directions."""
    u = np.arange(H)
    if pattern == 'unit':
        return np.ones(H, np.float32)
    if pattern == 'rows':  # -6 .. +2; the stride 5 is coprime to 8, 16, 32 and to the cycle of 9:
        # any 8 consecutive units (a workgroup's slice, half a row block) carry 8 scales
        return np.ldexp(np.float32(1), -6 + (5 * u) % 9).astype(np.float32)
    if pattern.startswith('outlier'):  # 'outlier4': a tamer high exponent (see E32_CAP)
        e = np.zeros(H, np.int64)
        e[5::16] = int(pattern[7:] or 5)
        e[11::32] = -6
        return np.ldexp(np.float32(1), e).astype(np.float32)
    raise ValueError(pattern)


def weights(rng, cell, H, pattern):
    G = 4 if cell else 3
    w = rng.normal(0, 1 / np.sqrt(H), (2, G * H, H)).astype(np.float32)
    w *= np.tile(unit_scales(pattern, H), G)[None, :, None]
    b = None if cell else rng.normal(0, 0.1, 2 * G * H).astype(np.float32)
    return w, b


def inputs(rng, cell, H, B, T_src, pattern):
    G = 4 if cell else 3
    xp = rng.normal(0, 1, (B, T_src, 2 * G * H)).astype(np.float32)
    if pattern == 'unit':
        return xp
    if pattern == 'batch':
        return xp * np.array([0.25, 1.0, 4.0], np.float32)[np.arange(B) % 3][:, None, None]
    if pattern == 'saturating':
        # x 16 on a fixed third of the (sequence, unit) pairs: gates pinned at 0 / 1, h at +-1;
        # exact zeros on a seventh of them; sequence 1 all zero (the LSTM's h stays 0)
        b, u = np.arange(B)[:, None], np.arange(H)[None, :]
        s = np.where((b + u) % 3 == 0, 16.0, 1.0)
        s = np.where((b + 2 * u) % 7 == 3, 0.0, s).astype(np.float32)
        if B > 1:
            s[1] = 0
        return xp * np.tile(s, 2 * G)[:, None, :]
    raise ValueError(pattern)


def make_lengths(B, T):
    """In [1, T], with 1 and T among them (B >= 2), lengths[b] != lengths[b - 8], [b - 16]."""
    if B == 1:
        return np.array([max(1, T - 2)], np.int32)
    b = np.arange(B)
    lens = 1 + (5 * b + b // 8) % T
    if T not in lens:
        lens[1] = T
    return lens.astype(np.int32)


def make_index(rng, B, T, T_src):
    """A frame -> source row map with repeats, a tail of -1 (0..2 frames) and, in every fourth
    row, a -1 at frame 1 (inside the sequence whatever its length, if above 1); frame 0 differs
    between rows b, b - 8 and b - 16."""
    idx = rng.integers(0, T_src, (B, T)).astype(np.int32)
    b = np.arange(B)
    idx[:, 0] = (b + b // 8) % T_src
    for i in range(B):
        tail = min(i % 3, T - 1)
        if tail:
            idx[i, T - tail:] = -1
        if i % 4 == 1 and T >= 3:
            idx[i, 1] = -1
    return idx


# ---------------------------------------------------------------- forms
# name -> (cell, H, mma, spread, switches, (kernel, units, wk, mode, cst, nbl, cr, kseg, nbv)).
# The switches are those of PER_CALL_CASES and ROW_VARIANTS in test_gpu_kernels.py; a GEMV form's
# nbv is filled in from the case's B.
Form = namedtuple('Form', 'cell H mma spread switches route')
G0 = {'GEMV': '0'}


def _bidir(cell, H, mma, spread, switches, units, wk, cst=0, nbl=16, cr=0):
    return Form(cell, H, mma, spread, dict(G0, **switches), ('bidir', units, wk, mma, cst, nbl, cr, 0, 0))


def _gemv(cell, H, kseg):
    sw = {'GEMV_KSEG': '8'} if kseg == 8 and H >= 256 else {}
    return Form(cell, H, 2, False, sw, ('gemv', 16, 0, 0, 0, 0, 0, kseg, None))


BIDIR_FORMS = {
    'gru64-u32': _bidir(0, 64, 2, False, {}, 32, 2),
    'gru64-u64': _bidir(0, 64, 2, False, {'U64': '64'}, 64, 2),
    'gru64-u64-bf16': _bidir(0, 64, 1, False, {}, 64, 2),
    'gru64-u64-f32': _bidir(0, 64, 0, False, {}, 64, 4),
    'gru128-f16': _bidir(0, 128, 2, False, {}, 16, 4),
    'gru128-bf16': _bidir(0, 128, 1, False, {}, 16, 4),
    'gru128-f32': _bidir(0, 128, 0, False, {}, 16, 4),
    'gru256-u8-cr': _bidir(0, 256, 2, True, {}, 8, 4, cst=1, cr=1),
    'gru256-u8': _bidir(0, 256, 2, True, {'CELLROWS': '0'}, 8, 4, cst=1),
    'gru256-nbl8': _bidir(0, 256, 2, True, {'U8': '0'}, 16, 4, cst=1, nbl=8),
    'gru256-cst': _bidir(0, 256, 2, False, {}, 16, 4, cst=1),
    'gru256-cst-spread': _bidir(0, 256, 2, True, {'U8': '0', 'NB': '16'}, 16, 4, cst=1),
    'gru256-comm': _bidir(0, 256, 2, False, {'CSTORE': '0'}, 16, 4),
    'gru256-bf16': _bidir(0, 256, 1, False, {}, 16, 4),
    'gru256-f32': _bidir(0, 256, 0, False, {}, 16, 4),
    'lstm-cr': _bidir(1, 512, 2, True, {}, 16, 4, cst=1, cr=1),
    'lstm-cst': _bidir(1, 512, 2, True, {'CELLROWS': '0'}, 16, 4, cst=1),
    'lstm-comm': _bidir(1, 512, 2, False, {'CSTORE': '0'}, 16, 4),
    'lstm-bf16': _bidir(1, 512, 1, False, {}, 16, 4),
    'lstm-f32': _bidir(1, 512, 0, False, {}, 16, 4),
}
GEMV_FORMS = {
    'gemv-lstm-k8': _gemv(1, 512, 8), 'gemv-lstm-k16': _gemv(1, 512, 16),
    'gemv-gru256-k8': _gemv(0, 256, 8), 'gemv-gru256-k16': _gemv(0, 256, 16),
    'gemv-gru128-k8': _gemv(0, 128, 8), 'gemv-gru64-k8': _gemv(0, 64, 8),
}
FORMS = dict(BIDIR_FORMS, **GEMV_FORMS)
# one form per (kernel family, units): GEMV, U 8, U 16 with and without CST, U 32, U 64, the
# LSTM with and without CR
SHORT_FORMS = ('gemv-gru256-k16', 'gru256-u8-cr', 'gru256-cst', 'gru128-f16', 'gru64-u32', 'gru64-u64',
               'lstm-cr', 'lstm-cst')
# the forms whose group fills fewer workgroups than the CUs, so that a batch reaches a second pass
PASS_FORMS = ('lstm-cr', 'gru256-cst', 'gru128-f16', 'gru64-u32')

MODES = ('plain', 'lengths', 'index', 'index+lengths')
# B = None: the first B at which the form's launch takes two passes on the device at hand
Case = namedtuple('Case', 'id axis form B T mode wpat xpat')


def _table():
    t = []
    for name, f in BIDIR_FORMS.items():  # one full chunk plus one live sequence
        for mode in MODES:
            t.append(Case(f'form-{name}-{mode}', 'forms', name, f.route[5] + 1, 7, mode, 'rows', 'batch'))
    for name in GEMV_FORMS:  # B = 3: nbv = 4 with a dead column
        for B in (1, 2, 3, 4):
            for mode in ('plain', 'index+lengths'):
                t.append(Case(f'form-{name}-B{B}-{mode}', 'forms', name, B, 7, mode, 'rows', 'batch'))
    for name in SHORT_FORMS:  # (the GEMV kernel takes at most 4 sequences)
        for T in (1, 2, 3):
            for mode in ('plain', 'lengths'):
                B = 4 if name in GEMV_FORMS else 5
                t.append(Case(f'short-{name}-T{T}-{mode}', 'short', name, B, T, mode, 'rows', 'batch'))
    for name in SHORT_FORMS + ('gru256-bf16', 'gru256-f32', 'lstm-bf16', 'lstm-f32'):
        for T in (3, 4):
            B = 4 if name in GEMV_FORMS else 5
            # H 256 at 2^5: E32 max 1.01e-5 at T = 3, past E32_CAP; 2^4 keeps it below
            wpat = 'outlier4' if FORMS[name].H == 256 else 'outlier'
            t.append(Case(f'domain-{name}-T{T}', 'domain', name, B, T, 'plain', wpat, 'saturating'))
    for name, B in (('gru256-cst', 5), ('gru256-u8-cr', 16), ('lstm-cr', 5), ('gemv-lstm-k16', 2)):
        for T in (66, 301):  # both parities of the exchange buffer, every phase of the tag
            t.append(Case(f'drift-{name}-T{T}', 'drift', name, B, T, 'lengths', 'unit', 'unit'))
    for name in PASS_FORMS:
        t.append(Case(f'passes-{name}', 'passes', name, None, 4, 'index+lengths', 'rows', 'batch'))
    return t


CASES = _table()
CASE_BY_ID = {c.id: c for c in CASES}


# ---------------------------------------------------------------- routes
def clear_switches(monkeypatch, switches):
    """Every FTMI_RNN_* switch unset, then the case's own."""
    for n in SWITCH_NAMES:
        monkeypatch.delenv('FTMI_RNN_' + n, raising=False)
    for n, v in switches.items():
        monkeypatch.setenv('FTMI_RNN_' + n, v)


def route(form, B, mma=None, cus=256):
    """ftmi_rnn_route of `form` at batch B under the switches now in the environment."""
    from forwardtacotron_amd import _lib
    r = _lib.RnnRoute()
    m = (form.mma if mma is None else mma) | (SPREAD if form.spread else 0)
    assert _lib.load().ftmi_rnn_route(form.cell, B, form.H, m, cus, ctypes.byref(r)) == 0
    assert r.status == 0, (form, B, r.status)
    return r


def route_coords(r):
    from forwardtacotron_amd import _lib
    kernel = {_lib.RNN_KERNEL_GEMV: 'gemv', _lib.RNN_KERNEL_BIDIR: 'bidir'}[r.kernel]
    return (kernel, r.units, r.wk, r.mode, r.cst, r.nbl, r.cr, r.kseg, r.nbv)


def expected_coords(case, B):
    c = FORMS[case.form].route
    return c[:8] + ((B if B <= 2 else 4),) if c[0] == 'gemv' else c


def resolve_B(case, cus=256):
    """The case's batch size; B = None: the first B with two passes on `cus` CUs (0: the
    device's own), under the switches now in the environment."""
    if case.B is not None:
        return case.B
    form = FORMS[case.form]
    B = 5
    while route(form, B, cus=cus).passes < 2:
        B += 1
        assert B < 5000
    return B


def path_of(case):
    form = FORMS[case.form]
    return 'gemv' if form.route[0] == 'gemv' else PATH_OF_MMA[form.mma]


# ---------------------------------------------------------------- operands and references
Operands = namedtuple('Operands', 'cell H B T xp w_hh b_hh kw ref64 ref32 stats')


@functools.lru_cache(maxsize=None)
def operands(cell, H, B, T, mode, wpat, xpat):
    """Seeded operands of one (shape, call mode, patterns) and their float64 / float32
    references, computed once: forms that share a shape share them.  Treat as read-only."""
    seed = [cell, H, B, T, MODES.index(mode), sum(map(ord, wpat + xpat))]
    rng = np.random.Generator(np.random.PCG64(seed))
    T_src = T
    w_hh, b_hh = weights(rng, cell, H, wpat)
    xp = inputs(rng, cell, H, B, T_src, xpat)
    kw = {}
    if 'index' in mode:
        kw['index'] = make_index(rng, B, T, T_src)
        kw['xp_zero'] = rng.normal(0, 0.1, xp.shape[2]).astype(np.float32)
    if 'lengths' in mode:
        kw['lengths'] = make_lengths(B, T)
        kw['pad_value'] = PAD_VALUE
    stats = {}
    ref64 = _recur(cell, xp, w_hh, b_hh, np.float64, stats=stats, **kw)
    ref32 = recur_ref(cell, xp, w_hh, b_hh, np.float32, **kw)
    for a in (xp, w_hh, ref64, ref32) + tuple(v for v in kw.values() if isinstance(v, np.ndarray)):
        a.setflags(write=False)
    return Operands(cell, H, B, T, xp, w_hh, b_hh, kw, ref64, ref32, stats)


def case_operands(case, B):
    form = FORMS[case.form]
    return operands(form.cell, form.H, B, case.T, case.mode, case.wpat, case.xpat)


def live_mask(op):
    """(B, T) True where the frame is inside the sequence."""
    lens = op.kw.get('lengths')
    if lens is None:
        return np.ones((op.B, op.T), bool)
    return np.arange(op.T)[None, :] < lens[:, None]
