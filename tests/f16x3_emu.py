"""Host-side (numpy) helpers of the value-domain tests: the weight patterns that make the
f16x3 column scale vary, the bounds, the structured attention inputs, and emulations of the
f16x3 GEMM and of the f16x3 flash attention with its lazy running max — close enough to the
kernels' arithmetic (f16 head / scaled tail operands, exact products, fp32 accumulation,
fp32 exp2) to say what error that arithmetic itself makes, and with switches that plant the
defects the GPU tests exist to catch (tests/test_value_domain_emu.py: the negative controls
run on the emulation only).

Not a conftest and not a test module: imported by test_value_domain_emu.py (CPU) and
test_gpu_value_domain.py (GPU)."""
import numpy as np

TS = np.float32(2048.0)      # tail scale 2^11
AH_KT = 64                   # keys per attention tile (transformer.hip)
AH_LAZY = 8.0                # the running max moves when a tile's max exceeds it by more
LOG2E = np.float32(1.4426950408889634)

# ---------------------------------------------------------------- bounds
# bound B: max|got - ref64| <= F * E32 + FLOOR * max|v|, E32 = max|ref32 - ref64| of the same
# formula in float32 on the host.  The emulation below stays within 0.55 x E32 on every B case
# (test_value_domain_emu.py recomputes that and holds it to F / 2), so 2 x its worst ratio is
# 1.1; the fp32 kernel (mma = 0) is held to the same bound and is one more draw of the fp32
# arithmetic that E32 measures (another summation order), whose maximum over the outputs can
# exceed E32's draw, but not by 2 x: F = 2.
ATTN_F = 2.0
ATTN_FLOOR = 2e-6


def bound_a(ref, atol, rtol):
    """Bound A: |err[:, n]| <= atol * rms(ref[:, n]) + rtol * |ref[:, n]| per output column n
    (ref: (rows, N) float64).  No max(1, .) floor: the columns' magnitudes differ by 2^16."""
    ref = np.asarray(ref, np.float64)
    rms = np.sqrt(np.mean(np.square(ref), axis=0, keepdims=True))
    return atol * rms + rtol * np.abs(ref)


def worst_ratio_a(got, ref, atol, rtol):
    """max |got - ref| / bound_a (0 / 0 counts as 0: an all-zero column must come out zero)."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    b = bound_a(ref, atol, rtol)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(err == 0, 0.0, err / b)
    return float(np.max(r))


# ---------------------------------------------------------------- weight patterns
def rows_exponents(N, group=0, lo=-3, hi=13):
    """j_n = (5 n mod 17) - 3 (+ the bank group index); a narrower [lo, hi] wraps into it."""
    j = (5 * np.arange(N)) % 17 - 3 + group
    if (lo, hi) != (-3, 13):  # (the default span is left unwrapped: group g reaches 13 + g)
        j = lo + (j - lo) % (hi - lo + 1)
    return j


def rows_pattern(w0, group=0, lo=-3, hi=13):
    """w[n] = w0[n] 2^{j_n}: the column scale differs between neighbouring columns, between
    16-column tiles and (group) between bank groups.  w0: (N, ...) fp32."""
    j = rows_exponents(w0.shape[0], group, lo, hi)
    return np.ldexp(w0, j.reshape((-1,) + (1,) * (w0.ndim - 1))).astype(np.float32)


def outlier_pattern(w0, group=0):
    """w0 with one entry per row set to +-2^{(n + group) mod 14} at (flat) column 7 n mod K:
    the scale exponent goes up to 10 while the output stays O(outlier x)."""
    w = w0.copy()
    flat = w.reshape(w.shape[0], -1)
    n = np.arange(flat.shape[0])
    flat[n, (7 * n) % flat.shape[1]] = np.where(n % 2, -1.0, 1.0) * np.ldexp(1.0, (n + group) % 14)
    return w


def boundary_rows(w, first):
    """Rows first .. first + 4 of w (N, ...) become: max|w| exactly 16.0, nextafter(16, 0),
    32.0, all zero, 2^-20-sized.  Returns the expected scale exponents e of those rows."""
    # (e = 1: 16 2^-1 = 8; e = 0: just below 16; e = 2; a zero row keeps e = 0; 2^-20 2^23 = 8)
    flat = w.reshape(w.shape[0], -1)
    for i, top in enumerate((16.0, np.nextafter(np.float32(16), np.float32(0)), 32.0)):
        r = flat[first + i]
        r *= np.float32(0.5) / np.abs(r).max()
        r[(3 * i + 1) % r.size] = top
    flat[first + 3] = 0.0
    flat[first + 4] *= np.float32(2.0 ** -21) / np.abs(flat[first + 4]).max()
    flat[first + 4, 2] = 2.0 ** -20
    return [1, 0, 2, 0, -23]


def scale_exponents(w):
    """e of ftmi_split_weights_f16 per row: 8 <= max|w[n]| 2^-e < 16 (e >= -100; a zero row:
    e = 0)."""
    m = np.abs(w.reshape(w.shape[0], -1)).max(1).astype(np.float64)
    ex = np.where(m > 0, np.frexp(m)[1], 4)
    return np.maximum(ex - 4, -100)


def read_colscale(blob, N, K):
    """colscale[N] of a split_weights_f16 block (uint8 array: f16 planes [3][N][Kpad], then
    float colscale[N]; test_gpu_kernels.py::test_split_weights_f16_layout)."""
    Kp = (K + 31) // 32 * 32
    o = 3 * N * Kp * 2
    return np.ascontiguousarray(blob[o:o + 4 * N]).view(np.float32).astype(np.float64)


def colscale_preconditions(cs, w=None, tile=16, distinct=8):
    """The scales the kernel will read are the ones the pattern asked for (w given), take at
    least `distinct` values, and adjacent columns differ somewhere in every full 16-column
    tile: a test that fell back to uniform scales fails here."""
    cs = np.asarray(cs, np.float64)
    if w is not None:
        np.testing.assert_array_equal(cs, np.ldexp(1.0, scale_exponents(w) - 11))
    assert len(np.unique(cs)) >= distinct, np.unique(cs)
    for t in range(len(cs) // tile):
        c = cs[t * tile:(t + 1) * tile]
        assert np.any(c[1:] != c[:-1]), f'uniform scales in column tile {t}'


# ---------------------------------------------------------------- f16x3 GEMM emulation
def _split(v):
    """fp32 -> (f16 head, f16 scaled tail), as split2h / split_weights_f16_kernel."""
    v = v.astype(np.float32)
    h = v.astype(np.float16)
    t = ((v - h.astype(np.float32)) * TS).astype(np.float16)
    return h, t


def split_weights_emu(w):
    """(head, tail) float32 planes of the column-scaled rows and colscale of w (N, K)."""
    e = scale_exponents(w)
    h, t = _split(np.ldexp(w.astype(np.float32), -e[:, None]))
    return h.astype(np.float32), t.astype(np.float32), np.ldexp(1.0, e - 11).astype(np.float32)


def gemm_emu(x, w, colscale=None, kstep=32):
    """x (M, K) @ w (N, K)^T on the f16x3 arithmetic: activations split per element, weight
    planes (2^11 h, t, h), one fp32 accumulator over 32-wide k-steps (the three products of a
    step are exact in fp32; the running sum rounds), colscale in the epilogue.  colscale: an
    override (the negative controls)."""
    wh, wt, cs = split_weights_emu(w)
    if colscale is not None:
        cs = np.asarray(colscale, np.float32)
    xh, xt = (a.astype(np.float32) for a in _split(x))
    acc = np.zeros((x.shape[0], w.shape[0]), np.float32)
    for k0 in range(0, x.shape[1], kstep):
        s = slice(k0, k0 + kstep)
        step = (xh[:, s].astype(np.float64) @ (wh[:, s].T.astype(np.float64) * 2048.0)
                + xh[:, s].astype(np.float64) @ wt[:, s].T.astype(np.float64)
                + xt[:, s].astype(np.float64) @ wh[:, s].T.astype(np.float64))
        acc = (acc.astype(np.float64) + step).astype(np.float32)
    return acc * cs[None, :]


# ---------------------------------------------------------------- attention inputs
PROFILES = ('ramp', 'saw', 'peak', 'offset', 'descend')
PEAK_KEY = 2 * AH_KT + 14  # a key of the third tile (not one the every-third-key mask kills)


def profile(name, T):
    j = np.arange(T, dtype=np.float64)
    if name == 'ramp':
        return 50.0 * j / max(T - 1, 1)
    if name == 'descend':
        return 50.0 * (1.0 - j / max(T - 1, 1))
    if name == 'saw':
        return (j % 64) / 64 * 20 + 9 * (j // 64)
    if name == 'offset':
        return np.full(T, 60.0)
    if name == 'peak':
        c = np.zeros(T)
        c[min(PEAK_KEY, T - 1)] = 30.0
        return c
    raise ValueError(name)


def query_gain(pattern, T):
    """a_i: 'one', or 'mixed' (sign alternating per query, magnitude (1 + i mod 5) / 5: the
    queries of one 16-query wave disagree on whether they move the max)."""
    i = np.arange(T)
    if pattern == 'one':
        return np.ones(T)
    return np.where(i % 2, -1.0, 1.0) * (1 + i % 5) / 5


def attention_inputs(prof, pattern, T, hd, B=2, H=2, seed=0):
    """qkv (B, T, 3 H hd) fp32 whose reference score of query i on key j is a_i c_j + noise:
    q_i = a_i sqrt(hd) u + eps, k_j = c_j u + eps' (u: one random unit vector per head)."""
    rng = np.random.RandomState(seed)
    d = H * hd
    u = rng.randn(H, hd)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    a, c = query_gain(pattern, T), profile(prof, T)
    q = a[None, :, None, None] * np.sqrt(hd) * u[None, None] + rng.randn(B, T, H, hd)
    k = c[None, :, None, None] * u[None, None] + rng.randn(B, T, H, hd)
    v = rng.randn(B, T, H, hd)
    return np.concatenate([t.reshape(B, T, d) for t in (q, k, v)], -1).astype(np.float32)


MASKS = ('none', 'suffix', 'prefix70', 'third', 'item')


def attention_mask(kind, B, T):
    """key_padding_mask (B, T) bool, True = dead; None for 'none'.  'item': batch item 0 fully
    masked (NaN rows there)."""
    if kind == 'none':
        return None
    m = np.zeros((B, T), bool)
    if kind == 'suffix':
        m[0, T - T // 3:] = True
        m[1, T // 2:] = True
    elif kind == 'prefix70':
        m[:, :min(70, T - 1)] = True
    elif kind == 'third':
        m[:, ::3] = True
    elif kind == 'item':
        m[0] = True
    else:
        raise ValueError(kind)
    return m


def _heads(qkv, H):
    B, T, d3 = qkv.shape
    d = d3 // 3
    sp = lambda t: t.reshape(B, T, H, d // H).transpose(0, 2, 1, 3)  # noqa: E731
    return sp(qkv[..., :d]), sp(qkv[..., d:2 * d]), sp(qkv[..., 2 * d:])


def attention_scores(qkv, H, mask=None, dt=np.float64):
    """(B, H, T, T) scores (q sqrt(1 / hd), in fp32 like the kernels and the reference) k^T,
    dead keys -inf."""
    q, k, _ = _heads(qkv, H)
    hd = q.shape[-1]
    s = (q * np.float32(np.sqrt(1.0 / hd))).astype(dt) @ k.astype(dt).transpose(0, 1, 3, 2)
    if mask is not None:
        s = np.where(mask[:, None, None, :], np.array(-np.inf, dt), s)
    return s


def attention_ref(qkv, H, mask=None, dt=np.float64):
    """softmax(scores) v in dtype dt -> (B, T, H hd); a fully masked item gives NaN rows."""
    s = attention_scores(qkv, H, mask, dt)
    _, _, v = _heads(qkv, H)
    with np.errstate(invalid='ignore'):
        e = np.exp(s - s.max(-1, keepdims=True))
        p = e / e.sum(-1, keepdims=True)
        o = p @ v.astype(dt)
    B, _, T, hd = o.shape
    return o.transpose(0, 2, 1, 3).reshape(B, T, H * hd)


def lazy_replay(s):
    """Replay the kernels' lazy running max on scores s (..., T queries, T keys; -inf dead).
    Returns (moves: (..., T) moves of the max after the query's first live tile,
             up: (..., T, tiles) whether the query moved the max on that tile)."""
    T = s.shape[-1]
    m = np.full(s.shape[:-1], -np.inf)
    ups = []
    for k0 in range(0, T, AH_KT):
        mx = s[..., k0:k0 + AH_KT].max(-1)
        up = mx > m + AH_LAZY
        m = np.where(up, mx, m)
        ups.append(up)
    up = np.stack(ups, -1)
    live = np.cumsum(up, -1) > 0
    first = live & ~np.concatenate([np.zeros_like(live[..., :1]), live[..., :-1]], -1)
    return (up & ~first).sum(-1), up


def mixed_wave_tiles(up):
    """Number of (16-query wave, tile) pairs in which some queries move the max and others do
    not, on a tile that is not the first (up: (..., T, tiles) of lazy_replay)."""
    T = up.shape[-2]
    n = 0
    for q0 in range(0, T, 16):
        w = up[..., q0:q0 + 16, 1:]
        n += int(np.sum(w.any(-2) & ~w.all(-2)))
    return n


# ---------------------------------------------------------------- f16x3 attention emulation
def _mm3(big, sm, ah, at, bh, bt, kstep=32):
    """big += ah bh, sm += at bh + ah bt as the MFMAs do it: k-steps of 32 (products exact, the
    step's sum in float64), the fp32 accumulators rounded once per step."""
    ah, at, bh, bt = (a.astype(np.float64) for a in (ah, at, bh, bt))
    for k0 in range(0, ah.shape[-1], kstep):
        s = slice(k0, k0 + kstep)
        big = (big + ah[..., s] @ bh[..., s, :]).astype(np.float32)
        sm = (sm + at[..., s] @ bh[..., s, :]).astype(np.float32)
        sm = (sm + ah[..., s] @ bt[..., s, :]).astype(np.float32)
    return big, sm


def attention_emu(qkv, H, mask=None, skip_osm_rescale=False, neighbour_alpha=False):
    """The t3 / h3 kernels' arithmetic: S on the f16x3 split (big + 2^-11 small), the lazy
    running max, P = exp2(fma(s, log2 e, -m log2 e)) in fp32, P split into f16 head / tail,
    O += P V with separate big / small accumulators, both rescaled by alpha on a move.
    skip_osm_rescale / neighbour_alpha plant the defects of the negative controls (the small
    accumulator left unscaled; query i scaled by query i xor 1's alpha)."""
    q, k, v = _heads(qkv, H)
    B, _, T, hd = q.shape
    qh, qt = _split(q * np.float32(np.sqrt(1.0 / hd)))
    kh, kt = _split(k)
    vh, vt = _split(v)
    ob = np.zeros((B, H, T, hd), np.float32)
    osm = np.zeros_like(ob)
    m = np.full((B, H, T), -np.inf, np.float32)
    l = np.zeros((B, H, T), np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        for k0 in range(0, T, AH_KT):
            ks = slice(k0, k0 + AH_KT)
            z = np.zeros((B, H, T, kh[:, :, ks].shape[2]), np.float32)
            big, sm = _mm3(z, z, qh, qt, kh[:, :, ks].transpose(0, 1, 3, 2),
                           kt[:, :, ks].transpose(0, 1, 3, 2))
            s = big + sm / TS
            if mask is not None:
                s = np.where(mask[:, None, None, ks], np.float32(-np.inf), s)
            mx = s.max(-1)
            up = mx > m + np.float32(AH_LAZY)
            mn = np.where(up, mx, m)
            alpha = np.where(up, np.exp2(((m - mn) * LOG2E).astype(np.float32)), np.float32(1))
            alpha = np.where(np.isnan(alpha), np.float32(0), alpha).astype(np.float32)
            off = np.where(np.isinf(mn), np.float32(0), -mn * LOG2E).astype(np.float32)
            arg = (s.astype(np.float64) * np.float64(LOG2E) + off[..., None]).astype(np.float32)
            p = np.exp2(arg).astype(np.float32)
            l = (l * alpha + p.sum(-1, dtype=np.float32)).astype(np.float32)
            m = mn
            al = alpha
            if neighbour_alpha:
                idx = np.minimum(np.arange(T) ^ 1, T - 1)
                al = alpha[..., idx]
            ob = (ob * al[..., None]).astype(np.float32)
            if not skip_osm_rescale:
                osm = (osm * al[..., None]).astype(np.float32)
            ph, pt = _split(p)
            ob, osm = _mm3(ob, osm, ph, pt, vh[:, :, ks], vt[:, :, ks])
        o = (ob + osm / TS) / l[..., None]
    return o.transpose(0, 2, 1, 3).reshape(B, T, H * hd)


def attention_bound(ref64, ref32, qkv, F=ATTN_F):
    """Bound B of one case: (F * E32 + floor, E32) over the finite rows of the reference."""
    ok = np.isfinite(ref64)
    e32 = float(np.abs(ref32.astype(np.float64) - ref64)[ok].max())
    d = qkv.shape[-1] // 3
    return F * e32 + ATTN_FLOOR * float(np.abs(qkv[..., 2 * d:]).max()), e32


# the B cases: (profile, gain pattern, T, hd, mask).  Every profile runs at one T that is a
# multiple of the 64-key tile and one that is not; T = 64 (one full tile, no tail) is covered;
# every mask kind appears; hd 64 and 128 both see moves.  ramp / saw with a_i = 1 run at
# T >= 192 (two moves after the first live tile need three live tiles); the mixed gain runs
# where a later tile can split a wave (not on `offset`, whose scores are flat along the keys).
ATTN_CASES = [
    ('ramp', 'one', 192, 64, 'none'), ('ramp', 'one', 257, 128, 'third'),
    ('ramp', 'mixed', 200, 128, 'suffix'),
    ('saw', 'one', 192, 128, 'none'), ('saw', 'one', 257, 64, 'prefix70'),
    ('saw', 'mixed', 200, 64, 'item'),
    ('peak', 'one', 192, 128, 'third'), ('peak', 'mixed', 200, 64, 'none'),
    ('offset', 'one', 64, 64, 'none'), ('offset', 'one', 257, 128, 'prefix70'),
    ('offset', 'one', 64, 128, 'item'),
    ('descend', 'one', 128, 64, 'suffix'), ('descend', 'mixed', 200, 128, 'none'),
    ('descend', 'mixed', 128, 128, 'third'),
]


def attention_case(prof, pattern, T, hd, mask_kind, B=2, H=2):
    """(qkv, mask, ref64, ref32) of one B case, seeded by its parameters."""
    seed = 1000 * PROFILES.index(prof) + T + hd + (7 if pattern == 'mixed' else 0)
    qkv = attention_inputs(prof, pattern, T, hd, B, H, seed)
    mask = attention_mask(mask_kind, B, T)
    return (qkv, mask, attention_ref(qkv, H, mask, np.float64),
            attention_ref(qkv, H, mask, np.float32))


def attention_preconditions(prof, pattern, qkv, mask, H):
    """A case that does not exercise the rescale path cannot pass vacuously: ramp / saw (with
    a_i = 1: under the mixed gain half the queries see a falling profile) move the max at least
    twice after the first live tile on a quarter of the live queries; the mixed pattern has a
    (wave, tile past the first) with moving and non-moving queries.  Returns the move count."""
    s = attention_scores(qkv, H, mask)
    moves, up = lazy_replay(s)
    live = np.isfinite(s).any(-1)
    if prof in ('ramp', 'saw') and pattern == 'one':
        assert np.mean(moves[live] >= 2) >= 0.25, float(np.mean(moves[live] >= 2))
    if pattern == 'mixed':
        assert mixed_wave_tiles(up) >= 1
    return int(moves.sum())


# ---------------------------------------------------------------- rescaled checkpoints
# Power-of-two rescalings of a state dict ({key: np.ndarray}, changed in place) that leave
# the network's function unchanged (exactly, but for eps next to a scaled running_var) while
# the rows of its GEMM weights take the `rows` pattern — so activations keep their range, the
# conditioning of the accuracy tests is kept, and every f16x3 consumer reads varied scales.
def _pow2(j):
    return np.ldexp(np.float32(1), np.asarray(j)).astype(np.float32)


def rescale_bn_conv(sd, pre, group=0, lo=-3, hi=12):
    """BatchNormConv `pre` (conv -> [ReLU] -> BatchNorm): conv row n by 2^j, running_mean by
    2^j, running_var by 4^j (ReLU commutes with a positive scale)."""
    s = _pow2(rows_exponents(sd[pre + '.conv.weight'].shape[0], group, lo, hi))
    sd[pre + '.conv.weight'] = sd[pre + '.conv.weight'] * s[:, None, None]
    sd[pre + '.bnorm.running_mean'] = sd[pre + '.bnorm.running_mean'] * s
    sd[pre + '.bnorm.running_var'] = sd[pre + '.bnorm.running_var'] * s * s


def rescale_cbhg_tail(sd, pre, n_highways, lo=-3, hi=8):
    """Channel n of the highway stream carries 2^j: pre_highway rows and W1 rows / biases by
    s_n, every consumer's columns (W1, W2, the GRU's weight_ih) by 1 / s_c."""
    s = _pow2(rows_exponents(sd[pre + '.pre_highway.weight'].shape[0], 0, lo, hi))
    sd[pre + '.pre_highway.weight'] = sd[pre + '.pre_highway.weight'] * s[:, None]
    for i in range(n_highways):
        p = f'{pre}.highways.{i}.'
        sd[p + 'W1.weight'] = sd[p + 'W1.weight'] * s[:, None] / s[None, :]
        sd[p + 'W1.bias'] = sd[p + 'W1.bias'] * s
        sd[p + 'W2.weight'] = sd[p + 'W2.weight'] / s[None, :]
    for sfx in ('', '_reverse'):
        sd[f'{pre}.rnn.weight_ih_l0{sfx}'] = sd[f'{pre}.rnn.weight_ih_l0{sfx}'] / s[None, :]


def rescale_forward_tacotron(sd):
    """The bank convs, both CBHG projections, the SeriesPredictor convs (BatchNorm-followed)
    and the CBHG tails (pre_highway, W1 | W2, the GRU's weight_ih) function-preserving; the
    LSTM's weight_ih rows and `lin` rows by 2^0 .. 2^2 outright (a different, equally valid
    network: the fp64 truth runs on the same state dict)."""
    for net in ('prenet', 'postnet'):
        K = sum(1 for k in sd if k.startswith(net + '.conv1d_bank.') and k.endswith('conv.weight'))
        for g in range(K):
            rescale_bn_conv(sd, f'{net}.conv1d_bank.{g}', group=g)
        rescale_bn_conv(sd, f'{net}.conv_project1')
        rescale_bn_conv(sd, f'{net}.conv_project2', group=3)
        L = sum(1 for k in sd if k.startswith(net + '.highways.') and k.endswith('W1.weight'))
        rescale_cbhg_tail(sd, net, L)
    for p in ('dur_pred', 'pitch_pred', 'energy_pred'):
        for i in range(3):
            rescale_bn_conv(sd, f'{p}.convs.{i}', group=i)
    for sfx in ('', '_reverse'):
        k = f'lstm.weight_ih_l0{sfx}'
        sd[k] = sd[k] * _pow2(rows_exponents(sd[k].shape[0], 0, 0, 2))[:, None]
    s = _pow2(rows_exponents(sd['lin.weight'].shape[0], 0, 0, 2))
    sd['lin.weight'] = sd['lin.weight'] * s[:, None]
    sd['lin.bias'] = sd['lin.bias'] * s
    return sd


def rescale_fft_block(sd, pre, lo=-3, hi=6):
    """FFTBlock `pre` (ending in '.'): q row i by s_i and k row i by 1 / s_i (q k^T unchanged),
    v row i by t_i and out_proj column i by 1 / t_i; conv1 row n (+ bias) by r_n and conv2's
    input channel n by 1 / r_n (ReLU between them)."""
    w = sd[pre + 'self_attn.in_proj_weight']
    d = w.shape[1]
    s = _pow2(rows_exponents(d, 0, lo, hi))
    t = _pow2(rows_exponents(d, 2, lo, hi))
    f = np.concatenate([s, 1 / s, t]).astype(np.float32)
    sd[pre + 'self_attn.in_proj_weight'] = w * f[:, None]
    sd[pre + 'self_attn.in_proj_bias'] = sd[pre + 'self_attn.in_proj_bias'] * f
    sd[pre + 'self_attn.out_proj.weight'] = sd[pre + 'self_attn.out_proj.weight'] / t[None, :]
    r = _pow2(rows_exponents(sd[pre + 'conv1.weight'].shape[0], 1, lo, hi + 4))
    sd[pre + 'conv1.weight'] = sd[pre + 'conv1.weight'] * r[:, None, None]
    sd[pre + 'conv1.bias'] = sd[pre + 'conv1.bias'] * r
    sd[pre + 'conv2.weight'] = sd[pre + 'conv2.weight'] / r[None, :, None]


def rescale_fast_pitch(sd):
    """Every FFT block of FastPitch (the three predictors' transformers, prenet, postnet),
    function-preserving."""
    pres = sorted({k[:-len('self_attn.in_proj_weight')] for k in sd
                   if k.endswith('self_attn.in_proj_weight')})
    for p in pres:
        rescale_fft_block(sd, p)
    return sd
