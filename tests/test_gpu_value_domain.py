"""The f16x3 kernels beyond unit-scale weights and flat attention scores.

Every other GPU parity test draws x ~ N(0, 1) and w ~ N(0, 1 / sqrt(fan_in)): there the
per-output-channel weight scale of ftmi_split_weights_f16 is nearly uniform and the lazy
running max of the f16x3 attention kernels never moves after the first tile.  Here

A. every consumer of `colscale` runs on weights whose scale differs between neighbouring
   columns, 16-column tiles and bank groups (tests/f16x3_emu.py: `rows`, `outlier`, boundary
   rows), against the float64 oracle under bound A — per output column,
   |err| <= ATOL rms(ref[:, n]) + RTOL |ref[:, n]| with the suite's ATOL = RTOL (2e-5; 5e-5
   banks; 1e-5 panel_proj) and no max(1, .) floor.  Each test first reads colscale back from
   the split block and asserts it varies as intended.
B. attention runs on scores a_i c_j + noise with ramps, saw teeth, a peak, a common offset of
   60 and a falling profile, full / suffix / prefix / every-third-key / whole-item masks and
   T = 64 .. 257, each case first replaying the lazy rule on the host to show the rescale path
   runs; bound B: max|err| <= F E32 + 2e-6 max|v| with E32 the error of the same formula in
   float32 on the host (F: f16x3_emu.ATTN_F).  The measured ratios go to attention_range.json
   beside test_gpu_accuracy.py's records (table in DESIGN.md section 6).
C. whole models on rescaled checkpoints (status 0: the f16x3 path is the one that ran).
D. LayerNorm at the widths, row counts, strides and offsets the FastPitch test leaves out.

Where a layer follows the GEMM (the highways), the bound is bound A on the pre-activations
carried through the layer's exact Lipschitz factors (`_highway_bound`): a gate pre-activation
scaled by 2^13 makes sigma'(z) (relu(z1) - x) large next to z = 0, and no kernel — nor plain
fp32 — meets bound A on the output there.

The CPU side (tests/test_value_domain_emu.py) shows on numpy emulations that these bounds
have headroom over the f16x3 arithmetic and that the defects aimed at (a neighbour's column
scale, unreversed group order, a skipped rescale of the small accumulator, a neighbour's
alpha) break them."""
import json

import numpy as np
import pytest
import torch

import f16x3_emu as E
from oracle import fp_oracle as FP
from oracle import ft_oracle as O
from test_gpu_kernels import dev, gemm_cases, host, split_rows_host, use_kernel

pytestmark = pytest.mark.gpu

RTOL = ATOL = 2e-5          # test_gpu_kernels.py
BANK_TOL = 5e-5             # test_conv_bank
PANEL_TOL = 1e-5            # test_panel_proj
EPS32 = 2.0 ** -24


@pytest.fixture
def rng():
    return np.random.Generator(np.random.PCG64(4321))


def _status():
    from forwardtacotron_amd import ops
    st = ops.status_word('cuda')
    st.zero_()
    return st


def within_a(got, ref, tol=ATOL, what=''):
    """Bound A over the last axis' columns."""
    N = ref.shape[-1]
    r = E.worst_ratio_a(np.asarray(got).reshape(-1, N), np.asarray(ref, np.float64).reshape(-1, N),
                        tol, tol)
    print(f'{what} worst |err| / bound A = {r:.3f}')
    assert r <= 1.0, (what, r)


def pattern_weight(rng, pattern, shape, group=0, lo=-3, hi=13):
    """w0 ~ N(0, 1 / sqrt(fan_in)) under one of the A patterns; shape (N, ...)."""
    fan_in = int(np.prod(shape[1:]))
    w0 = rng.normal(0, 1 / np.sqrt(fan_in), shape).astype(np.float32)
    if pattern == 'rows':
        return E.rows_pattern(w0, group, lo, hi)
    if pattern == 'outlier':
        return E.outlier_pattern(w0, group)
    raise ValueError(pattern)


def check_block(blob, w_packed, distinct=8):
    """The preconditions on the colscale the kernels will read (from the split block)."""
    N, K = w_packed.shape
    cs = E.read_colscale(host(blob), N, K)
    E.colscale_preconditions(cs, host(w_packed) if torch.is_tensor(w_packed) else w_packed,
                             distinct=distinct)
    return cs


# ================================================================ A. conv1d
CONV_SHAPES = [(1, 7, 16, 40, 4), (3, 301, 96, 200, 7), (1, 40, 416, 64, 3), (2, 60, 1024, 256, 3)]
F16X3 = [p for p in gemm_cases(CONV_SHAPES, rows=lambda s: s[0] * s[1], cols=lambda s: s[3])
         if p.values[5] == 2]


def _conv_setup(rng, pattern, B, T, Cin, N, k):
    from forwardtacotron_amd import ops
    from forwardtacotron_amd.common_layers import pack_conv
    x = rng.normal(0, 1, (B, T, Cin)).astype(np.float32)
    w = pattern_weight(rng, pattern, (N, Cin, k))
    b = (rng.normal(0, 0.1, N) * np.abs(w).reshape(N, -1).max(1)).astype(np.float32)
    sc = rng.uniform(0.5, 1.5, N).astype(np.float32)
    sh = rng.normal(0, 0.1, N).astype(np.float32)
    res = rng.normal(0, 1, (B, T, N)).astype(np.float32)
    f8 = np.float64
    ref = O.conv1d(x.transpose(0, 2, 1).astype(f8), w.astype(f8), k // 2, b.astype(f8))[:, :, :T]
    ref = np.maximum(ref, 0) * sc[None, :, None].astype(f8) + sh[None, :, None] + res.transpose(0, 2, 1)
    wp = pack_conv(torch.from_numpy(w)).cuda()
    w3 = ops.presplit_for(wp, 2)
    check_block(w3, wp)
    return x, wp, w3, b, sc, sh, res, ref.transpose(0, 2, 1)


def _conv_run(x, wp, w3, k, b, sc, sh, res, x_split=False):
    from forwardtacotron_amd import ops
    B, T, _ = x.shape
    yt = torch.empty(B, wp.size(0), T, device='cuda')
    xd = dev(x)
    y, _ = ops.conv1d(ops.split_rows(xd) if x_split else xd, wp, k, k // 2, bias=dev(b), relu=True,
                      bn=(dev(sc), dev(sh)), residual=dev(res), out_t=yt, mma=2, w_split=w3,
                      x_split=x_split)
    return host(y), host(yt)


@pytest.mark.parametrize('pattern', ['rows', 'outlier'])
@pytest.mark.parametrize('B,T,Cin,N,k,mma,pre,kernel', F16X3)
def test_conv1d_column_scales(B, T, Cin, N, k, mma, pre, kernel, pattern, rng, monkeypatch):
    """bias, ReLU, BN, residual and the transposed copy on the tiled, slab and skinny kernels
    (416 channels: the skinny finish over 7 splits)."""
    use_kernel(kernel, monkeypatch)
    x, wp, w3, b, sc, sh, res, ref = _conv_setup(rng, pattern, B, T, Cin, N, k)
    st = _status()
    y, yt = _conv_run(x, wp, w3, k, b, sc, sh, res)
    assert int(st.item()) == 0
    within_a(y, ref, what=f'conv1d {kernel} {pattern}')
    np.testing.assert_array_equal(yt, y.transpose(0, 2, 1))


@pytest.mark.parametrize('kernel', ['tiled', 'slab'])
@pytest.mark.parametrize('pattern', ['rows', 'outlier'])
def test_conv1d_column_scales_split_k(kernel, pattern, rng, monkeypatch):
    """Three split-K partials: the scale belongs after their sum (finish launch)."""
    from forwardtacotron_amd import ops
    use_kernel(kernel, monkeypatch)
    monkeypatch.setattr(ops, '_split_k', lambda *a, **kw: 3)
    B, T, Cin, N, k = CONV_SHAPES[3]
    x, wp, w3, b, sc, sh, res, ref = _conv_setup(rng, pattern, B, T, Cin, N, k)
    st = _status()
    y, yt = _conv_run(x, wp, w3, k, b, sc, sh, res)
    assert int(st.item()) == 0
    within_a(y, ref, what=f'conv1d split-K {kernel} {pattern}')
    np.testing.assert_array_equal(yt, y.transpose(0, 2, 1))


def test_conv1d_column_scales_slab_forms_bit_identical(rng, monkeypatch):
    """FTMI_SLAB_PF = 1 / 0 give the same bits, and so do split rows (x_split) against fp32
    rows, on scaled columns (ragged rows and columns, k = 7)."""
    monkeypatch.setenv('FTMI_GEMM_SKINNY', '0')
    B, T, Cin, N, k = CONV_SHAPES[1]
    x, wp, w3, b, sc, sh, res, ref = _conv_setup(rng, 'rows', B, T, Cin, N, k)
    st = _status()
    outs = {}
    for pf in ('1', '0'):
        monkeypatch.setenv('FTMI_SLAB_PF', pf)
        outs[pf] = _conv_run(x, wp, w3, k, b, sc, sh, res)
        outs[pf + 's'] = _conv_run(x, wp, w3, k, b, sc, sh, res, x_split=True)
    assert int(st.item()) == 0
    within_a(outs['1'][0], ref, what='conv1d slab prefetch')
    for key in ('0', '1s', '0s'):
        for a, c in zip(outs['1'], outs[key]):
            np.testing.assert_array_equal(a.view(np.uint32), c.view(np.uint32))


@pytest.mark.parametrize('B,T,Cin,N,k,mma,pre,kernel',
                         [p for p in F16X3 if p.values[:5] in (CONV_SHAPES[0], CONV_SHAPES[1])])
def test_conv1d_boundary_rows(B, T, Cin, N, k, mma, pre, kernel, rng, monkeypatch):
    """A bare GEMM (nothing added that could hide a small column) with rows of max|w| exactly
    16, just below 16, 32, all zero and 2^-20-sized among `rows`-pattern neighbours: the
    split block holds the expected scales; the zero row's column is exactly zero; every
    column, the 2^-20 one included, meets bound A."""
    from forwardtacotron_amd import ops
    from forwardtacotron_amd.common_layers import pack_conv
    use_kernel(kernel, monkeypatch)
    x = rng.normal(0, 1, (B, T, Cin)).astype(np.float32)
    w = pattern_weight(rng, 'rows', (N, Cin, k))
    want = E.boundary_rows(w, 17)
    wp = pack_conv(torch.from_numpy(w)).cuda()
    w3 = ops.presplit_for(wp, 2)
    cs = check_block(w3, wp)
    np.testing.assert_array_equal(np.log2(cs[17:22]) + 11, want)
    st = _status()
    y, _ = ops.conv1d(dev(x), wp, k, k // 2, mma=2, w_split=w3)
    y = host(y)
    assert int(st.item()) == 0
    f8 = np.float64
    ref = O.conv1d(x.transpose(0, 2, 1).astype(f8), w.astype(f8), k // 2)[:, :, :T].transpose(0, 2, 1)
    assert not y[..., 20].any() and np.abs(y[..., 21]).max() > 0
    within_a(y, ref, what=f'conv1d boundary rows {kernel}')


@pytest.mark.parametrize('B,T,Cin,N,k,mma,pre,kernel', [p for p in F16X3 if p.values[:5] == CONV_SHAPES[0]])
def test_conv1d_range_guard_boundary(B, T, Cin, N, k, mma, pre, kernel, rng, monkeypatch):
    """An activation of exactly 65504 (the largest f16) is in range: status 0 and the result
    within bound A; the next float up sets status bit 0."""
    from forwardtacotron_amd import ops
    from forwardtacotron_amd.common_layers import pack_conv
    use_kernel(kernel, monkeypatch)
    x = rng.normal(0, 1, (B, T, Cin)).astype(np.float32)
    x[0, 3, 5] = 65504.0
    w = pattern_weight(rng, 'rows', (N, Cin, k))
    wp = pack_conv(torch.from_numpy(w)).cuda()
    w3 = ops.presplit_for(wp, 2)
    check_block(w3, wp)
    st = _status()
    y, _ = ops.conv1d(dev(x), wp, k, k // 2, mma=2, w_split=w3)
    y = host(y)
    assert int(st.item()) == 0
    f8 = np.float64
    ref = O.conv1d(x.transpose(0, 2, 1).astype(f8), w.astype(f8), k // 2)[:, :, :T].transpose(0, 2, 1)
    within_a(y, ref, what=f'conv1d x = 65504 {kernel}')
    x[0, 3, 5] = np.nextafter(np.float32(65504), np.float32(np.inf))
    ops.conv1d(dev(x), wp, k, k // 2, mma=2, w_split=w3)
    torch.cuda.synchronize()
    assert int(st.item()) & 1
    st.zero_()


# ================================================================ A. conv bank
def _bank_setup(rng, pattern, K, Cin, B, T, lo=-3, hi=13):
    from forwardtacotron_amd import ops
    from forwardtacotron_amd._lib import load
    from forwardtacotron_amd.common_layers import pack_conv
    C = 256
    x = rng.normal(0, 1, (B, T, Cin)).astype(np.float32)
    ws = [pattern_weight(rng, pattern, (C, Cin, k), group=k - 1, lo=lo, hi=hi) for k in range(1, K + 1)]
    sc = rng.uniform(0.5, 1.5, K * C).astype(np.float32)
    sh = rng.normal(0, 0.1, K * C).astype(np.float32)
    f8 = np.float64
    xt = x.transpose(0, 2, 1).astype(f8)
    refs = [np.maximum(O.conv1d(xt, w.astype(f8), w.shape[2] // 2)[:, :, :T], 0) for w in ws]
    ref = (np.concatenate(refs, 1) * sc[None, :, None].astype(f8) + sh[None, :, None]).transpose(0, 2, 1)
    packed = [pack_conv(torch.from_numpy(w)) for w in ws]
    wp = torch.cat([p.reshape(-1) for p in packed]).cuda()
    w3 = ops.split_bank_weights(wp, K, Cin, C, 2)
    blob, off, css = host(w3), 0, []
    for g, p in enumerate(packed):  # group g's block: planes of [C][(g + 1) Cin], then colscale
        n = int(load().ftmi_split_weights_f16_bytes(C, (g + 1) * Cin))
        cs = E.read_colscale(blob[off:off + n], C, (g + 1) * Cin)
        E.colscale_preconditions(cs, p.numpy())
        css.append(cs)
        off += n
    assert off == blob.size
    for g in range(K - 1):
        assert np.any(css[g] != css[g + 1]), f'bank groups {g}, {g + 1}: the same scales'
    return x, wp, w3, sc, sh, ref


@pytest.mark.parametrize('pattern', ['rows', 'outlier'])
def test_conv_bank_column_scales_slab_and_pool(pattern, rng):
    """The slab bank kernel, plain and pooled (the pooled bank is the maxpool of the plain
    one bit for bit; the plain one meets bound A)."""
    from forwardtacotron_amd import ops
    K, Cin, B, T = 8, 80, 3, 200
    x, wp, w3, sc, sh, ref = _bank_setup(rng, pattern, K, Cin, B, T)
    xd = dev(x)
    assert ops.bank_pools(xd, K, 256, w_split=w3)
    st = _status()
    y = host(ops.conv_bank(xd, wp, K, 256, dev(sc), dev(sh), mma=2, w_split=w3))
    yp = host(ops.conv_bank(xd, wp, K, 256, dev(sc), dev(sh), mma=2, w_split=w3, pool=True))
    assert int(st.item()) == 0
    within_a(y, ref, BANK_TOL, f'bank slab {pattern}')
    np.testing.assert_array_equal(yp, O.maxpool_k2_s1_p1(y.transpose(0, 2, 1)).transpose(0, 2, 1))


@pytest.mark.parametrize('K,Cin,B,T', [(4, 48, 7, 5), (8, 80, 3, 200)])
def test_conv_bank_column_scales_walk(K, Cin, B, T, rng, monkeypatch):
    """The walking bank against the slab kernel's pooled bank, bit for bit, and against the
    oracle's maxpool within the bound of the two rows a pooled value comes from."""
    from forwardtacotron_amd import ops
    x, wp, w3, sc, sh, ref = _bank_setup(rng, 'rows', K, Cin, B, T)
    st = _status()
    out = {}
    for walk in ('1', '0'):
        monkeypatch.setenv('FTMI_BANK_WALK', walk)
        out[walk] = host(ops.conv_bank(dev(x), wp, K, 256, dev(sc), dev(sh), mma=2, w_split=w3,
                                       pool=True))
    assert int(st.item()) == 0
    np.testing.assert_array_equal(out['1'].view(np.uint32), out['0'].view(np.uint32))
    # |max(a, b) - max(a', b')| <= max(|a - a'|, |b - b'|): the larger of the two rows' bounds
    b = E.bound_a(ref.reshape(B * T, -1), BANK_TOL, BANK_TOL).reshape(ref.shape)
    bp = b.copy()
    bp[:, 1:] = np.maximum(b[:, 1:], b[:, :-1])
    refp = O.maxpool_k2_s1_p1(ref.transpose(0, 2, 1)).transpose(0, 2, 1)
    assert np.all(np.abs(out['1'] - refp) <= bp)


@pytest.mark.parametrize('K,Cin,B,T', [(4, 48, 7, 5), (8, 80, 3, 200)])
def test_conv_bank_column_scales_split_out(K, Cin, B, T, rng, monkeypatch):
    """split_out: exponents up to 11 keep every output inside the f16 range (status 0); the
    split rows are the host split of the fp32 pooled output, on both bank kernels."""
    from forwardtacotron_amd import ops
    x, wp, w3, sc, sh, ref = _bank_setup(rng, 'rows', K, Cin, B, T, lo=-3, hi=11)
    assert np.abs(ref).max() < 65504
    st = _status()
    for walk in ('1', '0'):
        monkeypatch.setenv('FTMI_BANK_WALK', walk)
        yp = ops.conv_bank(dev(x), wp, K, 256, dev(sc), dev(sh), mma=2, w_split=w3, pool=True)
        ys = ops.conv_bank(dev(x), wp, K, 256, dev(sc), dev(sh), mma=2, w_split=w3, pool=True,
                           split_out=True)
        np.testing.assert_array_equal(host(ys).view(np.float16), split_rows_host(host(yp)))
    assert int(st.item()) == 0


@pytest.mark.parametrize('schedule', ['halves', 'halves-image', 'pairs', 'groups'])
@pytest.mark.parametrize('K,Cin,B,T', [(4, 64, 1, 50), (8, 128, 1, 128), (8, 80, 1, 100)])
def test_conv_bank_column_scales_schedules(K, Cin, B, T, schedule, rng, monkeypatch):
    """The few-row bank on every block schedule (the halves kernel pairs group g with group
    K - 1 - g and its weight image stores the groups' scales in reversed order; Cin = 80 has
    no halves kernel and falls through, as in test_conv_bank_skinny_schedules)."""
    from forwardtacotron_amd import ops
    monkeypatch.setenv('FTMI_BANK_HALVES', '1' if schedule.startswith('halves') else '0')
    monkeypatch.setenv('FTMI_BANK_BALANCED', '0' if schedule == 'groups' else '1')
    x, wp, w3, sc, sh, ref = _bank_setup(rng, 'rows', K, Cin, B, T)
    assert ops._bank_halves(2, B, T, Cin, K, 256) == (schedule.startswith('halves') and Cin % 64 == 0)
    st = _status()
    y = ops.conv_bank(dev(x), wp, K, 256, dev(sc), dev(sh), mma=2, w_split=w3)
    within_a(host(y), ref, BANK_TOL, f'bank {schedule}')
    if schedule == 'halves-image':
        img = ops.bank_halves_image(w3, K, Cin, 256)
        if Cin % 64 == 0:
            assert img is not None
        if img is not None:
            yi = ops.conv_bank(dev(x), wp, K, 256, dev(sc), dev(sh), mma=2, w_split=w3, w_image=img)
            np.testing.assert_array_equal(host(yi).view(np.uint32), host(y).view(np.uint32))
    assert int(st.item()) == 0


# ================================================================ A. highways
def _sigmoid(z):
    return 0.5 * (1.0 + np.tanh(0.5 * z))


def _highway_bound(h, Bh, w1, b1, w2, b2, tol=ATOL):
    """(ref, bound) of y = g relu(z1) + (1 - g) h, g = sigmoid(z2), z = h W^T + b in float64,
    given |dh| <= Bh on the input.  z carries bound A plus |W| Bh; relu is 1-Lipschitz;
    |dg| <= sup sigma' over the interval around z2, plus the fp32 sigmoid's own rounding
    (exp of an argument rounded at |z2| 2^-23, a division: g (1 - g) (|z2| 2^-22 + 2^-21));
    dy = dg (r - h) + g dr + (1 - g) dh + dg (dr - dh), and three fp32 roundings of the
    epilogue's terms."""
    z1 = h @ w1.T + b1
    z2 = h @ w2.T + b2
    B1 = E.bound_a(z1, tol, tol) + Bh @ np.abs(w1).T
    B2 = E.bound_a(z2, tol, tol) + Bh @ np.abs(w2).T
    g, r = _sigmoid(z2), np.maximum(z1, 0)
    zn = np.maximum(np.abs(z2) - B2, 0)  # the point of the interval nearest 0: largest sigma'
    gn = _sigmoid(zn)
    Bg = gn * (1 - gn) * B2 + g * (1 - g) * (np.abs(z2) * 2.0 ** -22 + 2.0 ** -21)
    y = g * r + (1 - g) * h
    By = (Bg * np.abs(r - h) + g * B1 + (1 - g) * Bh + Bg * (B1 + Bh)
          + 4 * EPS32 * (np.abs(g * r) + np.abs((1 - g) * h) + np.abs(y)))
    return y, By


def _w12(w1, w2):
    """HighwayNetwork._pack's interleave: 32 rows of W1, 32 rows of W2, ..."""
    C = w1.shape[0]
    return np.stack([w1.reshape(C // 32, 32, C), w2.reshape(C // 32, 32, C)], 1).reshape(2 * C, C)


@pytest.mark.parametrize('pattern', ['rows', 'outlier'])
@pytest.mark.parametrize('C,B,T,mma,pre,kernel',
                         [p for p in gemm_cases([(160, 1, 90), (128, 2, 300)]) if p.values[3] == 2])
def test_highway_column_scales(C, B, T, mma, pre, kernel, pattern, rng, monkeypatch):
    from forwardtacotron_amd import ops
    use_kernel(kernel, monkeypatch)
    w1, w2 = (pattern_weight(rng, pattern, (C, C)) for _ in range(2))
    b1, b2 = (rng.normal(0, 0.1, C).astype(np.float32) for _ in range(2))
    x = rng.normal(0, 1, (B, T, C)).astype(np.float32)
    w12 = dev(_w12(w1, w2))
    w3 = ops.presplit_for(w12, 2)
    check_block(w3, w12)
    f8 = np.float64
    ref, bound = _highway_bound(x.reshape(-1, C).astype(f8), np.zeros((B * T, C)), w1.astype(f8),
                                b1.astype(f8), w2.astype(f8), b2.astype(f8))
    st = _status()
    y = host(ops.highway(dev(x), w12, dev(b1), dev(b2), mma=2, w_split=w3)).reshape(-1, C)
    assert int(st.item()) == 0
    ratio = float(np.max(np.abs(y - ref) / bound))
    print(f'highway {kernel} {pattern}: worst |err| / bound = {ratio:.3f}')
    assert ratio <= 1.0


def _stack_weights(rng, Cp, L):
    """pre_highway, L x (W1, b1, W2, b2) and W_ih with scaled rows.  Exponents at or below 2 in
    the layers whose output stays inside the kernel (its f16x3 operand: |h| < 65504, status
    0) — the normalising weight scale makes down-scaled rows as distinct as up-scaled ones —
    and the full `rows` span on W_ih, whose fp32 output has no range limit."""
    C = 256
    pre = pattern_weight(rng, 'rows', (C, Cp), lo=-8, hi=2)
    hws = []
    for _ in range(L):
        w1, w2 = (pattern_weight(rng, 'rows', (C, C), lo=-8, hi=2) for _ in range(2))
        hws.append((w1, rng.normal(0, 0.1, C).astype(np.float32), w2,
                    rng.normal(0, 0.1, C).astype(np.float32)))
    w_ih = pattern_weight(rng, 'rows', (6 * C, C))
    b_in = rng.normal(0, 0.1, 6 * C).astype(np.float32)
    return pre, hws, w_ih, b_in


def _stack_blocks(pre, hws, w_ih):
    from forwardtacotron_amd import ops
    f16 = lambda w: ops.split_weights_f16(dev(w), frag=True)  # noqa: E731
    blocks = (f16(pre), [f16(_w12(h[0], h[2])) for h in hws], f16(w_ih))
    check_block(blocks[0], pre)
    for blk, h in zip(blocks[1], hws):
        check_block(blk, _w12(h[0], h[2]))
    check_block(blocks[2], w_ih)
    return blocks


def _stack_prefix(xd, blocks, hws, w_ih, b_in, layers):
    from forwardtacotron_amd import ops
    pre_f, hw_f, ih_f = blocks
    b1s = [dev(h[1]) for h in hws[:layers]]
    b2s = [dev(h[3]) for h in hws[:layers]]
    return ops.highway_stack(xd, pre_f, 256, hw_f[:layers], b1s, b2s, ih_f, dev(b_in),
                             w_ih.shape[0], want_h=True)


def _check_stack(x, pre, hws, w_ih, b_in, blocks, what):
    """Layer by layer against float64: h_l of the stack run with l layers (always with the
    projection: the forms the suite already runs) is the input the run with l + 1 layers
    multiplies (the same arithmetic, h kept as f16x3 head + tail: 2^-21 relative), so each
    layer's reference starts from the GPU's own h_l and carries one layer's bound — sharp for
    every layer's column scales, no compounding; the projection is checked on the full run."""
    f8 = np.float64
    xd = dev(x)
    M = x.shape[0] * x.shape[1]
    L = len(hws)
    y, h = _stack_prefix(xd, blocks, hws, w_ih, b_in, 0)
    h = host(h).reshape(M, 256)
    within_a(h, x.reshape(M, -1).astype(f8) @ pre.astype(f8).T, what=f'{what} pre_highway')
    for l in range(L):
        y, hn = _stack_prefix(xd, blocks, hws, w_ih, b_in, l + 1)
        hn = host(hn).reshape(M, 256)
        w1, b1, w2, b2 = (a.astype(f8) for a in hws[l])
        ref, bound = _highway_bound(h.astype(f8), np.abs(h) * 2.0 ** -21, w1, b1, w2, b2)
        ratio = float(np.max(np.abs(hn - ref) / bound))
        print(f'{what} highway {l}: worst |err| / bound = {ratio:.3f}')
        assert ratio <= 1.0, (what, l, ratio)
        h = hn
    refy = h.astype(f8) @ w_ih.astype(f8).T + b_in
    By = E.bound_a(refy, ATOL, ATOL) + (np.abs(h) * 2.0 ** -21) @ np.abs(w_ih).T.astype(f8)
    ratio = float(np.max(np.abs(host(y).reshape(M, -1) - refy) / By))
    print(f'{what} W_ih: worst |err| / bound = {ratio:.3f}')
    assert ratio <= 1.0, (what, ratio)
    return host(y), h


@pytest.mark.parametrize('B,T,Cp,L', [(3, 77, 256, 4), (3, 333, 80, 4)])
def test_highway_stack_column_scales(B, T, Cp, L, rng, monkeypatch):
    """ftmi_highway_stack (cs_pre, cs_hw[l], cs_out) on scaled rows in the pre-projection, each
    highway's W1 | W2 and W_ih; status 0; on the second shape the 96-row form gives the
    64-row form's bits."""
    monkeypatch.setenv('FTMI_HS_SPREAD', '0')
    pre, hws, w_ih, b_in = _stack_weights(rng, Cp, L)
    blocks = _stack_blocks(pre, hws, w_ih)
    x = rng.normal(0, 1, (B, T, Cp)).astype(np.float32)
    st = _status()
    y, h = _check_stack(x, pre, hws, w_ih, b_in, blocks, f'stack {B}x{T}')
    assert int(st.item()) == 0
    if T == 333:
        for bm in ('96', '64'):
            monkeypatch.setenv('FTMI_HS_BM', bm)
            y2, h2 = _stack_prefix(dev(x), blocks, hws, w_ih, b_in, L)
            np.testing.assert_array_equal(host(y2).view(np.uint32), y.view(np.uint32))
            np.testing.assert_array_equal(host(h2).reshape(-1, 256).view(np.uint32), h.view(np.uint32))
        assert int(st.item()) == 0


@pytest.mark.parametrize('B,T,Cp,L', [(1, 50, 80, 2), (3, 43, 80, 0)])
def test_highway_stack_spread_column_scales(B, T, Cp, L, rng, monkeypatch):
    """The spread form: the oracle check layer by layer, and FTMI_HS_SPREAD = 1 / 0 bit for
    bit."""
    from forwardtacotron_amd import ops
    pre, hws, w_ih, b_in = _stack_weights(rng, Cp, L)
    blocks = _stack_blocks(pre, hws, w_ih)
    x = rng.normal(0, 1, (B, T, Cp)).astype(np.float32)
    assert ops.hs_spread_blocks(B * T, w_ih.shape[0]) == -(-B * T // 64) * 16
    st = _status()
    monkeypatch.setenv('FTMI_HS_SPREAD', '1')
    y, h = _check_stack(x, pre, hws, w_ih, b_in, blocks, f'spread {B}x{T}')
    monkeypatch.setenv('FTMI_HS_SPREAD', '0')
    y0, h0 = _stack_prefix(dev(x), blocks, hws, w_ih, b_in, L)
    np.testing.assert_array_equal(host(y0).view(np.uint32), y.view(np.uint32))
    np.testing.assert_array_equal(host(h0).reshape(-1, 256).view(np.uint32), h.view(np.uint32))
    assert int(st.item()) == 0


# ================================================================ A. panel_proj
def _ln64(z, g, bt, eps=1e-5):
    mu = z.mean(-1, keepdims=True)
    return (z - mu) / np.sqrt(((z - mu) ** 2).mean(-1, keepdims=True) + eps) * g + bt


@pytest.mark.parametrize('B,T,K,N,ln', [(2, 333, 96, 512, False), (1, 37, 256, 256, False),
                                        (1, 37, 256, 256, True)])
def test_panel_proj_column_scales(B, T, K, N, ln, rng):
    """ftmi_panel_proj with bias and residual: the full `rows` span without LayerNorm;
    exponents 0 .. 3 under LayerNorm (the row's variance is the large columns', and bound A
    is per column: f16x3_emu / test_value_domain_emu verify it at this span)."""
    from forwardtacotron_amd import ops
    x = rng.normal(0, 1, (B, T, K)).astype(np.float32)
    w = pattern_weight(rng, 'rows', (N, K), lo=0, hi=3) if ln else pattern_weight(rng, 'rows', (N, K))
    b = rng.normal(0, 0.1, N).astype(np.float32)
    r = rng.normal(0, 1, (B, T, N)).astype(np.float32)
    g = rng.normal(1, 0.2, N).astype(np.float32)
    bt = rng.normal(0, 0.2, N).astype(np.float32)
    wf = ops.split_weights_f16(dev(w), frag=True)
    check_block(wf, w, distinct=4 if ln else 8)
    st = _status()
    y = ops.panel_proj(dev(x), wf, N, bias=dev(b), residual=dev(r),
                       ln=(dev(g), dev(bt), 1e-5) if ln else None)
    f8 = np.float64
    ref = x.reshape(-1, K).astype(f8) @ w.astype(f8).T + b + r.reshape(-1, N)
    if ln:
        ref = _ln64(ref, g.astype(f8), bt.astype(f8))
    within_a(host(y), ref, PANEL_TOL, f'panel_proj ln={ln}')
    assert int(st.item()) == 0


def test_panel_proj_qkv_column_scales(rng):
    """ftmi_panel_proj_qkv + ftmi_attention_kv against ftmi_panel_proj + ftmi_attention, bit
    for bit, with in_proj rows scaled by 2^-8 .. 2^2 (q, k, v stay inside the f16 range: status
    0); the projected rows against the float64 oracle."""
    from forwardtacotron_amd import ops
    B, T, H, d = 2, 451, 4, 256
    x = rng.normal(0, 1, (B, T, d)).astype(np.float32)
    w = pattern_weight(rng, 'rows', (3 * d, d), lo=-8, hi=2)
    b = rng.normal(0, 0.1, 3 * d).astype(np.float32)
    mask = torch.arange(T)[None, :] >= torch.tensor([T, 300])[:, None]
    wf = ops.split_weights_f16(dev(w), frag=True)
    check_block(wf, w)
    st = _status()
    qkv = ops.panel_proj(dev(x), wf, 3 * d, bias=dev(b))
    ref = ops.attention(qkv, H, mask.cuda(), mma=2, presplit=True)
    q, kv = ops.panel_proj_qkv(dev(x), wf, d, H, bias=dev(b))
    got = ops.attention_kv(q, kv, H, mask.cuda())
    torch.cuda.synchronize()
    assert int(st.item()) == 0
    assert torch.equal(q, qkv[:, :, :d]) and torch.equal(got, ref)
    f8 = np.float64
    within_a(host(qkv), x.reshape(-1, d).astype(f8) @ w.astype(f8).T + b, PANEL_TOL, 'in_proj')


# ================================================================ B. attention
_ATTN = {}


def _attn_case(case):
    """One B case, computed once: inputs, references, bound, preconditions."""
    if case not in _ATTN:
        qkv, mask, r64, r32 = E.attention_case(*case)
        moves = E.attention_preconditions(case[0], case[1], qkv, mask, 2)
        bound, e32 = E.attention_bound(r64, r32, qkv)
        _ATTN[case] = dict(qkv=qkv, mask=mask, r64=r64, bound=bound, e32=e32, moves=moves)
    return _ATTN[case]


_TABLE = {}


def _record_attention(key, entry):
    """Every case's measured ratios, rewritten as one table (attention_range.json) beside the
    accuracy records of test_gpu_accuracy.py."""
    from test_gpu_accuracy import _record
    _TABLE[key] = entry
    print(key, json.dumps(entry))
    _record('attention_range', dict(sorted(_TABLE.items())), fname='attention_range.json')


def _attn_err(got, r64):
    """max |got - ref| over the reference's finite rows; NaN exactly where it has NaN (a fully
    masked item)."""
    ok = np.isfinite(r64)
    np.testing.assert_array_equal(np.isnan(got), ~ok)
    return float(np.abs(got - r64)[ok].max())


@pytest.mark.parametrize('prof,pattern,T,hd,mask_kind', E.ATTN_CASES,
                         ids=['-'.join(str(v) for v in c) for c in E.ATTN_CASES])
def test_attention_score_range(prof, pattern, T, hd, mask_kind, monkeypatch):
    """Every attention kernel against the float64 reference under bound B: fp32 MFMA, t3 with
    the split pass and with the in-kernel split (bit-identical), h3 in both forms
    (bit-identical; within E32 of t3); status 0; NaN rows exactly for a fully masked item."""
    from forwardtacotron_amd import ops
    c = _attn_case((prof, pattern, T, hd, mask_kind))
    qkv, r64, bound, e32 = dev(c['qkv']), c['r64'], c['bound'], c['e32']
    mk = dev(c['mask']) if c['mask'] is not None else None
    st = _status()
    run = lambda **kw: host(ops.attention(qkv, 2, mk, **kw))  # noqa: E731
    outs = {'f32': run(mma=0), 't3-presplit': run(mma=2, presplit=True), 't3': run(mma=2, presplit=False)}
    monkeypatch.setenv('FTMI_ATTN_T', '0')
    outs['h3-presplit'] = run(mma=2, presplit=True)
    outs['h3'] = run(mma=2, presplit=False)
    assert int(st.item()) == 0
    errs = {k: _attn_err(v, r64) for k, v in outs.items()}
    ok = np.isfinite(r64)
    t3_h3 = float(np.abs(outs['t3'] - outs['h3'])[ok].max())
    _record_attention(f'{prof}-{pattern}-T{T}-hd{hd}-{mask_kind}',
                      dict(moves=c['moves'], E32=e32, bound=bound, t3_vs_h3=t3_h3,
                           ratio={k: e / e32 for k, e in errs.items()}, err=errs))
    for k, e in errs.items():
        assert e <= bound, (k, e, bound, e32)
    np.testing.assert_array_equal(outs['t3-presplit'], outs['t3'])
    np.testing.assert_array_equal(outs['h3-presplit'], outs['h3'])
    assert t3_h3 <= e32


@pytest.mark.parametrize('prof,pattern,T,hd,mask_kind', [c for c in E.ATTN_CASES if c[3] == 128],
                         ids=['-'.join(str(v) for v in c) for c in E.ATTN_CASES if c[3] == 128])
def test_attention_kv_score_range(prof, pattern, T, hd, mask_kind, rng):
    """panel_proj_qkv + attention_kv (d = 256: the head-dim-128 cases).  in_proj builds the
    case's q = a sqrt(hd) u + eps, k = c u + eps' from rows x = (a, c, noise); the reference
    is the float64 attention of the projected rows the GPU produced, so bound B judges the
    attention alone.  Bit-identical to panel_proj + attention, as test_kv_fused_in_proj has it."""
    from forwardtacotron_amd import ops
    B, H, d = 2, 2, 256
    u = rng.normal(0, 1, (H, hd))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    x = rng.normal(0, 1, (B, T, d)).astype(np.float32)
    x[..., 0] = E.query_gain(pattern, T)
    x[..., 1] = E.profile(prof, T)
    w = rng.normal(0, 1 / np.sqrt(d - 2), (3 * d, d)).astype(np.float32)
    w[:, :2] = 0
    w[:d, 0] = np.sqrt(hd) * u.reshape(-1)
    w[d:2 * d, 1] = u.reshape(-1)
    mask = E.attention_mask(mask_kind, B, T)
    mk = dev(mask) if mask is not None else None
    wf = ops.split_weights_f16(dev(w), frag=True)
    st = _status()
    qkv = ops.panel_proj(dev(x), wf, 3 * d)
    ref_gpu = ops.attention(qkv, H, mk, mma=2, presplit=True)
    q, kv = ops.panel_proj_qkv(dev(x), wf, d, H)
    got = ops.attention_kv(q, kv, H, mk)
    torch.cuda.synchronize()
    assert int(st.item()) == 0
    assert torch.equal(q, qkv[:, :, :d])
    np.testing.assert_array_equal(host(got), host(ref_gpu))
    rows = host(qkv)
    E.attention_preconditions(prof, pattern, rows, mask, H)
    r64 = E.attention_ref(rows, H, mask, np.float64)
    bound, e32 = E.attention_bound(r64, E.attention_ref(rows, H, mask, np.float32), rows)
    err = _attn_err(host(got), r64)
    _record_attention(f'kv-{prof}-{pattern}-T{T}-hd{hd}-{mask_kind}',
                      dict(E32=e32, bound=bound, ratio={'kv': err / e32}, err={'kv': err}))
    assert err <= bound, (err, bound, e32)


@pytest.mark.parametrize('presplit', [True, False])
def test_attention_range_guard_boundary(presplit):
    """A value entry of exactly 65504 is in range on the f16x3 kernels (status 0, the result
    within bound B); the next float up sets status bit 0."""
    from forwardtacotron_amd import ops
    qkv = E.attention_inputs('ramp', 'one', 200, 64, seed=5)
    d = qkv.shape[-1] // 3
    qkv[1, 150, 2 * d + 3] = 65504.0
    r64 = E.attention_ref(qkv, 2, None, np.float64)
    bound, e32 = E.attention_bound(r64, E.attention_ref(qkv, 2, None, np.float32), qkv)
    st = _status()
    got = host(ops.attention(dev(qkv), 2, mma=2, presplit=presplit))
    assert int(st.item()) == 0
    assert _attn_err(got, r64) <= bound
    qkv[1, 150, 2 * d + 3] = np.nextafter(np.float32(65504), np.float32(np.inf))
    ops.attention(dev(qkv), 2, mma=2, presplit=presplit)
    torch.cuda.synchronize()
    assert int(st.item()) & 1
    st.zero_()


# ================================================================ D. LayerNorm
def _ln_inputs(M, C, seed=0):
    r = np.random.RandomState(1000 * C + M + seed)
    x = (r.randn(1, M, C) * 3 + 1).astype(np.float32)
    return x, r.uniform(0.5, 1.5, C).astype(np.float32), r.randn(C).astype(np.float32)


@pytest.mark.parametrize('M', [1, 5])
@pytest.mark.parametrize('C', [1, 65, 384, 520, 1024])
def test_layernorm_widths_and_rows(C, M):
    """2 values per lane with a ragged tail (C = 1, 65), 8 (384, 520: ragged) and 16 (1024);
    1 and 5 rows: a partial 4-row block."""
    from forwardtacotron_amd import ops
    x, g, b = _ln_inputs(M, C)
    got = host(ops.layernorm(dev(x), dev(g), dev(b)))
    np.testing.assert_allclose(got, FP.layer_norm(x, g, b), atol=2e-6, rtol=2e-6)


def test_layernorm_too_wide_raises():
    from forwardtacotron_amd import ops
    from forwardtacotron_amd._lib import FtmiError
    x, g, b = _ln_inputs(2, 1025)
    with pytest.raises(FtmiError):
        ops.layernorm(dev(x), dev(g), dev(b))


@pytest.mark.parametrize('C', [65, 520])
def test_layernorm_strided_views_and_alias(C):
    """Input and output as column ranges of wider tensors (what lies beside them is left
    alone), and out = x."""
    from forwardtacotron_amd import ops
    M = 5
    x, g, b = _ln_inputs(M, C)
    ref = FP.layer_norm(x, g, b)
    wide_in = torch.full((1, M, C + 24), 7.0, device='cuda')
    wide_in[:, :, 8:8 + C] = dev(x)
    wide_out = torch.full((1, M, C + 40), -3.0, device='cuda')
    y = ops.layernorm(wide_in[:, :, 8:8 + C], dev(g), dev(b), out=wide_out[:, :, 16:16 + C])
    np.testing.assert_allclose(host(y), ref, atol=2e-6, rtol=2e-6)
    np.testing.assert_array_equal(host(y), host(ops.layernorm(dev(x), dev(g), dev(b))))
    wo = host(wide_out)
    assert np.all(wo[:, :, :16] == -3.0) and np.all(wo[:, :, 16 + C:] == -3.0)
    xv = wide_in[:, :, 8:8 + C]
    y2 = ops.layernorm(xv, dev(g), dev(b), out=xv)
    assert y2.data_ptr() == xv.data_ptr()
    np.testing.assert_array_equal(host(y2), host(y))
    wi = host(wide_in)
    assert np.all(wi[:, :, :8] == 7.0) and np.all(wi[:, :, 8 + C:] == 7.0)


@pytest.mark.parametrize('C', [80, 256, 1024])
def test_layernorm_offset_rows(C):
    """Rows of mean 1e4 and standard deviation 1: x rstd - mean rstd cancels five digits, in
    the reference's fp32 kernel too; the error is held to F times the fp32 reference's own
    (torch layer_norm on the CPU), F and the floor as for attention."""
    from forwardtacotron_amd import ops
    r = np.random.RandomState(C)
    x = (r.randn(1, 37, C) + 1e4).astype(np.float32)
    g = r.uniform(0.5, 1.5, C).astype(np.float32)
    b = r.randn(C).astype(np.float32)
    xt, gt, bt = (torch.from_numpy(a) for a in (x, g, b))
    r64 = torch.nn.functional.layer_norm(xt.double(), (C,), gt.double(), bt.double()).numpy()
    r32 = torch.nn.functional.layer_norm(xt, (C,), gt, bt).numpy()
    e32 = float(np.abs(r32 - r64).max())
    got = host(ops.layernorm(dev(x), dev(g), dev(b)))
    err = float(np.abs(got - r64).max())
    print(f'layernorm offset rows C={C}: err {err:.3e}, E32 {e32:.3e}, ratio {err / e32:.2f}')
    assert err <= E.ATTN_F * e32 + E.ATTN_FLOOR * float(np.abs(r64).max())


def test_panel_proj_layernorm_offset_rows_bit_identical(rng, monkeypatch):
    """panel_proj(ln=) on rows whose residual carries an offset of 1e4 (so the normalised rows
    have mean 1e4, deviation ~1) against the unfused conv1d + layernorm: bit for bit where the
    unfused GEMM runs unsplit (test_panel_proj's condition), and against float64 within F
    times the error of torch's fp32 layer_norm of the same pre-norm rows."""
    from forwardtacotron_amd import ops
    monkeypatch.setenv('FTMI_GEMM_SKINNY', '0')
    B, T, K, N = 4, 900, 256, 256
    x = rng.normal(0, 1, (B, T, K)).astype(np.float32)
    w = (rng.normal(0, 1, (N, K)) / np.sqrt(K)).astype(np.float32)
    b = rng.normal(0, 0.1, N).astype(np.float32)
    r = (rng.normal(0, 1, (B, T, N)) + 1e4).astype(np.float32)
    g = rng.normal(1, 0.2, N).astype(np.float32)
    bt = rng.normal(0, 0.2, N).astype(np.float32)
    wd = dev(w)
    lnp = (dev(g), dev(bt), 1e-5)
    y = ops.panel_proj(dev(x), ops.split_weights_f16(wd, frag=True), N, bias=dev(b), residual=dev(r),
                       ln=lnp)
    yu, _ = ops.conv1d(dev(x), wd, 1, 0, bias=dev(b), residual=dev(r), w_split=ops.split_weights_f16(wd))
    pre = host(yu).copy()  # the pre-norm rows, as the GPU has them in fp32
    yu = ops.layernorm(yu, lnp[0], lnp[1], 1e-5, out=yu)
    assert B * T > 256 and ops._split_k(B * T, N, K, 2, True, K) == 1
    np.testing.assert_array_equal(host(y).view(np.uint32), host(yu).view(np.uint32))
    pt, gt, btt = (torch.from_numpy(a) for a in (pre, g, bt))
    r64 = torch.nn.functional.layer_norm(pt.double(), (N,), gt.double(), btt.double()).numpy()
    e32 = float(np.abs(torch.nn.functional.layer_norm(pt, (N,), gt, btt).numpy() - r64).max())
    err = float(np.abs(host(y) - r64).max())
    print(f'panel_proj ln offset rows: err {err:.3e}, E32 {e32:.3e}, ratio {err / e32:.2f}')
    assert err <= E.ATTN_F * e32 + E.ATTN_FLOOR * float(np.abs(r64).max())


# ================================================================ C. rescaled checkpoints
def _accuracy(name, got, ref32, ref64, keys):
    """test_gpu_accuracy.py's assertion form and FACTORS: the path is no further from the fp64
    truth than FACTOR x the fp32 reference is (+ FLOOR), in mean and in max."""
    from test_gpu_accuracy import FACTORS, FLOOR, _err, _record
    stats = {}
    for k in keys:
        truth = ref64[k].numpy()
        assert tuple(got[k].shape) == truth.shape
        stats[k] = {'fp32_reference': _err(ref32[k].numpy(), truth),
                    'default': _err(got[k].cpu().numpy(), truth)}
    _record(name, stats)
    f_mean, f_max = FACTORS['default']
    for k in keys:
        e, e_ref = stats[k]['default'], stats[k]['fp32_reference']
        assert e['mean'] <= f_mean * e_ref['mean'] + FLOOR, (k, e, e_ref)
        assert e['max'] <= f_max * e_ref['max'] + FLOOR, (k, e, e_ref)


def _varied(sd, keys):
    """The rescaled weights ask for at least 8 distinct column scales each."""
    for k in keys:
        assert len(np.unique(E.scale_exponents(sd[k]))) >= 8, k


def test_forward_tacotron_rescaled_checkpoint():
    """ForwardTacotron (B = 2, T = 40) on synthetic weights whose bank / projection /
    predictor conv rows, CBHG tails, LSTM weight_ih and lin rows are rescaled
    (f16x3_emu.rescale_forward_tacotron): generate() against the torch-CPU oracle in float64
    on the same state dict; duration counts bit-equal; status 0 (no exact rerun)."""
    from forwardtacotron_amd import ops
    from forwardtacotron_amd.forward_tacotron import ForwardTacotron
    from forwardtacotron_amd.synthetic import default_config, synthetic_state_dict, synthetic_tokens
    from oracle import ft_torch_cpu as TC
    m = ForwardTacotron.from_config(default_config())
    sd = E.rescale_forward_tacotron(synthetic_state_dict(m, seed=0))
    _varied(sd, ['prenet.conv1d_bank.3.conv.weight', 'postnet.conv_project1.conv.weight',
                 'prenet.pre_highway.weight', 'postnet.highways.2.W1.weight',
                 'dur_pred.convs.1.conv.weight'])
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m = m.to('cuda').eval()
    x = torch.from_numpy(synthetic_tokens(2, 40, seed=0, min_len=30))
    ref32 = TC.generate(TC.to_torch(sd), x)
    ref64 = TC.generate(TC.to_torch(sd, torch.float64), x, lr_dur=ref32['dur'])
    out = m.generate(x.cuda())
    assert int(ops.status_word('cuda').item()) == 0
    assert np.array_equal(O.duration_counts(out['dur'].cpu().numpy()),
                          O.duration_counts(ref32['dur'].numpy()))
    _accuracy('rescaled_forward_tacotron', out, ref32, ref64, ('mel', 'mel_post'))


def test_fast_pitch_rescaled_checkpoint():
    """FastPitch (B = 2, T = 40) with every FFT block's in_proj / out_proj and conv1 / conv2
    rescaled (f16x3_emu.rescale_fast_pitch), against the torch-CPU oracle in float64."""
    from forwardtacotron_amd import ops
    from forwardtacotron_amd.fast_pitch import FastPitch
    from forwardtacotron_amd.synthetic import default_config, synthetic_state_dict, synthetic_tokens
    from oracle import fp_torch_cpu as FTC
    m = FastPitch.from_config(default_config())
    sd = E.rescale_fast_pitch(synthetic_state_dict(m, 0, 'fast_pitch'))
    _varied(sd, ['prenet.layers.0.self_attn.in_proj_weight', 'postnet.layers.3.conv1.weight',
                 'dur_pred.transformer.layers.1.conv1.weight'])
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m = m.cuda().eval()
    x = torch.from_numpy(synthetic_tokens(2, 40, seed=0, min_len=30))
    ref32 = FTC.generate(FTC.to_torch(sd), x)
    ref64 = FTC.generate(FTC.to_torch(sd, torch.float64), x, lr_dur=ref32['dur'])
    out = m.generate(x.cuda())
    assert int(ops.status_word('cuda').item()) == 0
    assert np.array_equal(FP.duration_counts(out['dur'].cpu().numpy()),
                          FP.duration_counts(ref32['dur'].numpy()))
    _accuracy('rescaled_fast_pitch', out, ref32, ref64, ('mel',))


def test_wavernn_upsample_small_running_var():
    """WaveRNN's upsampling network with running_var = 1e-4 on three channels of the last
    ResBlock's first BatchNorm: the BN-folded conv rows there exceed 16 (their column scale
    differs from their neighbours').  upsample_forward against oracle/wr_torch_cpu.upsample in
    float64 on that state dict, test_upsample_matches_reference's bound per output channel:
    |err| <= 1e-5 |ref| + 2e-6 max|ref[:, c]|."""
    from conftest import load_golden
    from forwardtacotron_amd.synthetic import default_config, load_synthetic
    from forwardtacotron_amd.wavernn import WaveRNN
    from oracle import wr_torch_cpu as wr
    cfg = default_config()
    m = WaveRNN.from_config(cfg)
    load_synthetic(m, kind='wavernn')
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    rows = [1, 12, 23]
    sd['upsample.resnet.layers.9.batch_norm1.running_var'][rows] = 1e-4
    m.load_state_dict(sd)
    m = m.to('cuda').eval()
    w, _, w3 = m.packed_weights()[0][1][9][0]  # the folded conv1 of ResBlock 9 and its planes
    top = host(w.abs().amax(1))
    others = np.setdiff1d(np.arange(top.size), rows)
    assert np.all(top[rows] >= 16) and np.all(top[others] < 16)
    cs = E.read_colscale(host(w3), w.size(0), w.size(1))
    assert np.all(cs[rows] > cs[others].max())
    mels = torch.from_numpy(load_golden('wr_upsample')['mels'])
    sd64 = {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}
    refs = wr.upsample(sd64, mels.double(), dict(cfg['vocoder']['model']))
    st = _status()
    gots = m.upsample_forward(mels.cuda())
    assert int(st.item()) == 0
    for name, got, ref in zip(('up', 'aux'), gots, refs):
        got, ref = host(got).astype(np.float64), ref.numpy()
        bound = 1e-5 * np.abs(ref) + 2e-6 * np.abs(ref).max((0, 1), keepdims=True)
        ratio = float((np.abs(got - ref) / bound).max())
        print(f'wavernn upsample {name}: worst |err| / bound = {ratio:.3f}')
        assert ratio <= 1.0, (name, ratio)
