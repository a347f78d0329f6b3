"""The kernels of the length-aware batch (csrc/seq.hip: ftmi_fill_tail, ftmi_maxpool_rows,
ftmi_duration_counts_rows) against numpy restatements written here, bit for bit."""
import numpy as np
import pytest
import torch

from forwardtacotron_amd import _lib, ops

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-777.25)
GUARD = 64  # floats of sentinel before and after the operand (a multiple of 4: 16-byte aligned)

# (B, T, C, row stride, lengths): L = T, L = T - 1 (reach 4 is clamped at T) and L = 1
SHAPES = [
    (3, 5, 1, 3, [5, 4, 1]),
    (3, 5, 4, 8, [5, 4, 1]),
    (3, 5, 4, 6, [5, 4, 1]),       # a stride that is no multiple of 4: the 4-byte stores
    (3, 5, 260, 264, [5, 4, 1]),   # more than one pass of 64 lanes x 4 floats
    (2, 70, 512, 516, [69, 1]),
]


def _alloc(n, offset=0):
    buf = torch.full((GUARD + offset + n + GUARD,), float(SENTINEL), device='cuda')
    return buf, buf[GUARD + offset:GUARD + offset + n]


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _tail(L, reach, T):
    return range(L, T if reach < 0 else min(T, L + reach))


@pytest.mark.parametrize('B,T,C,S,lens', SHAPES)
@pytest.mark.parametrize('reach,value', [(4, 0.0), (1, 0.0), (-1, -11.5129), (2, 3.5)])
@pytest.mark.parametrize('offset', [0, 1])
def test_fill_tail_rows(B, T, C, S, lens, reach, value, offset):
    """Channels-last rows with a row stride larger than C, aligned (16-byte stores where C
    and the stride allow) and one float off (4-byte stores): the specified tails hold the
    value, every other byte of the allocation — the stride gap, the next item's row 0, the
    guards — is unchanged."""
    buf, flat = _alloc(B * T * S, offset)
    x = flat.view(B, T, S)[:, :, :C]
    want = buf.cpu().numpy().copy()
    w = want[GUARD + offset:GUARD + offset + B * T * S].reshape(B, T, S)
    for b, L in enumerate(lens):
        for t in _tail(L, reach, T):
            w[b, t, :C] = np.float32(value)
    ops.fill_tail(x, torch.tensor(lens, device='cuda'), reach=reach, value=value)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(buf.cpu().numpy()), _bits(want))


@pytest.mark.parametrize('B,T,C,S,lens', [(3, 5, 1, 5, [5, 4, 1]), (3, 5, 4, 7, [5, 4, 1]),
                                          (3, 5, 260, 9, [5, 4, 1]), (2, 70, 80, 73, [69, 1])])
@pytest.mark.parametrize('reach,value', [(4, 0.0), (-1, -11.5129)])
def test_fill_tail_time_last(B, T, C, S, lens, reach, value):
    """The (B, C, T) layout of mel / mel_post / pitch / energy, channel stride S >= T."""
    buf, flat = _alloc(B * C * S)
    x = flat.view(B, C, S)[:, :, :T]
    want = buf.cpu().numpy().copy()
    w = want[GUARD:GUARD + B * C * S].reshape(B, C, S)
    for b, L in enumerate(lens):
        for t in _tail(L, reach, T):
            w[b, :, t] = np.float32(value)
    ops.fill_tail(x, torch.tensor(lens, device='cuda'), reach=reach, value=value, time_last=True)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(buf.cpu().numpy()), _bits(want))


@pytest.mark.parametrize('B,T,C,S,lens', [s for s in SHAPES if s[2] % 2 == 0])
@pytest.mark.parametrize('reach,value', [(1, 0.0), (4, 0.3), (-1, 0.0)])
def test_fill_tail_split_rows(B, T, C, S, lens, reach, value):
    """f16x3 split rows (include/ftmi.h): a row is C f16 heads then C f16 tails
    t = f16((v - h) 2^11); zero is all-zero halves."""
    buf, flat = _alloc(B * T * S)
    x = flat.view(B, T, S)[:, :, :C]
    want = buf.cpu().numpy().copy()
    w = want[GUARD:GUARD + B * T * S].reshape(B, T, S)
    h = np.float16(np.float32(value))
    tl = np.float16((np.float32(value) - np.float32(h)) * np.float32(2048.0))
    row = np.concatenate([np.full(C, h, np.float16), np.full(C, tl, np.float16)]).view(np.float32)
    for b, L in enumerate(lens):
        for t in _tail(L, reach, T):
            w[b, t, :C] = row
    ops.fill_tail(x, torch.tensor(lens, device='cuda'), reach=reach, value=value, split=True)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(buf.cpu().numpy()), _bits(want))
    if value == 0.0:  # the same bytes as fp32 zeros
        assert all((w[b, t, :C] == 0).all() for b, L in enumerate(lens) for t in _tail(L, reach, T))


def test_fill_tail_refuses_odd_split_rows():
    x = torch.zeros(3, 5, 1, device='cuda')
    with pytest.raises(_lib.FtmiError, match='status 1002'):
        ops.fill_tail(x, torch.tensor([5, 4, 1], device='cuda'), reach=1, split=True)


@pytest.mark.parametrize('B,T,C,S,lens', [(3, 5, 4, 8, [5, 4, 1]), (3, 5, 260, 264, [5, 4, 1]),
                                          (2, 70, 512, 516, [69, 1])])
def test_maxpool_rows(B, T, C, S, lens):
    """max(x[t-1], x[t]) below an item's length (x[-1] = -inf), zero rows from there on;
    the input's stride gap and the guards are untouched."""
    rng = np.random.Generator(np.random.PCG64(7))
    buf, flat = _alloc(B * T * S)
    x = flat.view(B, T, S)[:, :, :C]
    xv = rng.standard_normal((B, T, C)).astype(np.float32)
    x.copy_(torch.from_numpy(xv))
    before = buf.cpu().numpy().copy()
    y = ops.maxpool_rows(x, torch.tensor(lens, device='cuda'))
    torch.cuda.synchronize()
    want = np.zeros((B, T, C), np.float32)
    for b, L in enumerate(lens):
        want[b, 0] = xv[b, 0]
        want[b, 1:L] = np.maximum(xv[b, :L - 1], xv[b, 1:L])
    assert np.array_equal(_bits(y.cpu().numpy()), _bits(want))
    assert np.array_equal(_bits(buf.cpu().numpy()), _bits(before))


def duration_rows_ref(dur, x_len, fill=np.float32(2.0)):
    """ftmi_duration_counts_rows in numpy: (dur after the call, offsets, totals, flags)."""
    dur = dur.copy()
    B, T = dur.shape
    off = np.zeros((B, T + 1), np.int32)
    flags = np.zeros(B, np.int32)
    for b in range(B):
        L = int(x_len[b])
        v = dur[b, :L]
        if np.trunc(v).astype(np.int64).sum() <= 0:
            v[:] = fill
            flags[b] = 1
        v[v < 0] = np.float32(0)
        dur[b, L:] = np.float32(0)
        counts = np.zeros(T, np.int64)
        counts[:L] = np.trunc((v + np.float32(0.5)).astype(np.float32)).astype(np.int64)
        off[b, 1:] = np.cumsum(counts)
    return dur, off, off[:, T].copy(), flags


@pytest.mark.parametrize('T', [1, 5, 65, 130])
def test_duration_counts_rows(T):
    """Six rows (two workgroups of four waves), T across the 64-lane scan chunks: row 0's
    valid durations are all below 1 (and partly negative) beside rows that are not — only it
    and row 4 fill, at their valid positions only; row 4's pads hold 5.0, which must count
    neither for the rule nor for the frames; x_len = 1 (row 1) and x_len = T (rows 0, 3, 5)."""
    rng = np.random.Generator(np.random.PCG64(100 + T))
    B = 6
    dur = rng.uniform(-1.0, 6.0, (B, T)).astype(np.float32)
    x_len = np.array([T, 1, max(1, T - 1), T, max(1, T // 2), T], np.int32)
    dur[0] = rng.uniform(-0.9, 0.99, T).astype(np.float32)
    dur[1, 0] = np.float32(4.25)
    dur[4] = np.float32(5.0)
    dur[4, :x_len[4]] = rng.uniform(0.0, 0.99, int(x_len[4])).astype(np.float32)
    dur[5, 0] = np.float32(3.0)
    want_dur, want_off, want_tot, want_flags = duration_rows_ref(dur, x_len)
    d = torch.from_numpy(dur).cuda()
    off, tot, flags = ops.duration_counts_rows(d, torch.from_numpy(x_len).cuda())
    torch.cuda.synchronize()
    assert np.array_equal(flags.cpu().numpy(), want_flags)
    assert want_flags[0] == 1 and want_flags[4] == 1 and want_flags[5] == 0
    assert np.array_equal(_bits(d.cpu().numpy()), _bits(want_dur))
    assert np.array_equal(off.cpu().numpy(), want_off)
    assert np.array_equal(tot.cpu().numpy(), want_tot)
    assert want_tot[4] == 2 * x_len[4] and (want_dur[4, x_len[4]:] == 0).all()


def test_duration_counts_rows_known_answer():
    """0.49999997 + 0.5 rounds to 1.0 in fp32 (one frame, not zero); the pad's 7.0 counts
    for nothing; a negative duration is clipped in place."""
    dur = np.array([[0.49999997, 3.0, -0.25, 7.0]], np.float32)
    d = torch.from_numpy(dur).cuda()
    off, tot, flags = ops.duration_counts_rows(d, torch.tensor([3], device='cuda'))
    torch.cuda.synchronize()
    assert off.cpu().tolist() == [[0, 1, 4, 4, 4]] and tot.cpu().tolist() == [4]
    assert flags.cpu().tolist() == [0]
    assert np.array_equal(_bits(d.cpu().numpy()),
                          _bits(np.array([[0.49999997, 3.0, 0.0, 0.0]], np.float32)))
    want = duration_rows_ref(dur, [3])
    assert np.array_equal(want[1], off.cpu().numpy())


def test_duration_counts_rows_equals_duration_counts_on_full_rows():
    """With every x_len = T and one row, the per-item kernel is the existing kernel."""
    rng = np.random.Generator(np.random.PCG64(5))
    dur = rng.uniform(-1.0, 6.0, (1, 130)).astype(np.float32)
    a, b = torch.from_numpy(dur).cuda(), torch.from_numpy(dur).cuda()
    off_a, tot_a, _ = ops.duration_counts(a, apply_fill=True)
    off_b, tot_b, _ = ops.duration_counts_rows(b, torch.tensor([130], device='cuda'))
    assert torch.equal(off_a, off_b) and torch.equal(tot_a, tot_b) and torch.equal(a, b)
