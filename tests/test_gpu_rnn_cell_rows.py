"""The cell-row form of the f16x3 recurrence (rnn_bidir_kernel CR: unit-major W_hh rows, each
cell's four gate sums in one lane, 16-byte K-split exchange) against the gate-major form it
replaces (FTMI_RNN_CELLROWS=0): the K-split partials are added in the same order, so y must
be bit-identical — every frame of both directions, which includes the final hidden states
(y[:, len - 1, :H] forward, y[:, 0, H:] reverse; the cell state is not exposed, but every
h_t = o * tanh(c_t) is).  The gate-major form itself is held to the numpy oracle by
test_gpu_kernels.py and the model tests; test_gpu_rnn_cases.py holds both layouts to float64
with lengths / index, T < 3 and off the unit value scale (a mistake both layouts share).

Shapes: the LSTM (H 512, 16 units per workgroup) at B = 5 (one ragged chunk, past the GEMV
kernel's B <= 4), 16 (one full chunk), 17 (a ragged second chunk), 64 (four chunks: one
workgroup per CU); the spread GRU (H 256, 8 units per workgroup) at B = 16 / 40 / 64; T = 3,
4, 5, 8 covers every residue of the 3-step register rotation."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TS = (3, 4, 5, 8)


@pytest.fixture
def f16x3(monkeypatch):
    """The default dispatch: f16x3, compute-wave h stores, the spread GRU on 8 units."""
    from forwardtacotron_amd import ops
    monkeypatch.setattr(ops, 'RNN_MMA', 2)
    for v in ('FTMI_RNN_CSTORE', 'FTMI_RNN_U8', 'FTMI_RNN_GEMV', 'FTMI_RNN_NB', 'FTMI_RNN_PAD',
              'FTMI_RNN_XCD_LOCAL', 'FTMI_RNN_CELLROWS', 'FTMI_RNN_PSLEEP'):
        monkeypatch.delenv(v, raising=False)
    return ops


def _case(cell, H, B, T, mode, seed):
    """Random weights and projections; the projections' scale varies over the batch rows."""
    rng = np.random.Generator(np.random.PCG64(seed))
    G = 4 if cell else 3
    T_src = T if mode != 'index' else max(2, T - 1)
    w_hh = rng.normal(0, 1 / np.sqrt(H), (2, G * H, H)).astype(np.float32)
    b_hh = rng.normal(0, 0.1, 2 * G * H).astype(np.float32)
    xp = rng.normal(0, 1, (B, T_src, 2 * G * H)).astype(np.float32)
    xp *= np.array([0.25, 1.0, 4.0], np.float32)[np.arange(B) % 3][:, None, None]
    kw = {}
    if mode == 'index':  # a LengthRegulator map: rows repeat, -1 = past the sequence's end
        idx = np.sort(rng.integers(0, T_src, (B, T)), axis=1).astype(np.int32)
        for b in range(B):
            idx[b, T - (b % 3):] = -1
        kw['index'] = torch.from_numpy(idx).cuda()
        kw['xp_zero'] = torch.from_numpy(rng.normal(0, 0.1, 2 * G * H).astype(np.float32)).cuda()
    if mode == 'lengths':  # shorter than T: pads the forward tail, restarts the reverse pass
        kw['lengths'] = torch.from_numpy(np.array([max(1, T - (b % 4)) for b in range(B)], np.int32))
        kw['pad_value'] = -11.5129
    return (torch.from_numpy(xp).cuda(), torch.from_numpy(w_hh).cuda(),
            None if cell else torch.from_numpy(b_hh).cuda(), kw)


def _both(ops, monkeypatch, cell, H, B, T, mode, spread, seed=7):
    xp, w_hh, b_hh, kw = _case(cell, H, B, T, mode, seed)
    st = ops.status_word('cuda')
    st.zero_()
    out = {}
    for rows in ('1', '0'):
        monkeypatch.setenv('FTMI_RNN_CELLROWS', rows)
        y = ops.rnn_bidir(cell, xp, H, w_hh, b_hh, T=T, check=True, spread=spread, **kw)
        torch.cuda.synchronize()
        out[rows] = y.cpu().numpy()
    assert int(st.item()) == 0
    new, old = out['1'], out['0']
    assert np.isfinite(old).all() and old.std() > 0.01, 'degenerate case'
    assert np.array_equal(new, old), (
        f'B={B} T={T} {mode}: {np.count_nonzero(new != old)} of {old.size} values differ, '
        f'max |diff| {np.abs(new - old).max():.3e}')
    return new


@pytest.mark.parametrize('mode', ['plain', 'index', 'lengths'])
@pytest.mark.parametrize('B', [5, 16, 17, 64])
def test_lstm_cell_rows_equal_gate_major(B, mode, f16x3, monkeypatch):
    for T in TS:
        _both(f16x3, monkeypatch, 1, 512, B, T, mode, spread=True)


@pytest.mark.parametrize('mode', ['plain', 'lengths'])
@pytest.mark.parametrize('B', [16, 40, 64])
def test_spread_gru_u8_cell_rows_equal_gate_major(B, mode, f16x3, monkeypatch):
    ops = f16x3
    # the 8-unit form: every group's 32 workgroups, the grid padded to 8 groups
    ngroups = 2 * ((B + 15) // 16)
    assert ops.rnn_blocks(0, B, 256, 2 | ops.RNN_SPREAD) == max(8, ngroups) * 32
    for T in TS:
        _both(ops, monkeypatch, 0, 256, B, T, mode, spread=True)


@pytest.mark.parametrize('cell,H,B', [(1, 512, 17), (0, 256, 40)])
def test_cell_rows_write_through_fallback(cell, H, B, f16x3, monkeypatch):
    """FTMI_RNN_XCD_LOCAL=0: groups by blockIdx, h stored write-through (the 8-byte pieces
    take the sc1 store)."""
    monkeypatch.setenv('FTMI_RNN_XCD_LOCAL', '0')
    ref = None
    for T in (4, 5):
        got = _both(f16x3, monkeypatch, cell, H, B, T, 'lengths', spread=True)
        if T == 5:
            ref = got
    # and the fallback computes what the XCD-local mode computes
    monkeypatch.delenv('FTMI_RNN_XCD_LOCAL')
    assert np.array_equal(_both(f16x3, monkeypatch, cell, H, B, 5, 'lengths', spread=True), ref)


@pytest.mark.parametrize('cell,H', [(1, 512), (0, 256)])
def test_cell_rows_no_timeout_at_default_spin_limit(cell, H, f16x3, monkeypatch):
    """At the normal spin bound no workgroup gives up: status bit 2 stays clear."""
    from forwardtacotron_amd import _lib
    ops = f16x3
    lib = _lib.load()
    lib.ftmi_set_rnn_spin_limit(0)  # 0 = the default bound
    xp, w_hh, b_hh, kw = _case(cell, H, 64, 8, 'plain', 11)
    st = ops.status_word('cuda')
    st.zero_()
    monkeypatch.setenv('FTMI_RNN_CELLROWS', '1')
    ops.rnn_bidir(cell, xp, H, w_hh, b_hh, T=8, check=True, spread=True, **kw)
    torch.cuda.synchronize()
    assert int(st.item()) & ops.STATUS_RNN_TIMEOUT == 0
