"""The host side of the recurrence cases (no GPU; the route test needs the built library, like
test_rnn_route.py): the reference `recur_ref` against torch.nn.GRU / LSTM, the conditions under
which a case says something about a kernel, the planted defects against the bound with the
committed F values, and the routes the case table reaches."""
import numpy as np
import pytest
import torch

import rnn_cases as R

CUS = 256  # the count the route is asked for here; the GPU test asks the device's own


def _B(case):
    return R.resolve_B(case, CUS)


@pytest.fixture
def switches(monkeypatch):
    def use(case):
        R.clear_switches(monkeypatch, R.FORMS[case.form].switches)
    return use


# ---------------------------------------------------------------- the reference
def _torch_module(cell, H, w_hh, b_hh):
    """nn.GRU / nn.LSTM in float64 whose input projection reproduces xp: W_ih = I on a G H wide
    input, b_ih = 0 (and b_hh = 0 for the LSTM, which ftmi_rnn_bidir runs without one)."""
    G = 4 if cell else 3
    m = (torch.nn.LSTM if cell else torch.nn.GRU)(G * H, H, batch_first=True, bidirectional=True).double()
    sd = {}
    for d, sfx in enumerate(('', '_reverse')):
        sd['weight_ih_l0' + sfx] = torch.eye(G * H, dtype=torch.float64)
        sd['weight_hh_l0' + sfx] = torch.from_numpy(w_hh[d].astype(np.float64))
        sd['bias_ih_l0' + sfx] = torch.zeros(G * H, dtype=torch.float64)
        sd['bias_hh_l0' + sfx] = (torch.zeros(G * H, dtype=torch.float64) if b_hh is None else
                                  torch.from_numpy(b_hh[d * G * H:(d + 1) * G * H].astype(np.float64)))
    m.load_state_dict(sd)
    return m


def _torch_run(m, xe, lengths, pad_value):
    """Both directions read their own half of xe: two passes, each keeping its direction."""
    from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence
    H, T = m.hidden_size, xe.shape[1]
    GH = xe.shape[2] // 2
    out = []
    for d in (0, 1):
        x = torch.from_numpy(xe[:, :, d * GH:(d + 1) * GH].astype(np.float64))
        with torch.no_grad():
            if lengths is None:
                y = m(x)[0]
            else:
                p = pack_padded_sequence(x, torch.from_numpy(lengths.astype(np.int64)), batch_first=True,
                                         enforce_sorted=False)
                y = pad_packed_sequence(m(p)[0], batch_first=True, padding_value=pad_value,
                                        total_length=T)[0]
        out.append(y[..., d * H:(d + 1) * H].numpy())
    return np.concatenate(out, axis=2)


@pytest.mark.parametrize('mode', R.MODES)
@pytest.mark.parametrize('cell,H,B,T', [(0, 64, 5, 7), (0, 128, 19, 4), (1, 512, 3, 5), (0, 256, 2, 1),
                                        (1, 512, 9, 2)])
def test_reference_is_torch(cell, H, B, T, mode):
    """recur_ref in float64 is nn.GRU / nn.LSTM (CPU, float64, bidirectional) to 1e-12: lengths
    through pack_padded_sequence / pad_packed_sequence(padding_value=pad_value), index through
    the explicitly gathered sequence.  Independent of oracle/ft_oracle.py."""
    op = R.operands(cell, H, B, T, mode, 'rows', 'batch')
    xe = op.xp
    if 'index' in op.kw:
        idx = op.kw['index']
        xe = np.where((idx >= 0)[..., None], op.xp[np.arange(B)[:, None], np.maximum(idx, 0)],
                      op.kw['xp_zero'])
    want = _torch_run(_torch_module(cell, H, op.w_hh, op.b_hh), xe, op.kw.get('lengths'),
                      op.kw.get('pad_value', 0.0))
    assert op.ref64.shape == want.shape == (B, T, 2 * H) and op.ref64.dtype == np.float64
    assert np.abs(op.ref64 - want).max() <= 1e-12
    assert op.ref32.dtype == np.float32


# ---------------------------------------------------------------- the cases
def test_table_axes():
    """What the table holds: every BIDIR form in all four call modes at one full chunk plus one
    sequence, every GEMV form at B = 1..4, T = 1, 2, 3, the value domain at T <= 4 only."""
    by_axis = {}
    for c in R.CASES:
        by_axis.setdefault(c.axis, []).append(c)
    forms = {(c.form, c.mode) for c in by_axis['forms']}
    assert {(f, m) for f in R.BIDIR_FORMS for m in R.MODES} <= forms
    assert all(c.B == R.FORMS[c.form].route[5] + 1 and c.T == 7 for c in by_axis['forms']
               if c.form in R.BIDIR_FORMS)
    assert {(c.form, c.B, c.mode) for c in by_axis['forms'] if c.form in R.GEMV_FORMS} == {
        (f, B, m) for f in R.GEMV_FORMS for B in (1, 2, 3, 4) for m in ('plain', 'index+lengths')}
    assert {(c.form, c.T, c.mode) for c in by_axis['short']} == {
        (f, T, m) for f in R.SHORT_FORMS for T in (1, 2, 3) for m in ('plain', 'lengths')}
    assert all(c.T <= 4 for c in R.CASES if c.wpat.startswith('outlier') or c.xpat == 'saturating')
    assert {c.T for c in by_axis['drift']} == {66, 301}
    assert len({c.id for c in R.CASES}) == len(R.CASES)


@pytest.mark.parametrize('case', R.CASES, ids=[c.id for c in R.CASES])
def test_case_conditions(case, switches):
    """float32 itself stays within E32_CAP of float64 (the case is not chaotic), the output is
    not degenerate, a saturating pattern saturates on both sides, lengths are in [1, T] with 1
    and T among them and differ, like the index rows, between a sequence and the ones 8 and 16
    before it (what a kernel reading another chunk's rows would mix up)."""
    switches(case)
    B = _B(case)
    op = R.case_operands(case, B)
    e_max, _ = R.errors(op.ref32, op.ref64)
    assert e_max <= R.E32_CAP
    live = R.live_mask(op)
    assert np.isfinite(op.ref64).all() and op.ref64[live].std() > 0.01
    if case.xpat == 'saturating':
        assert op.stats['sat_hi'] > 0.05 and op.stats['sat_lo'] > 0.05
        assert not op.xp[1].any() and np.count_nonzero(op.xp[0] == 0) > 0.05 * op.xp[0].size
        # h pinned at +-1 (the LSTM's o tanh(c) with |c| <= T reaches tanh(3) = 0.995 at T = 3)
        assert np.abs(op.ref64).max() > 0.99
    lens, idx = op.kw.get('lengths'), op.kw.get('index')
    if lens is not None:
        assert lens.min() >= 1 and lens.max() <= case.T
        if B >= 2:
            assert lens.min() == 1 and lens.max() == case.T
        assert (op.ref64[~live] == R.PAD_VALUE).all() and (op.ref32[~live] == np.float32(R.PAD_VALUE)).all()
        for k in (8, 16):
            assert (lens[k:] != lens[:-k]).all()
    if idx is not None:
        assert idx.min() >= -1 and idx.max() < op.xp.shape[1] and idx.shape == (B, case.T)
        assert B == 1 or (idx[live] == -1).any()
        for k in (8, 16):
            assert (idx[k:, 0] != idx[:-k, 0]).all()


def applicable_defects(case, B):
    nbl = R.FORMS[case.form].route[5] or 16
    d = []
    if R.path_of(case) == 'f16x3' and case.T >= 2:
        d += ['a', 'b']
    if 'lengths' in case.mode and case.T >= 2:  # (T = 1: every length is T)
        d += ['c', 'd']
    if 'index' in case.mode and B > 1:  # (B = 1: the row has no -1 tail)
        d += ['e']
    if case.mode != 'plain' and B > nbl and R.FORMS[case.form].route[0] == 'bidir':
        d += ['f']
    return d, nbl


@pytest.mark.parametrize('case', R.CASES, ids=[c.id for c in R.CASES])
def test_defects_break_the_bound(case, switches):
    """Teeth: each applicable planted defect is at least 8 x the bound away from float64, in
    the max or in the mean, with the committed F; every f16x3 or ragged case with T >= 2 is
    caught by at least one.  The condition the F values must keep."""
    switches(case)
    B = _B(case)
    op = R.case_operands(case, B)
    (b_max, b_mean), _ = R.bound(op.ref64, op.ref32, R.path_of(case))
    defects, nbl = applicable_defects(case, B)
    for k in defects:
        got = R.DEFECTS[k](op.cell, op.xp, op.w_hh, op.b_hh, np.float64, nbl=nbl, **op.kw)
        e_max, e_mean = R.errors(got, op.ref64)
        assert e_max >= 8 * b_max or e_mean >= 8 * b_mean, (
            k, f'max {e_max:.2e} / {b_max:.2e}, mean {e_mean:.2e} / {b_mean:.2e}')
    if case.T >= 2 and (R.path_of(case) == 'f16x3' or case.mode != 'plain'):
        assert defects


# ---------------------------------------------------------------- routes
# The 37 instantiations of RNN_KERNELS (csrc/rnn.hip; the same table as INSTANCES in
# test_rnn_route.py), as (kernel, cell, H, units, wk, mode, cst, nbl, cr, kseg, nbv)
RNN_KERNELS = {('gemv', c, H, 16, 0, 0, 0, 0, 0, k, nbv)
               for c, H, k in ((1, 512, 8), (1, 512, 16), (0, 256, 8), (0, 256, 16), (0, 128, 8), (0, 64, 8))
               for nbv in (1, 2, 4)} | {
    ('bidir', 0, 64, 32, 2, 2, 0, 16, 0, 0, 0), ('bidir', 0, 64, 64, 2, 2, 0, 16, 0, 0, 0),
    ('bidir', 0, 64, 64, 2, 1, 0, 16, 0, 0, 0), ('bidir', 0, 64, 64, 4, 0, 0, 16, 0, 0, 0),
    *(('bidir', c, H, 16, 4, m, 0, 16, 0, 0, 0) for c, H in ((0, 128), (0, 256), (1, 512))
      for m in (2, 1, 0)),
    ('bidir', 0, 256, 16, 4, 2, 1, 16, 0, 0, 0), ('bidir', 0, 256, 16, 4, 2, 1, 8, 0, 0, 0),
    ('bidir', 0, 256, 8, 4, 2, 1, 16, 0, 0, 0), ('bidir', 0, 256, 8, 4, 2, 1, 16, 1, 0, 0),
    ('bidir', 1, 512, 16, 4, 2, 1, 16, 0, 0, 0), ('bidir', 1, 512, 16, 4, 2, 1, 16, 1, 0, 0)}


def test_routes_cover_every_instantiation(monkeypatch):
    """Under its own switches, on 256 CUs, every case's route is the one it names, and together
    the cases reach exactly the 37 instantiations; the `passes` cases take two passes at B =
    65 / 129 / 257 / 1025."""
    assert len(RNN_KERNELS) == 18 + 19
    seen, two_pass = set(), {}
    for case in R.CASES:
        form = R.FORMS[case.form]
        R.clear_switches(monkeypatch, form.switches)
        B = R.resolve_B(case, CUS)
        r = R.route(form, B, cus=CUS)
        coords = R.route_coords(r)
        assert coords == R.expected_coords(case, B), case.id
        assert (r.cell, r.H) == (form.cell, form.H)
        seen.add(coords[:1] + (r.cell, r.H) + coords[1:])
        if case.axis == 'passes':
            two_pass[case.form] = B
            assert r.passes == 2 and R.route(form, B - 1, cus=CUS).passes == 1
        else:
            assert r.passes == 1
    assert seen == RNN_KERNELS
    assert two_pass == {'lstm-cr': 65, 'gru256-cst': 129, 'gru128-f16': 257, 'gru64-u32': 1025}


# ---------------------------------------------------------------- the committed measurement
def test_committed_F_is_twice_the_measured_ratios():
    """profiles/rnn_range.json (a copy of what test_gpu_rnn_cases.py wrote on the MI355X) holds
    a ratio for every case, and on every path it ran on; each committed F is twice the path's
    worst ratio, rounded up to one significant digit."""
    import json
    import math
    from pathlib import Path
    table = json.loads((Path(__file__).resolve().parent.parent / 'profiles' / 'rnn_range.json').read_text())
    worst = {p: [0.0, 0.0] for p in R.F}
    for case in R.CASES:
        path = R.path_of(case)
        keys = [case.id] + ([f'{case.id}@bf16x6', f'{case.id}@f32'] if path == 'f16x3' else [])
        for k, p in zip(keys, (path, 'bf16x6', 'f32')):
            assert table[k]['path'] == p
    for e in table.values():
        for i in (0, 1):
            worst[e['path']][i] = max(worst[e['path']][i], e['ratio'][i])
            assert e['err'][i] <= R.F[e['path']][i] * e['E32'][i] + R.FLOOR / (1, 8)[i]

    def one_digit_up(x):
        unit = 10.0 ** math.floor(math.log10(x))
        return math.ceil(x / unit - 1e-9) * unit

    for p, f in R.F.items():
        assert tuple(one_digit_up(2 * w) for w in worst[p]) == f, (p, worst[p])
