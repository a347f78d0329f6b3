"""Every recurrence kernel form against a float64 reference (tests/rnn_cases.py): each of the
19 rnn_bidir_kernel and 18 rnn_gemv_kernel instantiations with `lengths` (pack / pad semantics,
the reverse restart at len - 1, pad_value), `index` / `xp_zero` (the length-regulator map) and
both, T = 1, 2, 3 (the early exits of the 3-step rotation, the clamped prefetch, the step-0/1
rule of the tag), W_hh rows at 2^-6 .. 2^5 with gates pinned at 0 / 1 and h at 0 / +-1, 66 and
301 steps, launches of several passes (chunk0 > 0) with `index` and `lengths`, a strided xp and
the f16 boundary 65504 of W_hh.

The bound is rnn_cases.bound: F x the error of the same recurrence in float32 on the host, plus
four ulps; test_rnn_cases.py shows on the host that a kernel that dropped the f16 tail of h or
of W_hh, ignored a length, or read another chunk's lengths / index rows breaks it by 8 x or
more.  Every run's ratios go to rnn_range.json beside the accuracy records of
test_gpu_accuracy.py (table in DESIGN.md section 6)."""
import json

import numpy as np
import pytest
import torch

import rnn_cases as R

pytestmark = pytest.mark.gpu

_TABLE = {}


def _record_range(key, entry):
    from test_gpu_accuracy import _record
    _TABLE[key] = entry
    print(key, json.dumps(entry))
    _record('rnn_range', dict(sorted(_TABLE.items())), fname='rnn_range.json')


def _device_kw(kw):
    out = dict(kw)
    for k in ('index', 'xp_zero'):
        if k in out:
            out[k] = torch.tensor(out[k]).cuda()
    if 'lengths' in out:  # host-side, as pack_padded_sequence takes them
        out['lengths'] = torch.tensor(out['lengths'])
    return out


def _run(form, op, mma, w_hh=None, xp=None):
    """One ops.rnn_bidir call on the case's operands -> (y, status word)."""
    from forwardtacotron_amd import ops
    st = ops.status_word('cuda')
    st.zero_()
    xp = torch.tensor(op.xp).cuda() if xp is None else xp
    w = torch.tensor(op.w_hh if w_hh is None else w_hh).cuda()
    b = None if op.b_hh is None else torch.tensor(op.b_hh).cuda()
    y = ops.rnn_bidir(form.cell, xp, form.H, w, b, T=op.T, check=True, mma=mma, spread=form.spread,
                      **_device_kw(op.kw))
    torch.cuda.synchronize()
    return y.cpu().numpy(), int(st.item())


def _held(key, got, status, op, path, ref64=None, ref32=None):
    """Status 0 (no range flag, no timeout), shape, finiteness, padded frames exactly pad_value,
    the bound against float64; the ratios are recorded before anything is asserted on them."""
    ref64 = op.ref64 if ref64 is None else ref64
    (b_max, b_mean), (e32_max, e32_mean) = R.bound(ref64, op.ref32 if ref32 is None else ref32, path)
    assert status == 0, f'status word {status}'
    assert got.shape == ref64.shape and got.dtype == np.float32
    assert np.isfinite(got).all()
    live = R.live_mask(op)
    assert (got[~live] == np.float32(op.kw.get('pad_value', 0.0))).all()
    e_max, e_mean = R.errors(got, ref64)
    _record_range(key, dict(path=path, E32=[e32_max, e32_mean], err=[e_max, e_mean],
                            ratio=[e_max / e32_max, e_mean / e32_mean],
                            over_floor=[max(0.0, e_max - R.FLOOR) / e32_max,
                                        max(0.0, e_mean - R.FLOOR / 8) / e32_mean]))
    assert e_max <= b_max, f'max |err| {e_max:.3e} > {b_max:.3e} (E32 {e32_max:.3e})'
    assert e_mean <= b_mean, f'mean |err| {e_mean:.3e} > {b_mean:.3e} (E32 {e32_mean:.3e})'
    return b_max, b_mean


@pytest.mark.parametrize('case', R.CASES, ids=[c.id for c in R.CASES])
def test_rnn_case(case, monkeypatch):
    """One row of rnn_cases.CASES: the route is the form the case names, then the kernel against
    float64 under the case's switches (every other FTMI_RNN_* switch unset)."""
    form = R.FORMS[case.form]
    R.clear_switches(monkeypatch, form.switches)
    B = R.resolve_B(case, cus=0)  # the device's own CU count
    r = R.route(form, B, cus=0)
    assert R.route_coords(r) == R.expected_coords(case, B)
    if case.axis == 'passes':
        assert r.passes >= 2
    op = R.case_operands(case, B)
    path = R.path_of(case)
    got, status = _run(form, op, form.mma)
    bounds = {path: (got, _held(case.id, got, status, op, path))}
    if path != 'f16x3':
        return
    # the same operands on the two other matrix paths, which share nothing with f16x3 past the
    # operand fetch: each within its own bound, each pair within the sum of the two
    for mma in (1, 0):
        other = R.PATH_OF_MMA[mma]
        assert R.route(form, B, mma=mma, cus=0).mode == mma
        y, status = _run(form, op, mma)
        bounds[other] = (y, _held(f'{case.id}@{other}', y, status, op, other))
    names = sorted(bounds)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            d_max, d_mean = R.errors(bounds[a][0], bounds[b][0].astype(np.float64))
            assert d_max <= bounds[a][1][0] + bounds[b][1][0], (a, b, d_max)
            assert d_mean <= bounds[a][1][1] + bounds[b][1][1], (a, b, d_mean)


@pytest.mark.parametrize('case_id', ['form-lstm-cr-index+lengths', 'form-gru256-u8-cr-lengths',
                                     'form-gemv-gru256-k16-B3-index+lengths'])
def test_strided_xp_is_the_contiguous_call(case_id, monkeypatch):
    """xp as a column slice of a wider tensor (row stride above 2 G H, an offset of 4 floats;
    the columns around it hold 1e30): bit for bit the result of the contiguous call."""
    case = R.CASE_BY_ID[case_id]
    form = R.FORMS[case.form]
    R.clear_switches(monkeypatch, form.switches)
    op = R.case_operands(case, case.B)
    C = op.xp.shape[2]
    wide = torch.full((op.B, op.xp.shape[1], C + 12), 1e30, device='cuda')
    view = wide[:, :, 4:4 + C]
    view.copy_(torch.tensor(op.xp))
    assert not view.is_contiguous() and view.stride(1) == C + 12
    want, s0 = _run(form, op, form.mma)
    got, s1 = _run(form, op, form.mma, xp=view)
    assert (s0, s1) == (0, 0)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    _held(f'strided-{case_id}', got, s1, op, R.path_of(case))


@pytest.mark.parametrize('form_name', ['gru256-cst', 'gru64-u64'])
def test_whh_f16_boundary(form_name, monkeypatch):
    """A W_hh entry of exactly 65504, the largest f16, is in range on the f16x3 recurrence
    (status bit 1 stays clear, the result within the bound: the entry's update gate saturates in
    the reference too); the next float up sets bit 1.  On a form of several workgroups per group
    and on the one-workgroup U-64 form."""
    from forwardtacotron_amd import ops
    form = R.FORMS[form_name]
    R.clear_switches(monkeypatch, form.switches)
    B, T, H = 5, 3, form.H
    assert R.route_coords(R.route(form, B, cus=0)) == form.route
    op = R.operands(form.cell, H, B, T, 'plain', 'rows', 'batch')
    w = op.w_hh.copy()
    w[0, H + 3, 7] = 65504.0  # forward direction, the update gate of unit 3, from h[7]
    ref64 = R.recur_ref(form.cell, op.xp, w, op.b_hh, np.float64)
    ref32 = R.recur_ref(form.cell, op.xp, w, op.b_hh, np.float32)
    assert np.isfinite(ref64).all() and R.errors(ref32, ref64)[0] <= R.E32_CAP
    assert np.abs(ref64 - op.ref64)[:, 1:, 3].max() > 0.01  # the entry matters
    got, status = _run(form, op, 2, w_hh=w)
    assert status & ops.STATUS_WHH_RANGE == 0
    _held(f'boundary-{form_name}', got, status, op, 'f16x3', ref64, ref32)
    w[0, H + 3, 7] = np.nextafter(np.float32(65504.0), np.float32(np.inf))
    _, status = _run(form, op, 2, w_hh=w)
    assert status & ops.STATUS_WHH_RANGE
