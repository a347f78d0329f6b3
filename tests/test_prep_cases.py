"""What tests/test_gpu_prep.py relies on, checked without a GPU: the case table of
tests/prep_cases.py keeps every frame clear of the trim threshold (so the float32 restatement,
the float64 one and the device must agree), the named cases trim non-trivially, the mu-law
inputs stay clear of a rounding boundary, each planted defect moves the bounds of its case,
and the C ABI of csrc/prep.hip rejects bad arguments before any launch."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import prep_cases as pc
from forwardtacotron_amd import _lib

CASES = pc.cases()
MARGIN_DB = 0.01  # float32 against float64: 2048 * 2^-24 relative is 5e-4 dB, plus log10 rounding


@pytest.mark.parametrize('case', CASES, ids=lambda c: c.name)
def test_every_frame_is_clear_of_the_threshold(case):
    for v in case.items:
        db = pc.frame_db_np(pc.frame_power_np(v, case.frame_length, case.hop, np.float64))
        margin = np.abs(db + case.top_db).min()
        print(f'{case.name}: margin {margin:.4f} dB')
        assert margin >= MARGIN_DB


@pytest.mark.parametrize('case', CASES, ids=lambda c: c.name)
def test_float32_and_float64_restatements_agree(case):
    assert pc.expected_bounds(case.name, 'float32') == pc.expected_bounds(case.name, 'float64')


def test_table_covers_the_listed_shapes():
    framings = {(c.frame_length, c.hop) for c in CASES}
    assert {(2048, 512), (256, 64), (2048, 300)} <= framings
    lengths = {len(v) for c in CASES for v in c.items}
    assert {700, 1025, 2047, 12345, 30000} <= lengths
    assert {1, 3, 5} <= {len(c.items) for c in CASES}
    assert {10, 30, 60} <= {c.top_db for c in CASES}
    assert any(c.stride > max(len(v) for v in c.items) for c in CASES)
    assert any(len({len(v) for v in c.items}) > 1 for c in CASES)
    assert any(not v.any() for c in CASES for v in c.items)  # an all-zero item


def test_named_cases_trim_non_trivially():
    n = 0
    for c in CASES:
        for b in c.named:
            s, e = pc.expected_bounds(c.name, 'float64')[b]
            assert 0 < s < e < len(c.items[b]), (c.name, b, s, e)
            n += 1
    assert n >= 10


def test_edge_items():
    by = {c.name: c for c in CASES}
    # loud at sample 0: starts at 0
    assert pc.expected_bounds('ref-b3', 'float64')[0][0] == 0
    assert pc.expected_bounds('ref-edge-start', 'float64')[0][0] == 0
    # last frame non-silent with L % hop != 0: the end is the item's length, not a hop multiple
    v = by['ref-b3'].items[1]
    assert len(v) % 512 != 0 and pc.expected_bounds('ref-b3', 'float64')[1][1] == len(v)
    # all-zero: every frame ties the reference at the floor
    z = by['ref-b5'].items[2]
    assert not z.any() and pc.expected_bounds('ref-b5', 'float64')[2] == (0, len(z))
    # a quiet item beside a loud one still finds its own burst
    s, e = pc.expected_bounds('ref-b5', 'float64')[1]
    assert 8000 < s < 10500 and 17500 < e < 20000


def test_rows_plant_past_each_item():
    case = next(c for c in CASES if c.name == 'ref-b5')
    y, lengths = pc.rows(case)
    assert y.shape == (5, case.stride) and case.stride > lengths.max()
    for b, n in enumerate(lengths):
        assert (y[b, n:] == pc.PLANT).all() and np.array_equal(y[b, :n], case.items[b])


def _defect_bounds(defect, case, b):
    v = case.items[b]
    kw = dict(top_db=case.top_db, frame_length=case.frame_length, hop=case.hop)
    if defect == 'zero_pad':
        return pc.trim_bounds_np(v, pad_mode='constant', **kw)
    if defect == 'batch_reference':
        ref = max(pc.frame_power_np(u, case.frame_length, case.hop).max() for u in case.items)
        return pc.trim_bounds_np(v, ref=ref, **kw)
    if defect == 'lengths_ignored':
        return pc.trim_bounds_np(pc.rows(case)[0][b], **kw)
    if defect == 'end_not_clipped':
        return pc.trim_bounds_np(v, clip_end=False, **kw)
    if defect == 'centre_start':
        return pc.trim_bounds_np(v, centre_start=True, **kw)
    raise KeyError(defect)


@pytest.mark.parametrize('defect', sorted(pc.DEFECTS))
def test_planted_defect_changes_the_bounds(defect):
    name, b = pc.DEFECTS[defect]
    case = next(c for c in CASES if c.name == name)
    good = pc.expected_bounds(name, 'float64')[b]
    bad = _defect_bounds(defect, case, b)
    print(defect, good, bad)
    assert tuple(bad) != tuple(good)


@pytest.mark.parametrize('case', pc.prep_cases(), ids=lambda c: c.name)
def test_prep_cases_cover_the_rules(case):
    peaks, scaled = [], []
    for v in case.items:
        s, e, peak, w, q = pc.prepare_np(v, case.top_db, case.peak_norm, case.mode, case.trim)
        peaks.append(float(peak))
        scaled.append(not np.array_equal(w, v[s:e]))
        assert q.dtype == np.int64 and q.min() >= 0 and q.max() <= 2 ** case.mode[1] - 1
        if case.trim and v.any():
            assert 0 < s < e < len(v)
        if case.mode[0] == 'mu':
            pre, _ = pc.mu_law_prefloor(w, case.mode[1])
            nz = w != 0
            assert (np.abs(pre[nz] - np.round(pre[nz])) >= 1e-9).all()
    if case.name.endswith('norm-off'):
        assert peaks[0] > 1 and scaled[0]              # above 1: scaled although peak_norm is off
        assert 0 < peaks[2] < 1 and not scaled[2]
    if case.name.endswith('norm-on'):
        assert 0 < peaks[0] < 1 and scaled[0]          # below 1: scaled because peak_norm is on
    assert peaks[-1] == 0 or not case.trim             # the all-zero item
    # -1, 0 and +1 reach the labels
    unit = next(v for v in case.items if (v == 1.0).any())
    _, _, peak, w, q = pc.prepare_np(unit, case.top_db, case.peak_norm, case.mode, case.trim)
    assert peak == 1.0
    for x, want in ((-1.0, 0), (1.0, 2 ** case.mode[1] - 1)):
        assert (w == x).any() and (q[w == x] == want).all()
    assert (w == 0.0).any()


def test_label_restatement_matches_the_class_helpers():
    from forwardtacotron_amd.dsp import DSP
    x = np.concatenate([np.linspace(-1, 1, 4001), [-1.0, 0.0, 1.0]]).astype(np.float32)
    assert np.array_equal(pc.labels_np(x, ('mu', 9)),
                          DSP.encode_mu_law(x.astype(np.float64), 2 ** 9).astype(np.int64))
    for bits in (10, 16):
        assert np.array_equal(pc.labels_np(x, ('raw', bits)),
                              DSP.float_2_label(x, bits).astype(np.int64))


# --- the C ABI (no GPU: these return before any launch) --------------------------------------------

def test_abi_version_and_header():
    assert _lib.ABI_VERSION == 22
    header = Path(__file__).resolve().parent.parent / 'include' / 'ftmi.h'
    text = re.sub(r'/\*.*?\*/', '', header.read_text(), flags=re.S)
    declared = set(re.findall(r'\b(ftmi_[a-z0-9_]+)\s*\(', text))
    assert declared == set(_lib.SIGNATURES)
    lib = _lib.load()
    for name in ('ftmi_frame_power', 'ftmi_trim_bounds', 'ftmi_peak_abs', 'ftmi_prepare_audio'):
        assert name in declared and hasattr(lib, name)
    assert lib.ftmi_abi_version() == 22


F = ctypes.c_void_p(256)  # never dereferenced: validation fails first
TD = ctypes.c_double(60.0)


@pytest.mark.parametrize('call,code', [
    # null pointers
    (lambda L: L.ftmi_frame_power(None, 4096, 1, 4096, None, 2048, 512, 9, F, None), 1001),
    (lambda L: L.ftmi_frame_power(F, 4096, 1, 4096, None, 2048, 512, 9, None, None), 1001),
    (lambda L: L.ftmi_trim_bounds(None, 1, 9, 4096, None, 512, TD, F, None), 1001),
    (lambda L: L.ftmi_trim_bounds(F, 1, 9, 4096, None, 512, TD, None, None), 1001),
    (lambda L: L.ftmi_peak_abs(None, 4096, 1, 4096, F, F, None), 1001),
    (lambda L: L.ftmi_peak_abs(F, 4096, 1, 4096, None, F, None), 1001),
    (lambda L: L.ftmi_peak_abs(F, 4096, 1, 4096, F, None, None), 1001),
    (lambda L: L.ftmi_prepare_audio(None, 4096, 1, 4096, F, F, 0, 1, 9, F, 4096, F, 4096, F, None), 1001),
    (lambda L: L.ftmi_prepare_audio(F, 4096, 1, 4096, None, F, 0, 1, 9, F, 4096, F, 4096, F, None), 1001),
    (lambda L: L.ftmi_prepare_audio(F, 4096, 1, 4096, F, None, 0, 1, 9, F, 4096, F, 4096, F, None), 1001),
    (lambda L: L.ftmi_prepare_audio(F, 4096, 1, 4096, F, F, 0, 1, 9, None, 4096, F, 4096, F, None), 1001),
    (lambda L: L.ftmi_prepare_audio(F, 4096, 1, 4096, F, F, 0, 1, 9, ctypes.c_void_p(512), 4096, F, 4096, None, None), 1001),
    # odd or non-positive frame_length, hop < 1
    (lambda L: L.ftmi_frame_power(F, 4096, 1, 4096, None, 2047, 512, 9, F, None), 1001),
    (lambda L: L.ftmi_frame_power(F, 4096, 1, 4096, None, 0, 512, 9, F, None), 1001),
    (lambda L: L.ftmi_frame_power(F, 4096, 1, 4096, None, -2048, 512, 9, F, None), 1001),
    (lambda L: L.ftmi_frame_power(F, 4096, 1, 4096, None, 2048, 0, 9, F, None), 1001),
    (lambda L: L.ftmi_trim_bounds(F, 1, 9, 4096, None, 0, TD, F, None), 1001),
    # rows shorter than 2 samples
    (lambda L: L.ftmi_frame_power(F, 4096, 1, 1, None, 2048, 512, 1, F, None), 1001),
    (lambda L: L.ftmi_trim_bounds(F, 1, 1, 1, None, 512, TD, F, None), 1001),
    (lambda L: L.ftmi_peak_abs(F, 4096, 1, 1, F, F, None), 1001),
    (lambda L: L.ftmi_prepare_audio(F, 4096, 1, 1, F, F, 0, 1, 9, ctypes.c_void_p(512), 4096, F, 4096, F, None), 1001),
    # bits outside 1..16
    (lambda L: L.ftmi_prepare_audio(F, 4096, 1, 4096, F, F, 0, 1, 0, ctypes.c_void_p(512), 4096, F, 4096, F, None), 1003),
    (lambda L: L.ftmi_prepare_audio(F, 4096, 1, 4096, F, F, 0, 0, 17, ctypes.c_void_p(512), 4096, F, 4096, F, None), 1003),
    # a row stride below L, more frames than the row has, in-place rows
    (lambda L: L.ftmi_frame_power(F, 4000, 2, 4096, None, 2048, 512, 9, F, None), 1002),
    (lambda L: L.ftmi_frame_power(F, 4096, 1, 4096, None, 2048, 512, 10, F, None), 1002),
    (lambda L: L.ftmi_prepare_audio(F, 4096, 1, 4096, F, F, 0, 1, 9, ctypes.c_void_p(512), 4000, F, 4096, F, None), 1002),
    (lambda L: L.ftmi_prepare_audio(F, 4096, 1, 4096, F, F, 0, 1, 9, F, 4096, F, 4096, F, None), 1001),
])
def test_argument_errors(call, code):
    assert call(_lib.load()) == code
