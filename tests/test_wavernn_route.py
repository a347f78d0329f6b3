"""The host-only WaveRNN queries (ftmi_wavernn_route, ftmi_wr_check_folds, ftmi_wr_check_items)
against the records of what they replace: the launch loop restated in wr_cases.launches, and the
numpy row rules ops.check_wr_folds / ops.wr_unfold_packed stated before the library's checks took
over (copied here verbatim, as tests/test_route_abi.py keeps the GEMM rules).  No GPU: every call
here returns before any launch.

An entry point is handed a table its check ACCEPTS only where no device is present (it then stops
at the first device call); with a device it would launch on the placeholder pointers.  Refused
tables go to the entry points everywhere."""
import ctypes

import numpy as np
import pytest
import torch

import wr_cases as C
import wr_pack_cases as PC
from forwardtacotron_amd import _lib, ops
from forwardtacotron_amd.wavernn import WaveRNN
from test_wavernn_pack import FAKE, GOOD, _fold_table, _packed_args, _unfold

E_ARG, E_SHAPE = 1001, 1002
I32 = 2 ** 31 - 1
NO_DEVICE = not torch.cuda.is_available()


# ---------------------------------------------------------------------------------------
# the launches

def test_route_is_the_parents_launch_loop(monkeypatch):
    monkeypatch.delenv('FTMI_WR_NI', raising=False)
    for n in range(1, 101):
        assert ops.wavernn_route(n) == C.launches(n), n
    monkeypatch.setenv('FTMI_WR_NI', '1')  # read per call
    for n in range(1, 101):
        assert ops.wavernn_route(n) == C.launches(n, 1), n
    monkeypatch.setenv('FTMI_WR_NI', '2')
    assert ops.wavernn_route(93) == C.launches(93)


def test_pack_plan_reports_the_one_instance_launches(monkeypatch):
    """FTMI_WR_NI=1: the library launches <32, 1>, and the plan must say so (a plan with a launch
    rule of its own reported <16, 2>)."""
    model = WaveRNN.from_config(C.small_config(PC.FACTORS, 9))
    monkeypatch.setenv('FTMI_WR_NI', '1')
    plan = model.pack_plan(list(range(21, 56)), False, 5, 1)
    assert plan.launches == C.launches(35, 1) == [(32, 1, 0, 32), (8, 1, 32, 3)]
    assert plan.launch_steps == [55 * 6, 23 * 6]
    plan = model.pack_plan(PC.ITEMS_T, True, *PC.FOLD)
    assert plan.launches == C.launches(93, 1) == [(32, 1, 0, 32), (32, 1, 32, 32), (32, 1, 64, 29)]
    monkeypatch.delenv('FTMI_WR_NI')
    assert model.pack_plan(PC.ITEMS_T, True, *PC.FOLD).launches == C.launches(93)


def test_route_refuses_no_folds():
    lib, n = _lib.load(), ctypes.c_int32(7)
    for bad in (0, -1):
        assert lib.ftmi_wavernn_route(bad, None, 0, ctypes.byref(n)) == E_ARG
        with pytest.raises(_lib.FtmiError):
            ops.wavernn_route(bad)
    assert lib.ftmi_wavernn_route(5, None, 0, None) == E_ARG
    assert lib.ftmi_wavernn_route(5, None, 1, ctypes.byref(n)) == E_ARG
    assert lib.ftmi_wavernn_route(70, None, 0, ctypes.byref(n)) == 0 and n.value == 3  # the count alone
    buf = (ctypes.c_int32 * 8)(*([-7] * 8))
    assert lib.ftmi_wavernn_route(70, buf, 1, ctypes.byref(n)) == 0 and n.value == 3
    assert list(buf) == [16, 2, 0, 32] + [-7] * 4  # no more than capacity is written


# ---------------------------------------------------------------------------------------
# the fold rows

def _parent_fold_ok(f, L, n_out_rows, n_mel_rows, bias_row, hop):
    """ops.check_wr_folds' numpy rule before the library's check replaced it, verbatim."""
    mel0, cond0, g0, n, pb, orow = (f[:, i].astype(np.int64) for i in range(6))
    ok = ((g0 >= 0) & (n > 0) & (g0 < n) & (g0 <= 2 ** 31 - 1 - L) & (orow >= 0) & (orow < n_out_rows)
          & (pb >= 0) & (mel0 >= 0) & (mel0 + n <= n_mel_rows) & (cond0 >= 0)
          & (cond0 + (n - 1) // hop < bias_row))
    return ok


def _edges(*limits):
    """-1, 0, 1 and each limit - 1, limit, limit + 1, as far as int32 holds them."""
    v = {-1, 0, 1}
    for lim in limits:
        v |= {lim - 1, lim, lim + 1}
    return sorted(x for x in v if -2 ** 31 <= x <= I32)


def _draw(rng, n, base, *columns):
    """n rows with every field drawn from its edges, then the base row with every pair of fields
    set to every pair of their edges (most all-edges rows miss more than one rule)."""
    rows = [np.stack([rng.choice(np.asarray(c, dtype=np.int64), n) for c in columns], 1)]
    for i in range(len(columns)):
        for j in range(i + 1, len(columns)):
            a, b = np.meshgrid(columns[i], columns[j], indexing='ij')
            pairs = np.tile(np.asarray(base, dtype=np.int64), (a.size, 1))
            pairs[:, i], pairs[:, j] = a.ravel(), b.ravel()
            rows.append(pairs)
    return np.concatenate(rows, 0).astype(np.int32)


# L, n_out_rows, n_mel_rows, bias_row, hop: the argument-check shape, and limits at the end of int32
# (where g0 <= INT32_MAX - L is the only rule a row can still miss)
FOLD_LIMITS = [(7, 2, 126, 21, 6), (7, 2, I32, I32, 6)]


def _lib_check_folds(lib, t, lim):
    bad = ctypes.c_int32(-1)
    rc = lib.ftmi_wr_check_folds(t.ctypes.data, len(t), *lim, ctypes.byref(bad))
    return rc, bad.value


@pytest.mark.parametrize('lim', FOLD_LIMITS)
def test_fold_check_is_the_rule_it_replaces(lim):
    L, n_out, n_mel, bias_row, hop = lim
    lib = _lib.load()
    rng = np.random.Generator(np.random.PCG64(2207))
    g0s = sorted(set(_edges(n_mel) + [I32 - L - 1, I32 - L, I32 - L + 1]))
    # mel_row0, cond_row0, g0, n_rows, philox_b, out_row (k0, k1 are not checked)
    base = [GOOD[k] for k in _lib.WR_FOLD_COLS[:6]]
    rows = _draw(rng, 2000, base, _edges(n_mel), _edges(bias_row), g0s, _edges(n_mel), _edges(I32), _edges(n_out))
    rows = np.concatenate([rows, np.zeros((len(rows), 2), np.int32)], 1)
    good = _fold_table([GOOD])
    assert _parent_fold_ok(good, *lim).all()
    verdicts = []
    for r in rows:
        t = np.ascontiguousarray(np.concatenate([good, r[None]], 0))
        assert t.ctypes.data % 16 == 0
        ok = _parent_fold_ok(t, *lim)
        want = (0, -1) if ok.all() else (E_SHAPE, int(np.flatnonzero(~ok)[0]))
        assert _lib_check_folds(lib, t, lim) == want, r.tolist()
        if want[0] or NO_DEVICE:
            a = _packed_args(folds=t.ctypes.data, L=L, n_out_rows=n_out, n_mel_rows=n_mel,
                             bias_row=bias_row, hop=hop)
            rc = lib.ftmi_wavernn_packed(ctypes.byref(a), None)
            assert (rc == E_SHAPE) == bool(want[0]), (r.tolist(), rc)
        if want[0]:
            with pytest.raises(ValueError, match='fold descriptor 1 out of range'):
                ops.check_wr_folds(t, *lim)
        else:
            ops.check_wr_folds(t, *lim)
        verdicts.append(want[0])
    assert min(verdicts.count(0), verdicts.count(E_SHAPE)) >= 20, 'both verdicts must occur'
    # the first refused row of one long table
    t = np.ascontiguousarray(np.concatenate([good, rows], 0))
    ok = _parent_fold_ok(t, *lim)
    assert _lib_check_folds(lib, t, lim) == (E_SHAPE, int(np.flatnonzero(~ok)[0]))
    assert _lib_check_folds(lib, np.ascontiguousarray(t[ok]), lim) == (0, -1)


def test_fold_check_arguments():
    lib, t = _lib.load(), _fold_table([GOOD])
    assert lib.ftmi_wr_check_folds(None, 1, 7, 2, 126, 21, 6, None) == E_ARG
    assert lib.ftmi_wr_check_folds(t.ctypes.data, 0, 7, 2, 126, 21, 6, None) == E_ARG
    assert lib.ftmi_wr_check_folds(t.ctypes.data, 1, 7, 2, 126, 21, 0, None) == E_ARG
    assert lib.ftmi_wr_check_folds(t.ctypes.data, 1, 7, 2, 126, 21, 6, None) == 0
    assert lib.ftmi_wr_check_folds(t.ctypes.data, 1, 7, 0, 126, 21, 6, None) == E_SHAPE  # no index asked for


# ---------------------------------------------------------------------------------------
# the item rows

def _parent_item_ok(it, F, L, target, overlap, batched, fade_len, out_len):
    """ops.wr_unfold_packed's numpy rule before the library's check replaced it, verbatim; its
    out_len was max(out_offset + wave_len) by construction, here a limit of its own (the last
    term, which is ftmi_wr_unfold_packed's)."""
    r0, nf, wl, off = (it[:, i].astype(np.int64) for i in range(4))
    ok = (r0 >= 0) & (nf > 0) & (r0 + nf <= F) & (wl > 0) & (wl >= fade_len) & (off >= 0)
    ok &= (wl <= nf * (target + overlap) + overlap) if batched else ((nf == 1) & (wl <= L))
    return ok & (off + wl <= out_len)


N_ROWS, L_ITEM, TARGET, OVERLAP, OUT_LEN = 5, 7, 5, 1, 100


def _lib_check_items(lib, it, n_rows, batched, fade, out_len):
    bad = ctypes.c_int32(-1)
    rc = lib.ftmi_wr_check_items(it.ctypes.data, len(it), n_rows, L_ITEM, TARGET, OVERLAP, batched, fade,
                                 out_len, ctypes.byref(bad))
    return rc, bad.value


@pytest.mark.parametrize('batched', [1, 0])
@pytest.mark.parametrize('fade', [0, 20])
def test_item_check_is_the_rule_it_replaces(batched, fade):
    lib = _lib.load()
    rng = np.random.Generator(np.random.PCG64(2208 + 2 * batched + fade))
    stride = TARGET + OVERLAP
    waves = _edges(L_ITEM, 20, *[k * stride + OVERLAP for k in range(1, N_ROWS + 2)], OUT_LEN)
    rows = _draw(rng, 1500, [0, 4, 25, 0] if batched else [0, 1, 7, 0], _edges(N_ROWS), _edges(N_ROWS), waves,
                 _edges(OUT_LEN, OUT_LEN - 20))
    cfg = (N_ROWS, L_ITEM, TARGET, OVERLAP, batched, fade, OUT_LEN)
    # the good row in front: 4 folds hold the 20-sample fade; no unbatched row of 7 samples does,
    # so there every row stands alone (and is refused)
    good = None if fade and not batched else np.asarray([[0, 4, 25, 0] if batched else [0, 1, 7, 0]], dtype=np.int32)
    assert good is None or _parent_item_ok(good, *cfg).all()
    verdicts = []
    for r in rows:
        it = np.ascontiguousarray(r[None] if good is None else np.concatenate([good, r[None]], 0))
        assert it.ctypes.data % 16 == 0
        ok = _parent_item_ok(it, *cfg)
        want = (0, -1) if ok.all() else (E_SHAPE, int(np.flatnonzero(~ok)[0]))
        assert _lib_check_items(lib, it, N_ROWS, batched, fade, OUT_LEN) == want, r.tolist()
        if want[0] or NO_DEVICE:
            rc = _unfold(lib, it, n_rows=N_ROWS, L=L_ITEM, target=TARGET, overlap=OVERLAP, batched=batched,
                         fade=fade, out_len=OUT_LEN)
            assert (rc == E_SHAPE) == bool(want[0]), (r.tolist(), rc)
        verdicts.append(want[0])
    if good is not None:
        assert min(verdicts.count(0), verdicts.count(E_SHAPE)) >= 20, 'both verdicts must occur'
    # ftmi_wr_unfold is one item from row 0 of its own B rows: all of them batched, fold 0 alone
    # unbatched (it reads no other row, whatever B); out_len = wave_len
    for B, wave_len in sorted({(int(r[1]), int(r[2])) for r in rows}):
        it = np.asarray([[0, B if batched else 1, wave_len, 0]], dtype=np.int32)
        rc, _ = _lib_check_items(lib, it, B, batched, fade, wave_len)
        assert rc == (0 if _parent_item_ok(it, B, L_ITEM, TARGET, OVERLAP, batched, fade, wave_len).all() else E_SHAPE)
        if B <= 0 or wave_len <= 0:  # its own argument errors come first
            want = E_ARG
        elif rc or NO_DEVICE:
            want = rc
        else:
            continue
        got = lib.ftmi_wr_unfold(FAKE, B, L_ITEM, TARGET, OVERLAP, batched, 0, 512, wave_len, fade, FAKE, None)
        assert (got == want) if want else (got not in (E_ARG, E_SHAPE)), (B, wave_len, got, want)


def test_item_check_arguments_and_the_bindings_message():
    it = np.asarray([[0, 3, 19, 0], [3, 3, 19, 19]], dtype=np.int32)
    lib = _lib.load()
    assert lib.ftmi_wr_check_items(None, 1, 5, 7, 5, 1, 1, 0, 100, None) == E_ARG
    assert lib.ftmi_wr_check_items(it.ctypes.data, 0, 5, 7, 5, 1, 1, 0, 100, None) == E_ARG
    assert lib.ftmi_wr_check_items(it.ctypes.data, 2, 5, 7, 5, 1, 1, 0, 100, None) == E_SHAPE
    assert lib.ftmi_wr_check_items(it.ctypes.data, 2, 6, 7, 5, 1, 1, 0, 100, None) == 0
    with pytest.raises(ValueError, match='item 1 out of range'):  # ops.wr_unfold_packed's check
        ops._check_wr_table('ftmi_wr_check_items', 'item', _lib.WR_ITEM_COLS, it, 5, 7, 5, 1, 1, 0, 100)
    with pytest.raises(_lib.FtmiError):  # not a row
        ops._check_wr_table('ftmi_wr_check_items', 'item', _lib.WR_ITEM_COLS, it[:0], 5, 7, 5, 1, 1, 0, 100)
