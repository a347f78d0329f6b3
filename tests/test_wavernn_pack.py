"""CPU side of the packed WaveRNN launches (tests/test_gpu_wavernn_pack.py): WaveRNN.pack_plan
against the oracle's folding, the defects the GPU tests exist to catch — planted in the oracle
only (tests/wr_pack_cases.py) — and the argument checks of ftmi_wavernn_packed /
ftmi_wr_unfold_packed, which return before any launch."""
import ctypes

import numpy as np
import pytest
import torch

import wr_cases as C
import wr_pack_cases as PC
from forwardtacotron_amd import _lib, ops
from forwardtacotron_amd.wavernn import WaveRNN
from oracle import wr_torch_cpu as wr

COLS = {n: i for i, n in enumerate(_lib.WR_FOLD_COLS)}


@pytest.fixture(scope='module')
def model():
    return WaveRNN.from_config(C.small_config(PC.FACTORS, 9))  # on the CPU: pack_plan needs no device


def _positions(T, target, overlap):
    """fold_with_overlap on the utterance's own indices 1 .. T hop: 0 marks a padded position."""
    idx = torch.arange(1, T * PC.HOP + 1, dtype=torch.float64).view(1, -1, 1)
    return wr.fold_with_overlap(idx, target, overlap)[:, :, 0].numpy().astype(np.int64)


# lengths, (target, overlap), what the case is there for
BATCHED = [
    ((27,), (5, 1), 'one utterance only'),
    ((21, 27, 45), (5, 1), 'utterances straddle both launch boundaries; one ends inside an instance'),
    ((45, 21, 45), (200, 10), 'a one-fold utterance between longer ones'),
    ((33, 33, 21), (20, 5), 'one launch, an uneven instance split (11 + 10)'),
]


@pytest.mark.parametrize('lengths,fold,why', BATCHED)
def test_pack_plan_batched_matches_the_oracles_folding(model, lengths, fold, why):
    target, overlap = fold
    plan = model.pack_plan(lengths, True, target, overlap)
    f = plan.folds
    assert f.dtype == np.int32 and f.shape[1] == 8 and plan.order == list(range(len(lengths)))
    assert plan.L == target + 2 * overlap and plan.launch_steps is None
    row = mel0 = cond0 = off = 0
    for k, T in enumerate(lengths):
        want = _positions(T, target, overlap)  # (folds, L)
        nf = want.shape[0]
        assert nf == PC.fold_count(T, target, overlap) == model._fold_shape(T * PC.HOP, 1, True, target, overlap)[0]
        assert plan.rows(k) == slice(row, row + nf)
        d = f[row:row + nf]
        g = d[:, COLS['g0']][:, None] + np.arange(plan.L)[None, :]
        real = g < d[:, COLS['n_rows']][:, None]
        assert np.array_equal(np.where(real, g + 1, 0), want), why  # real and padded positions
        assert d[:, COLS['philox_b']].tolist() == list(range(nf))   # restarts per utterance
        assert d[:, COLS['out_row']].tolist() == list(range(row, row + nf))
        assert set(d[:, COLS['mel_row0']].tolist()) == {mel0} and set(d[:, COLS['cond_row0']].tolist()) == {cond0}
        assert set(d[:, COLS['n_rows']].tolist()) == {T * PC.HOP}
        assert plan.items[k].tolist() == [row, nf, (T - 1) * PC.HOP, off]
        assert (plan.item_of_fold[row:row + nf] == k).all()
        row, mel0, cond0, off = row + nf, mel0 + T * PC.HOP, cond0 + T, off + (T - 1) * PC.HOP
    assert f.shape[0] == row
    assert plan.launches == C.launches(row)
    ops.check_wr_folds(plan.table([1] * len(lengths)), plan.L, row, mel0, cond0, PC.HOP)


def test_the_gpu_shapes_reach_what_they_claim(model):
    """21 + 27 + 45 folds: launches of 32, 32, 29, all <16, 2>; utterance 0 ends inside the
    second instance of launch 0; utterances 1 and 2 each cross a launch boundary; the 27- and
    45-fold utterances alone take <16, 2> for their first 32 folds too."""
    plan = model.pack_plan(PC.ITEMS_T, True, *PC.FOLD)
    assert [PC.fold_count(T, *PC.FOLD) for T in PC.ITEMS_T] == [21, 27, 45]
    assert plan.launches == [(16, 2, 0, 32), (16, 2, 32, 32), (16, 2, 64, 29)]
    assert C.instance_split(32, 2) == [16, 16] and 16 < 21 < 32
    ends = np.cumsum([21, 27, 45])
    assert ends[0] < 32 < ends[1] < 64 < ends[2]
    assert C.launches(27) == [(16, 2, 0, 27)] and C.launches(45)[0] == (16, 2, 0, 32)
    # every utterance's last fold has exactly one padded position
    for T in PC.ITEMS_T:
        assert (_positions(T, *PC.FOLD) == 0).sum(axis=1).tolist() == [0] * (T - 1) + [1]


def test_pack_plan_unbatched_sorts_longest_first(model):
    lengths = (21, 33, 30, 33)
    plan = model.pack_plan(lengths, False, 5, 1)
    assert plan.order == [1, 3, 2, 0]  # stable among equals
    f = plan.folds
    assert f[:, COLS['n_rows']].tolist() == [198, 198, 180, 126] and plan.L == 198
    assert f[:, COLS['g0']].tolist() == [0] * 4 and f[:, COLS['philox_b']].tolist() == [0] * 4
    assert f[:, COLS['out_row']].tolist() == [0, 1, 2, 3]
    assert f[:, COLS['mel_row0']].tolist() == [0, 198, 396, 576]
    assert f[:, COLS['cond_row0']].tolist() == [0, 33, 66, 96]
    assert plan.launches == C.launches(4) == [(8, 2, 0, 4)] and plan.launch_steps == [198]
    assert [plan.rows(i) for i in range(4)] == [slice(3, 4), slice(0, 1), slice(2, 3), slice(1, 2)]
    assert plan.items[:, 2].tolist() == [(lengths[i] - 1) * PC.HOP for i in plan.order]
    # 35 rows: the second launch runs its own longest row
    plan = model.pack_plan(list(range(21, 56)), False, 5, 1)
    assert plan.launches == C.launches(35) and plan.launch_steps == [55 * 6, 23 * 6]
    # keys: low word, high word, per utterance in the caller's order
    t = model.pack_plan((21, 30), False, 5, 1).table([5, 2 ** 40 + 7])
    assert t.view(np.uint32)[:, 6:].tolist() == [[7, 256], [5, 0]]


def test_pack_plan_refuses_what_cannot_run(model):
    with pytest.raises(ValueError):
        model.pack_plan([], True, 5, 1)
    with pytest.raises(ValueError):
        model.pack_plan([21, 1], True, 5, 1)
    with pytest.raises(ValueError):  # 126 samples do not reach one fold of 11000 + 2 * 550
        model.pack_plan([21], True, 11000, 550)
    plan = model.pack_plan((21, 27), True, 5, 1)
    bad = plan.table([1, 2])
    bad[3, COLS['out_row']] = 48
    with pytest.raises(ValueError, match='fold descriptor 3'):
        ops.check_wr_folds(bad, plan.L, 48, 48 * 6, 48, 6)


def test_one_utterance_api_is_unchanged(model):
    with pytest.raises(ValueError, match='ONE utterance'):
        model._fold_shape(126, 2, True, 5, 1)
    assert model._fold_shape(126, 2, False, 5, 1) == (2, 126)


# ---------------------------------------------------------------------------------------
# discriminating power (the oracle only)

@pytest.mark.parametrize('bits', [9, None])
def test_bounds_and_a_fold_that_reads_on_is_caught(bits):
    """Defect (a): only the last fold of utterances 0 and 1 has a position past the end; reading
    the next utterance's first row there moves that step's logits by more than 10 bounds."""
    for i in range(3):
        l64 = PC.oracle(bits, i)
        d, b = PC.drift(bits, i), PC.bound(bits, i)
        assert 0 < d < 5e-5 and b <= C.existing_bar(l64), (i, d, b)
        bad = PC.oracle(bits, i, torch.float64, 'reads_next_item')
        if i == 2:  # nothing lies behind the last utterance: padding either way
            assert np.array_equal(bad, l64)
            continue
        assert np.array_equal(bad[:-1], l64[:-1]) and np.array_equal(bad[-1, :-1], l64[-1, :-1])
        ratio = float(np.abs(bad[-1, -1] - l64[-1, -1]).max()) / b
        assert ratio > 10, (bits, i, ratio)


@pytest.mark.parametrize('bits', [8, 4, None])
def test_a_global_fold_word_or_a_shared_key_moves_the_draws(bits):
    """Defects (b) and (c) on utterance 1 (rows 21 .. 47 of the table): drawing with fold words
    21 + b, or with utterance 0's key, changes its samples; utterance 0 cannot see (b)."""
    l64 = np.asarray(PC.oracle(bits, 1))
    draw = PC.mol_draws if bits is None else PC.gumbel_draws
    good = draw(l64, PC.SEEDS[1])
    assert np.array_equal(good, draw(l64, PC.SEEDS[1], word0=0))
    glob = draw(l64, PC.SEEDS[1], word0=21)
    shared = draw(l64, PC.SEEDS[0])
    n = good.size
    assert (glob != good).sum() > 0.2 * n, (glob != good).sum()
    assert (shared != good).sum() > 0.2 * n, (shared != good).sum()
    l0 = np.asarray(PC.oracle(bits, 0))
    assert np.array_equal(draw(l0, PC.SEEDS[0], word0=0), draw(l0, PC.SEEDS[0]))


def test_every_defect_is_covered():
    assert sorted(PC.DEFECTS) == ['first_items_key', 'global_fold_word', 'reads_next_item']


# ---------------------------------------------------------------------------------------
# argument checks (no GPU: they return before any launch)

FAKE = 256  # never dereferenced: validation fails first


def _packed_args(**over):
    a = _lib.WaveRNNPackedArgs()
    for n in ('w_hh1', 'w_hh2', 'w_ih2a', 'w_fc1a', 'w_fc2a', 'w_fc3', 'b_fc3', 'b_hh1', 'b_hh2',
              'u1', 'u2', 'v1', 'wm', 'cond', 'mel', 'samples', 'workspace', 'folds'):
        setattr(a, n, FAKE)
    a.n_folds, a.L, a.n_out_rows, a.n_mel_rows, a.bias_row, a.hop = 2, 7, 2, 126, 21, 6
    a.n_classes, a.mol = 512, 0
    a.rnn_dims, a.fc_dims, a.feat_dims, a.aux_dims = 512, 512, 80, 32
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _fold_table(rows):
    t = np.zeros((len(rows), 8), dtype=np.int32)
    for i, r in enumerate(rows):
        for k, v in r.items():
            t[i, COLS[k]] = v
    return t


GOOD = dict(mel_row0=0, cond_row0=0, g0=0, n_rows=126, philox_b=0, out_row=0)


def test_wavernn_packed_argument_errors():
    lib = _lib.load()
    assert lib.ftmi_wavernn_packed(None, None) == 1001
    assert lib.ftmi_wavernn_packed(ctypes.byref(_lib.WaveRNNPackedArgs()), None) == 1001
    assert lib.ftmi_wavernn_packed(ctypes.byref(_packed_args(folds=None)), None) == 1001
    assert lib.ftmi_wavernn_packed(ctypes.byref(_packed_args(n_folds=0)), None) == 1001
    assert lib.ftmi_wavernn_packed(ctypes.byref(_packed_args(samples=None)), None) == 1001
    assert lib.ftmi_wavernn_packed(ctypes.byref(_packed_args(rnn_dims=256)), None) == 1003
    assert lib.ftmi_wavernn_packed(ctypes.byref(_packed_args(n_classes=1024)), None) == 1003
    assert lib.ftmi_wavernn_packed(ctypes.byref(_packed_args(mol=1, n_classes=512)), None) == 1003
    assert lib.ftmi_wavernn_packed(ctypes.byref(_packed_args(folds=FAKE + 4)), None) == 1004
    assert lib.ftmi_wavernn_packed(ctypes.byref(_packed_args(mel=FAKE + 8)), None) == 1004
    steps = (ctypes.c_int32 * 1)(8)  # more steps than a row holds
    a = _packed_args(launch_steps=ctypes.cast(steps, ctypes.c_void_p).value)
    assert lib.ftmi_wavernn_packed(ctypes.byref(a), None) == 1002


@pytest.mark.parametrize('row', [dict(g0=-1), dict(n_rows=0), dict(n_rows=-5), dict(out_row=-1),
                                 dict(out_row=2), dict(g0=126), dict(mel_row0=1), dict(mel_row0=-1),
                                 dict(cond_row0=1), dict(cond_row0=-1), dict(philox_b=-1)])
def test_wavernn_packed_checks_a_host_table(row):
    """A host table is read back and every row checked before anything is launched."""
    lib = _lib.load()
    t = _fold_table([GOOD, {**GOOD, 'out_row': 1, **row}])
    assert t.ctypes.data % 16 == 0
    a = _packed_args(folds=t.ctypes.data)
    assert lib.ftmi_wavernn_packed(ctypes.byref(a), None) == 1002
    with pytest.raises(ValueError):  # the binding's check of a table bound for the device
        ops.check_wr_folds(t, 7, 2, 126, 21, 6)


def _unfold(lib, items, n_rows=5, L=7, target=5, overlap=1, batched=1, mu_law=0, nc=512, fade=0,
            out_len=100, samples=FAKE, out=FAKE):
    ptr = items if isinstance(items, (int, type(None))) else items.ctypes.data
    return lib.ftmi_wr_unfold_packed(samples, n_rows, L, ptr, 1 if isinstance(items, (int, type(None))) else len(items),
                                     target, overlap, batched, mu_law, nc, fade, out, out_len, None)


def test_unfold_packed_argument_errors():
    lib = _lib.load()
    assert _unfold(lib, None) == 1001
    assert _unfold(lib, FAKE, samples=None) == 1001
    assert _unfold(lib, FAKE, out_len=0) == 1001
    assert _unfold(lib, FAKE, L=8) == 1002            # L != target + 2 overlap
    assert _unfold(lib, FAKE, mu_law=1, nc=30) == 1003
    assert _unfold(lib, FAKE + 4) == 1004
    good = [0, 3, 19, 0]  # 3 folds: up to 3 * 6 + 1 samples
    for bad in ([0, 3, 20, 0],     # wave_len > folds * stride + overlap
                [3, 3, 19, 0],     # rows past the matrix
                [0, 0, 19, 0], [-1, 3, 19, 0], [0, 3, 0, 0],
                [0, 3, 19, 82],    # past out_len
                [0, 3, 19, -1]):
        it = np.asarray([good, bad], dtype=np.int32)
        assert it.ctypes.data % 16 == 0
        assert _unfold(lib, it) == 1002, bad
    it = np.asarray([good], dtype=np.int32)
    assert _unfold(lib, it, fade=20) == 1002          # wave_len < fade_len
    assert _unfold(lib, np.asarray([[0, 2, 5, 0]], dtype=np.int32), batched=0) == 1002  # unbatched: one row
    assert _unfold(lib, np.asarray([[0, 1, 8, 0]], dtype=np.int32), batched=0) == 1002  # wave_len > L


def test_header_and_binding_still_agree():
    import re
    from pathlib import Path
    text = re.sub(r'/\*.*?\*/', '', (Path(__file__).resolve().parent.parent / 'include' / 'ftmi.h').read_text(),
                  flags=re.S)
    declared = sorted(set(re.findall(r'\b(ftmi_[a-z0-9_]+)\s*\(', text)))
    assert declared == sorted(_lib.SIGNATURES)
    assert {'ftmi_wavernn_packed', 'ftmi_wr_unfold_packed'} <= set(declared)
    assert _lib.load().ftmi_abi_version() == _lib.ABI_VERSION == 22
    assert ctypes.sizeof(_lib.WaveRNNPackedArgs) == 22 * 8 + 12 * 4
