"""What tests/test_gpu_dsp_configs.py relies on, checked without a GPU: every configuration of
tests/dsp_cases.py has the filterbank shape the kernels assume (the oracle's filters, at most
two per bin, none empty), the restatements equal the oracle, every NNLS parity case sits in the
iteration band that decides which history the device solver runs with, and the comparisons
used on the device reject each planted defect."""
import ctypes

import numpy as np
import pytest

import dsp_cases as dc
from forwardtacotron_amd import _lib
from forwardtacotron_amd import dsp as G
from oracle import dsp_oracle as D

IDS = [c.id for c in dc.CONFIGS]


@pytest.mark.parametrize('cid', IDS)
def test_filterbank_and_plan(cid):
    c = dc.BY_ID[cid]
    A = dc.filters(c)
    assert np.array_equal(G.mel_basis(c.sr, c.n_fft, c.mels, c.fmin, c.fmax), A)
    assert ((A > 0).sum(axis=0) <= 2).all()          # a bin feeds at most two filters
    assert (A > 0).any(axis=1).all()                 # no empty filter
    plan = G.DspPlan(c.sr, c.n_fft, c.hop, c.win, c.mels, c.fmin, c.fmax, 'cpu')
    assert plan.nnls_cols == dc.nnls_cols(c) == D.MAX_MEM_BLOCK // (dc.n_bins(c) * 4)
    assert plan.nb == dc.n_bins(c) and plan.frames(len(dc.single(cid))) == dc.FRAMES
    w = dc.window(c)
    assert np.array_equal(plan.window.numpy(), w) and np.array_equal(w, D.pad_center(D.get_window(c.win), c.n_fft))
    A2, pinv, inv_L = dc.fista_consts(c)
    assert np.array_equal(plan.pinv.numpy(), pinv) and plan.inv_L == inv_L


def test_table_reaches_what_it_names():
    by = dc.BY_ID
    assert {c.n_fft for c in dc.CONFIGS} >= {64, 256, 512, 2048, 4096}
    assert by['A'].win < by['A'].n_fft and (by['A'].n_fft - by['A'].win) % 2 == 0
    assert (by['B'].n_fft - by['B'].win) % 2 == 1                      # the odd pad split
    assert 2 * by['B'].n_fft * 16 == 64 * 1024 and 2 * by['C'].n_fft * 16 == 128 * 1024
    assert by['C'].n_fft % by['C'].hop and by['E'].n_fft % by['E'].hop
    assert by['D'].n_fft // 2 < 256                                    # fewer butterflies than threads
    assert by['E'].hop > by['E'].n_fft // 2 and by['G'].hop > by['G'].win
    nj = {cid: (dc.n_bins(by[cid]) + 63) // 64 for cid in dc.MEL_IDS}  # ftmi_mel_nnls' dispatch
    assert (nj['D'] <= 3 and 3 < nj['A'] <= 5 and 9 < nj['B'] <= 17 and nj['C'] > 17)
    assert by['C'].mels > 128 and all(by[k].mels <= 128 for k in 'ABDE')
    assert {dc.nnls_cols(by[k]) for k in 'ABC'} == {255, 63, 31}
    assert dc.SHORT_ITEM < by['B'].n_fft // 2 and 2 * (dc.SHORT_ITEM - 1) < by['C'].n_fft // 2
    # the window sum-square has exact zeros at G (samples no window reaches); at E it dips
    # between two frames (2 sin^4(28 pi / 256) = 0.026) but stays positive
    assert (dc.cropped_wss(by['G'], dc.FRAMES) == 0).any()
    wss_e = dc.cropped_wss(by['E'], dc.FRAMES)
    assert 0 < wss_e.min() < 0.03


@pytest.mark.parametrize('cid', IDS)
def test_inputs(cid):
    c = dc.BY_ID[cid]
    rows, lengths, frames, items = dc.batch(cid)
    assert rows.shape[0] == 3 and list(frames) == [7, 4, 1]
    assert [1 + len(v) // c.hop for v in items] == [7, 4, 1] and all(len(v) % c.hop for v in items)
    for b, v in enumerate(items):
        assert np.array_equal(rows[b, :len(v)], v) and (rows[b, len(v):] == dc.PLANT).all()
    assert len(dc.single(cid)) // c.hop + 1 == dc.FRAMES


@pytest.mark.parametrize('cid', IDS)
def test_stft_restatements_against_the_oracle(cid):
    """numpy's FFT of the restated frames is the oracle bit for bit; the kernel's packed
    Stockham transform in float64 is within the device bound of it, and its bit-identical
    share r (the floor the GPU test scales) is what a correct kernel can be asked for."""
    c = dc.BY_ID[cid]
    ys = [dc.single(cid)] + dc.batch(cid)[3] + ([dc.short_item(cid)] if cid in 'BC' else [])
    for y in ys:
        ref = D.stft(y, c.n_fft, c.hop, c.win)
        assert np.array_equal(dc.stft_np(y, c), ref)
        packed = dc.stft_packed_np(y, c)
        assert dc.stft_close(packed, ref)
        r = dc.identical_share(packed, ref)
        print(f'{cid}: {len(y)} samples, {ref.shape[1]} frames, r = {r:.4f}')
        # frame 0 of an item is even about its centre under a symmetric window (reflect padding),
        # so its imaginary parts are rounding noise that no two FFTs share: 6 of 7 frames at most
        assert r > 0.7 or ref.shape[1] < 4


@pytest.mark.parametrize('cid', IDS)
def test_istft_restatement_against_the_oracle(cid):
    c = dc.BY_ID[cid]
    X = dc.random_spectrum(c, dc.FRAMES, 3)
    ref = D.istft(X, c.hop, c.win)
    wss = dc.cropped_wss(c, dc.FRAMES)
    got, w2 = dc.ola_np(dc.istft_frames_np(X, c), dc.window(c) ** 2, c.hop)
    assert np.array_equal(w2, wss) and got.shape == ref.shape == (c.hop * (dc.FRAMES - 1),)
    assert np.array_equal(got, ref)
    assert dc.weighted_istft_close(got, ref, wss)
    if cid in 'ABCD':
        assert dc.istft_close(got, ref) and (wss > 1e-3).all()
    else:
        # a small sum-square: the plain bound's scale is set by the few samples divided by it
        print(f'{cid}: min positive wss {wss[wss > 0].min():.3e}, zeros {(wss == 0).sum()}, '
              f'max |ref| {np.abs(ref).max():.3e}, max |ref * wss| {np.abs(ref * wss).max():.3e}')
        assert wss[wss > 0].min() < 0.03 and np.abs(ref).max() > 2 * np.abs(ref * wss).max()


# --- NNLS parity cases -----------------------------------------------------------------------------

@pytest.mark.parametrize('case', dc.NNLS_CASES, ids=lambda k: k.name)
def test_nnls_case_sits_in_its_band(case):
    """scipy's iteration count decides the device's path: up to 32 updates fit the first pass
    (m = 32), more take the rerun with m = min(n_bins, 513).  The bands keep a margin to both."""
    c = dc.BY_ID[case.cid]
    M, S, nits = dc.nnls_reference(case.name)
    print(f'{case.name}: nit {nits} (table {list(case.nit)})')
    assert M.shape == (c.mels, case.frames) and S.shape == (dc.n_bins(c), case.frames) and (S >= 0).all()
    if case.kind == 'first':
        assert len(nits) == 1 and nits[0] <= dc.FIRST_PASS_MAX
    elif case.kind == 'rerun':
        assert len(nits) == 1 and dc.RERUN_MIN <= nits[0] <= dc.n_bins(c) // 2
        assert nits[0] < G.NNLS_M_MAX
    else:
        assert case.frames > dc.nnls_cols(c) and len(nits) == 2 and max(nits) <= dc.FIRST_PASS_MAX


def test_some_first_pass_case_searches():
    """D's speech mel converges at the start point; the random mel there iterates."""
    assert dc.nnls_reference('D-speech')[2] == [0]
    assert dc.nnls_reference('D-rand')[2][0] > 0 and dc.nnls_reference('A-mixed')[2][0] > 0


@pytest.mark.parametrize('name', ['A-speech', 'D-rand', 'C-blocks'])
def test_oracle_nnls_with_counts_is_the_oracle(name):
    case = next(k for k in dc.NNLS_CASES if k.name == name)
    c = dc.BY_ID[case.cid]
    M, S, _ = dc.nnls_reference(name)
    assert np.array_equal(D.mel_to_stft(M, c.sr, c.n_fft, c.fmin, c.fmax), S)


# --- FISTA restatements ---------------------------------------------------------------------------

@pytest.mark.parametrize('cid', dc.MEL_IDS)
@pytest.mark.parametrize('kind', ['speech', 'rand'])
def test_fista_restatements(cid, kind):
    """The float32 and float64 forms of nnls_kernel's iteration from one start: non-negative,
    apart by float32 rounding only, so the bound built on them is far below the magnitudes; on
    the random mel (not converged after 32 steps) a solver one step short, or with another
    step size, is outside it."""
    c = dc.BY_ID[cid]
    A, pinv, inv_L = dc.fista_consts(c)
    M = dc.fista_mel(cid, kind)
    x32 = dc.fista_np(A, pinv, inv_L, M, 32, np.float32)
    x64 = dc.fista_np(A, pinv, inv_L, M, 32, np.float64)
    assert x32.dtype == np.float32 and x64.dtype == np.float64 and (x32 >= 0).all() and (x64 >= 0).all()
    scale = np.abs(x64).max()
    bound = dc.fista_bound(x32, x64, scale)
    print(f'{cid}-{kind}: max |x32 - x64| {np.abs(x32 - x64).max():.3e}, scale {scale:.3e}, bound {bound:.3e}')
    assert bound <= 1e-4 * scale
    if kind == 'rand':
        for bad in (dc.fista_np(A, pinv, inv_L, M, 31, np.float64),
                    dc.fista_np(A, pinv, 0.9 * inv_L, M, 32, np.float64)):
            print(f'    defect: {np.abs(bad - x64).max():.3e}')
            assert np.abs(bad - x64).max() > bound


# --- planted defects --------------------------------------------------------------------------------

def _stft_defects():
    return [
        ('window-left-aligned-A', 'A', 'single', dict(win=dc.window(dc.BY_ID['A'], align='left'))),
        ('window-left-aligned-B', 'B', 'single', dict(win=dc.window(dc.BY_ID['B'], align='left'))),
        ('odd-split-other-way-B', 'B', 'single', dict(win=dc.window(dc.BY_ID['B'], split='ceil'))),
        ('edge-padding-A', 'A', 'single', dict(pad_mode='edge')),
        ('edge-padding-D', 'D', 'single', dict(pad_mode='edge')),
        ('single-reflection-C', 'C', 'short', dict(single_reflection=True)),
        ('hop-quarter-n-C', 'C', 'single', dict(hop=dc.BY_ID['C'].n_fft // 4)),
        ('hop-quarter-n-E', 'E', 'single', dict(hop=dc.BY_ID['E'].n_fft // 4)),
        ('pair-swapped-D', 'D', 'single', dict(swap_pairs=True)),
        ('pair-swapped-C', 'C', 'single', dict(swap_pairs=True)),
        ('lone-frame-dropped-A', 'A', 'single', dict(drop_lone=True)),
        ('lone-frame-dropped-G', 'G', 'single', dict(drop_lone=True)),
    ]


@pytest.mark.parametrize('name,cid,which,defect', _stft_defects(), ids=[d[0] for d in _stft_defects()])
def test_stft_comparison_rejects_planted_defect(name, cid, which, defect):
    c = dc.BY_ID[cid]
    y = dc.single(cid) if which == 'single' else dc.short_item(cid)
    ref = D.stft(y, c.n_fft, c.hop, c.win)
    assert dc.stft_close(dc.stft_np(y, c), ref)
    bad = dc.stft_np(y, c, **defect)
    err = np.abs(bad - ref).max() / np.abs(ref).max()
    print(f'{name}: max error {err:.3e} of the scale (bound {dc.STFT_RTOL:.0e})')
    assert not dc.stft_close(bad, ref)
    if 'window' in name or 'split' in name or 'padding' in name or 'reflection' in name:
        # the log-mel comparison (atol 2e-5) sees it too where the configuration has mels
        if cid in dc.MEL_IDS:
            A = dc.filters(c)
            mel = lambda X: np.log(np.clip(A @ np.abs(X), 1e-5, None))  # noqa: E731
            assert np.abs(mel(bad) - mel(ref)).max() > dc.MEL_ATOL


def test_weighted_comparison_rejects_division_by_a_denormal_sum_square():
    """`w2 > 0` in place of `w2 > tiny`: at G's geometry, with a window that is 1e-20 at one tap
    that no other frame's window reaches (its square, 1e-40, is a float32 denormal), the right
    kernel leaves the undivided sum there and the defect divides it."""
    c = dc.BY_ID['G']
    w = dc.window(c).copy()
    assert w[40] == 0 and w[200] == 0 and c.hop == 160
    w[40] = 1e-20
    X = dc.random_spectrum(c, dc.FRAMES, 5)
    fr = dc.istft_frames_np(X, c, win=w)
    ref, wss = dc.ola_np(fr, w ** 2, c.hop)
    bad, _ = dc.ola_np(fr, w ** 2, c.hop, gt_zero=True)
    denorm = (wss > 0) & (wss <= dc.TINY32)
    assert denorm.sum() == dc.FRAMES - 1 and (wss == 0).any()
    assert (ref[denorm] != 0).all() and (np.abs(ref[denorm]) < 1e-18).all()
    assert dc.weighted_istft_close(ref, ref, wss)
    assert not dc.weighted_istft_close(bad, ref, wss)
    assert np.array_equal(bad[~denorm], ref[~denorm])  # the defect shows only there


@pytest.mark.parametrize('cid', ['E', 'G'])
def test_weighted_comparison_rejects_wrong_samples(cid):
    """The weighted comparison is no weaker than the plain one where the sum-square is
    ordinary: a frame shifted by one sample, a missing window, a dropped frame."""
    c = dc.BY_ID[cid]
    X = dc.random_spectrum(c, dc.FRAMES, 3)
    ref = D.istft(X, c.hop, c.win)
    wss = dc.cropped_wss(c, dc.FRAMES)
    fr = dc.istft_frames_np(X, c)
    w2 = dc.window(c) ** 2
    assert dc.weighted_istft_close(dc.ola_np(fr, w2, c.hop)[0], ref, wss)
    shifted = fr.copy()
    shifted[3] = np.roll(shifted[3], 1)
    dropped = fr.copy()
    dropped[dc.FRAMES - 1] = 0
    left = dc.istft_frames_np(X, c, win=np.roll(dc.window(c), 3))
    for bad in (shifted, dropped, left):
        assert not dc.weighted_istft_close(dc.ola_np(bad, w2, c.hop)[0], ref, wss)
    nonzero_tail = ref.copy()
    z = np.flatnonzero(wss <= dc.TINY32)
    if z.size:
        nonzero_tail[z[0]] += np.float32(1e-30)
        assert not dc.weighted_istft_close(nonzero_tail, ref, wss)


def test_overlap_add_order_matters():
    """The float32 overlap-add rounds after every add: frames summed last to first give other
    bits (so the kernel's frame order is part of what the ISTFT comparison holds)."""
    c = dc.BY_ID['A']
    fr = dc.istft_frames_np(dc.random_spectrum(c, dc.FRAMES, 3), c)
    fwd, _ = dc.ola_np(fr, dc.window(c) ** 2, c.hop)
    rev, _ = dc.ola_np(fr, dc.window(c) ** 2, c.hop, reverse=True)
    assert not np.array_equal(fwd, rev)
    assert dc.istft_close(rev, fwd)  # rounding only: inside the bound, outside equality


# --- the history cap of the L-BFGS-B NNLS (host side: these return before any launch) ------------------

def _nnls_args(m):
    F = ctypes.c_void_p(256)  # never dereferenced: validation fails first
    return _lib.NnlsArgs(F, 1, 7, 80, 1025, 0, F, 1, 32, m, 63, 0, 0, F, F, F, F, F, F, F, F, F)


def test_history_cap():
    lib = _lib.load()
    assert G.NNLS_M_MAX == 513 and _lib.ABI_VERSION == 22
    assert lib.ftmi_nnls_lbfgsb_workspace_bytes(1, 1025, 63, 514, 32) == 0
    assert lib.ftmi_nnls_lbfgsb_workspace_bytes(1, 2049, 31, 2049, 32) == 0
    assert lib.ftmi_nnls_lbfgsb_workspace_bytes(1, 1025, 63, 513, 32) > 0
    assert lib.ftmi_nnls_lbfgsb_workspace_bytes(1, 1025, 63, 32, 32) > 0
    a = _nnls_args(514)
    assert lib.ftmi_nnls_lbfgsb_start(ctypes.byref(a), None) == 1001
    assert lib.ftmi_nnls_lbfgsb_cycles(ctypes.byref(a), 1, None) == 1001
    st = ctypes.c_void_p(256)
    assert lib.ftmi_nnls_lbfgsb_finish(ctypes.byref(a), None, st, None, None) == 1001


@pytest.mark.parametrize('cid', dc.GL_IDS)
def test_griffinlim_inputs_are_well_conditioned(cid):
    """A Griffin-Lim input on which the oracle itself moves by a tenth of the device bound
    under a one-ulp change of S says nothing about the kernel: none of the table's does."""
    s = dc.gl_oracle_sensitivity(cid)
    print(f'{cid}: the oracle moves {s:.3e} of the peak per ulp of S (bound {dc.GL_RTOL:.0e})')
    assert s <= 0.1 * dc.GL_RTOL
