"""The audio kernels (csrc/dsp.hip, csrc/nnls.hip, forwardtacotron_amd/dsp.py) off the
reference configuration, against the librosa-0.7.2 oracle (oracle/dsp_oracle.py): the six
configurations of tests/dsp_cases.py (n_fft 64 .. 4096, win < n_fft with an even and an odd pad
split, hops that do not divide n_fft or exceed n_fft / 2 or the window, 8 .. 160 mels), items of 7
frames (the frame-pair kernels end on a lone frame), a batch of 7 / 4 / 1 frames with per-item
lengths and a row stride wider than the longest item, and an item shorter than n_fft / 2.
tests/test_dsp_cases.py (CPU) checks the table and shows that each comparison used here rejects
the planted defects.

Bounds are the project's (tests/test_gpu_dsp.py): STFT and ISTFT 1e-6 of the scale, log-mel
2e-5, Griffin-Lim 1e-4 of the peak, the L-BFGS-B magnitudes 1e-6 relative with scipy's iteration
count; the FISTA solver is held to 8 x the distance of its own float32 and float64 restatements.

Every test prints its figures before it asserts; DESIGN.md section 4c ("The audio path off the
reference configuration") lists them as measured on an MI355X.
"""
import ctypes

import numpy as np
import pytest
import torch

import dsp_cases as dc
from oracle import dsp_oracle as D

pytestmark = pytest.mark.gpu

IDS = [c.id for c in dc.CONFIGS]


@pytest.fixture(scope='module')
def dsps():
    from forwardtacotron_amd.dsp import DSP
    return {c.id: DSP.from_config(dc.config_dict(c)) for c in dc.CONFIGS}


def _dev(a):
    return torch.from_numpy(np.array(a, order='C')).cuda()  # a copy: the shared cases are read-only


def _wide(rows, extra=13):
    """Device rows as a view of a wider buffer (row stride > L), PLANT in the margin."""
    wide = torch.full((rows.shape[0], rows.shape[1] + extra), dc.PLANT, device='cuda')
    wide[:, :rows.shape[1]] = _dev(rows)
    view = wide[:, :rows.shape[1]]
    assert view.stride(0) > view.shape[1] and view.stride(1) == 1
    return view


def _ostft(y, c):
    return D.stft(y, c.n_fft, c.hop, c.win)


# --- STFT ------------------------------------------------------------------------------------------

@pytest.mark.parametrize('cid', IDS)
def test_stft_complex(dsps, cid):
    """Complex STFT within 1e-6 of max |ref|; on the 7-frame item the share of bit-identical bins
    is at least 0.9 r, r the share the float64 restatement of the kernel's own transform (two
    frames per Stockham FFT, dsp_cases.stft_packed_np) reaches against the oracle on the same
    input (frame 0 is even about its centre under a symmetric window, so its imaginary parts
    are rounding noise that no two FFTs share: r is 6/7 there, 1 at B's odd split).  Measured:
    the device's share equals r at every configuration (A 0.8588, B 1.0, C 0.8575, D 0.8745,
    E 0.8594, G 0.8616), max error 6e-16 of the scale."""
    from forwardtacotron_amd import dsp as G
    c = dc.BY_ID[cid]
    plan = dsps[cid].plan()
    assert (plan.n_fft, plan.hop, plan.nb, plan.n_mels) == (c.n_fft, c.hop, dc.n_bins(c), c.mels)
    y = dc.single(cid)
    ref = _ostft(y, c)
    X = G.stft(plan, _dev(y)[None])[0].cpu().numpy().T
    assert X.shape == ref.shape == (dc.n_bins(c), dc.FRAMES)
    err = np.abs(X - ref).max() / np.abs(ref).max()
    r = dc.identical_share(dc.stft_packed_np(y, c), ref)
    share = dc.identical_share(X, ref)
    print(f'{cid}: max error {err:.3e} of the scale, identical share {share:.4f}, restatement r {r:.4f}')
    assert dc.stft_close(X, ref)
    assert share >= 0.9 * r


@pytest.mark.parametrize('cid', IDS)
def test_stft_batch_lengths_and_stride(dsps, cid):
    from forwardtacotron_amd import dsp as G
    c = dc.BY_ID[cid]
    rows, lengths, frames, items = dc.batch(cid)
    Xb = G.stft(dsps[cid].plan(), _wide(rows), lengths=_dev(lengths)).cpu().numpy()
    assert Xb.shape == (3, dc.FRAMES, dc.n_bins(c))
    for b, v in enumerate(items):
        ref = _ostft(v, c)
        got = Xb[b, :frames[b]].T
        print(f'{cid}[{b}]: max error {np.abs(got - ref).max() / np.abs(ref).max():.3e} of the scale')
        assert dc.stft_close(got, ref)


@pytest.mark.parametrize('cid', ['B', 'C'])
def test_stft_item_shorter_than_the_padding(dsps, cid):
    """700 samples under a pad of 1024 (B) and 2048 (C: reflected three times)."""
    from forwardtacotron_amd import dsp as G
    c = dc.BY_ID[cid]
    y = dc.short_item(cid)
    ref = _ostft(y, c)
    X = G.stft(dsps[cid].plan(), _dev(y)[None])[0].cpu().numpy().T
    print(f'{cid}: max error {np.abs(X - ref).max() / np.abs(ref).max():.3e} of the scale')
    assert dc.stft_close(X, ref)
    mel = dsps[cid].wav_to_mel(y)
    np.testing.assert_allclose(mel, D.wav_to_mel(y, **dc.kw(c)), rtol=0, atol=dc.MEL_ATOL)


# --- log-mel ------------------------------------------------------------------------------------------

@pytest.mark.parametrize('cid', dc.MEL_IDS)
def test_wav_to_mel(dsps, cid):
    c = dc.BY_ID[cid]
    y = dc.single(cid)
    ref = D.wav_to_mel(y, **dc.kw(c))
    got = dsps[cid].wav_to_mel(y)
    assert got.shape == ref.shape == (c.mels, dc.FRAMES) and got.dtype == np.float32
    print(f'{cid}: max |log-mel error| {np.abs(got - ref).max():.3e}')
    np.testing.assert_allclose(got, ref, rtol=0, atol=dc.MEL_ATOL)


@pytest.mark.parametrize('cid', dc.MEL_IDS)
def test_mel_batch_with_frames(dsps, cid):
    """Items of 7 / 4 / 1 frames with lengths, frames and a wide row stride: each against the
    oracle, zeros past its frames, and bit-equal to the single-item call (mel_spectrogram's
    docstring: an item's last frame is the lone frame of its own transform when its frame
    count is given)."""
    from forwardtacotron_amd import dsp as G
    c = dc.BY_ID[cid]
    plan = dsps[cid].plan()
    rows, lengths, frames, items = dc.batch(cid)
    mel = G.mel_spectrogram(plan, _wide(rows), lengths=_dev(lengths), frames=_dev(frames)).cpu().numpy()
    assert mel.shape == (3, c.mels, dc.FRAMES)
    for b, v in enumerate(items):
        fb = int(frames[b])
        ref = D.wav_to_mel(v, **dc.kw(c))
        assert ref.shape == (c.mels, fb)
        np.testing.assert_allclose(mel[b, :, :fb], ref, rtol=0, atol=dc.MEL_ATOL)
        assert (mel[b, :, fb:] == 0).all()
        alone = G.mel_spectrogram(plan, _dev(v)[None])[0].cpu().numpy()
        assert np.array_equal(mel[b, :, :fb].view(np.int32), alone.view(np.int32))


# --- ISTFT ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('cid', IDS)
def test_istft(dsps, cid):
    """Random spectra, items of 7 / 4 / 1 frames (garbage planted in the frames past each item):
    A-D at 1e-6 of max |ref|; E and G, whose window sum-square dips towards zero (G: exact zeros
    where no window reaches, the undivided sum kept there), by the weighted comparison.  Zeros
    after hop * (frames - 1); item 0 alone gives the same bits."""
    from forwardtacotron_amd import dsp as G
    c = dc.BY_ID[cid]
    plan = dsps[cid].plan()
    nb, F = dc.n_bins(c), dc.FRAMES
    Xb = np.full((3, F, nb), dc.PLANT * (1 + 1j), dtype=np.complex64)
    specs = [dc.random_spectrum(c, f, 3 + b) for b, f in enumerate(dc.BATCH_FRAMES)]
    for b, X in enumerate(specs):
        Xb[b, :X.shape[1]] = X.T
    got = G.istft(plan, _dev(Xb), frames=_dev(np.array(dc.BATCH_FRAMES, np.int32))).cpu().numpy()
    assert got.shape == (3, c.hop * (F - 1))
    for b, X in enumerate(specs):
        fb = X.shape[1]
        n = c.hop * (fb - 1)
        assert not got[b, n:].any()
        if fb == 1:
            continue
        ref = D.istft(X, c.hop, c.win)
        assert ref.shape == (n,)
        if cid in 'ABCD':
            print(f'{cid}[{b}]: max error {np.abs(got[b, :n] - ref).max() / np.abs(ref).max():.3e} of max |ref|')
            assert dc.istft_close(got[b, :n], ref)
        else:
            wss = dc.cropped_wss(c, fb)
            e = np.abs((got[b, :n].astype(np.float64) - ref) * wss).max() / np.abs(ref * wss).max()
            print(f'{cid}[{b}]: max weighted error {e:.3e} of max |ref * wss|, '
                  f'{(wss <= dc.TINY32).sum()} samples without a window')
            assert dc.weighted_istft_close(got[b, :n], ref, wss)
    alone = G.istft(plan, _dev(Xb[:1]))[0].cpu().numpy()
    assert np.array_equal(alone.view(np.int32), got[0].view(np.int32))


# --- Griffin-Lim (the generic three-kernel loop: no configuration here is 1024 / 256) ----------------------

@pytest.mark.parametrize('cid', dc.GL_IDS)
def test_griffinlim_from_stft(dsps, cid):
    """8 iterations from the oracle's S and phases, 1e-4 of the peak (test_dsp_cases.py: the
    oracle itself moves less than 1e-6 of the peak per ulp of S on these inputs).  Measured:
    A 5.2e-7, B 6.1e-7, C 4.9e-7, D 4.0e-7 of the peak."""
    from forwardtacotron_amd import dsp as G
    c = dc.BY_ID[cid]
    plan = dsps[cid].plan()
    assert not G._gl_fused(plan)
    S, ang, ref = dc.gl_case(cid)
    got = G.griffinlim_from_stft(plan, _dev(S.T)[None], _dev(ang.T)[None], dc.GL_ITERS)[0].cpu().numpy()
    assert got.shape == ref.shape == (c.hop * (dc.FRAMES - 1),)
    peak = np.abs(ref).max()
    print(f'{cid}: max deviation {np.abs(got - ref).max() / peak:.3e} of the peak')
    np.testing.assert_allclose(got, ref, rtol=0, atol=dc.GL_RTOL * peak)


def test_griffinlim_end_to_end_at_A(dsps):
    """DSP.griffinlim(mel, random_state=s) — exp, the L-BFGS-B NNLS, 32 iterations — against the
    oracle's whole chain under the same seed, at the bounds of test_gpu_dsp.py's end-to-end
    test: 1e-3 x peak per sample, <= 1 % of samples past 1e-4 x peak, relative L2 < 1e-3.
    Measured: 1.2e-5 x peak at most, relative L2 7.2e-6."""
    c = dc.BY_ID['A']
    mel = dc.speech_mel('A')
    T, nb = mel.shape[1], dc.n_bins(c)
    ang = np.exp(2j * np.pi * np.random.RandomState(dc.E2E_SEED).rand(nb, T)).astype(np.complex64)
    S = D.mel_to_stft(np.exp(mel), c.sr, c.n_fft, c.fmin, c.fmax)
    ref = D.griffinlim_from_stft(S, ang, n_iter=32, hop_length=c.hop, win_length=c.win)
    got = dsps['A'].griffinlim(mel, random_state=dc.E2E_SEED)
    assert got.shape == ref.shape == (c.hop * (T - 1),) and got.dtype == np.float32
    peak = np.abs(ref).max()
    d = np.abs(got - ref) / peak
    print(f'A: max deviation {d.max():.3e} of the peak, {(d > 1e-4).mean():.4f} of samples past 1e-4, '
          f'relative L2 {np.linalg.norm(got - ref) / np.linalg.norm(ref):.3e}')
    assert d.max() <= 1e-3
    assert (d > 1e-4).mean() <= 0.01
    assert np.linalg.norm(got - ref) / np.linalg.norm(ref) < 1e-3


# --- FISTA NNLS (nnls_kernel<3 | 5 | 17 | 33, 2> and <33, 8>) ------------------------------------------------

@pytest.mark.parametrize('cid', dc.MEL_IDS)
@pytest.mark.parametrize('kind', ['speech', 'rand'])
def test_mel_to_stft_fista(dsps, cid, kind):
    """The kernel against the float64 restatement of its own iteration (same start, inv_L, t /
    beta recurrence and step count): within 8 x the distance between the float32 and float64
    restatements plus 1e-7 of max |S| (the kernel is the float32 form summed in another
    order).  Non-negative; the frames past each item's count exactly zero.  Measured ratio
    max |S - fista64| / max |fista32 - fista64|: speech A 0.67, B 2.50, C 1.00, D 2.11, E 0.61;
    random mel A 0.93, B 1.14, C 1.00, D 1.26, E 0.87."""
    from forwardtacotron_amd import dsp as G
    c = dc.BY_ID[cid]
    plan = dsps[cid].plan()
    M = dc.fista_mel(cid, kind)
    A, pinv, inv_L = dc.filters(c), plan.pinv.cpu().numpy(), plan.inv_L
    assert np.array_equal(A, plan.basis_np)
    x32 = dc.fista_np(A, pinv, inv_L, M, 32, np.float32)
    x64 = dc.fista_np(A, pinv, inv_L, M, 32, np.float64)
    bound = dc.fista_bound(x32, x64, np.abs(x64).max())
    Mb = np.full((3, c.mels, dc.FRAMES), dc.PLANT, dtype=np.float32)
    cols = [np.arange(7), np.array([6, 4, 2, 0]), np.array([3])]
    for b, k in enumerate(cols):
        Mb[b, :, :len(k)] = M[:, k]
    S = G.mel_to_stft(plan, _dev(Mb), _dev(np.array(dc.BATCH_FRAMES, np.int32)), denorm=False,
                      iters=32, method='fista').cpu().numpy()
    assert S.shape == (3, dc.FRAMES, dc.n_bins(c)) and S.dtype == np.float32 and (S >= 0).all()
    worst = 0.0
    for b, k in enumerate(cols):
        assert not S[b, len(k):].any()
        worst = max(worst, float(np.abs(S[b, :len(k)].T.astype(np.float64) - x64[:, k]).max()))
    d32 = float(np.abs(x32 - x64).max())
    print(f'{cid}-{kind}: max |S - fista64| {worst:.3e}, max |fista32 - fista64| {d32:.3e}, '
          f'ratio {worst / max(d32, 1e-300):.2f}, bound {bound:.3e}, max |S| {np.abs(x64).max():.3e}')
    assert worst <= bound


# --- L-BFGS-B NNLS (block widths 255 / 63 / 31, the rerun with the capped history) ------------------------------

@pytest.mark.parametrize('case', dc.NNLS_CASES, ids=lambda k: k.name)
def test_mel_to_stft_lbfgsb_is_the_reference(dsps, case):
    """mel_to_stft(method='lbfgsb') returns the oracle's S to 1e-6 with scipy's iteration count
    per block: first-pass cases (history m = 32), rerun cases (m = min(n_bins, 513): 257 at A,
    129 at E, the cap 513 at B and C) and 33 frames at C (blocks of 31 and 2 frames, the second
    from the oracle's warm start).  Measured relative error: 0 .. 2.1e-16 on the first pass,
    rerun A 3.1e-10, B 7.1e-18, C 1.4e-13, E 1.8e-7; the iteration counts equal scipy's."""
    from forwardtacotron_amd import dsp as G
    c = dc.BY_ID[case.cid]
    plan = dsps[case.cid].plan()
    assert plan.nnls_cols == dc.nnls_cols(c)
    M, ref, nits = dc.nnls_reference(case.name)
    md = _dev(M)[None]
    S = G.mel_to_stft(plan, md, denorm=False, method='lbfgsb')[0].cpu().numpy().T
    info, debug = [], {}
    S2 = G._nnls_lbfgsb(plan, md, None, False, info=info, debug=debug)[0].cpu().numpy().T
    assert np.array_equal(S, S2)
    assert S.shape == ref.shape and S.dtype == np.float32 and (S >= 0).all()
    rel = np.linalg.norm(S.astype(np.float64) - ref) / np.linalg.norm(ref)
    its = [int(r[0]) for r in info]
    print(f'{case.name}: relative error {rel:.3e}, iterations {its} (scipy {nits}), history m = {debug["m"]}')
    assert rel <= dc.NNLS_RTOL
    assert np.abs(S - ref).max() <= dc.NNLS_RTOL * 10 * np.abs(ref).max()
    assert its == nits
    assert debug['m'] == (min(plan.nb, G.NNLS_M_MAX) if case.kind == 'rerun' else 32)


# --- the history cap (host side only: these calls return before any launch) --------------------------------------

def test_history_cap():
    """csrc/nnls.hip holds its history vectors in LDS arrays of 2 * 513 entries: a history of
    more columns is refused by the argument check of every entry point."""
    from forwardtacotron_amd import _lib
    from forwardtacotron_amd import dsp as G
    lib = _lib.load()
    assert G.NNLS_M_MAX == 513
    assert lib.ftmi_nnls_lbfgsb_workspace_bytes(1, 1025, 63, 514, 32) == 0
    assert lib.ftmi_nnls_lbfgsb_workspace_bytes(1, 1025, 63, 513, 32) > 0
    F = ctypes.c_void_p(256)  # never dereferenced: validation fails first
    a = _lib.NnlsArgs(F, 1, 7, 80, 1025, 0, F, 1, 32, 514, 63, 0, 0, F, F, F, F, F, F, F, F, F)
    assert lib.ftmi_nnls_lbfgsb_start(ctypes.byref(a), None) == 1001
