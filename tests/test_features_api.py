"""The phoneme pitch / energy entry points through ctypes, without a GPU: every argument error
returns an FTMI_E_* code on the host, before any launch (the pointers here are never
dereferenced).  ftmi_phoneme_features keeps its frames in LDS and takes no workspace, so there
is no workspace query whose 0 would mark an unsupported shape: T > 512 answers
FTMI_E_UNSUPPORTED from the entry point itself."""
import ctypes

from forwardtacotron_amd import _lib

ARG, SHAPE, UNSUPPORTED, ALIGN = 1001, 1002, 1003, 1004
f, g = ctypes.c_void_p(256), ctypes.c_void_p(258)


def features(lib, mel=f, ld_bin=40, ld_item=3200, B=1, n_mels=80, rows=40, mel_len=f, dur=f, ld_dur=12,
             T=12, x_len=None, pitch=f, ld_pitch=40, P=40, pitch_len=f, fmax=400.0, pitch_out=f,
             energy_out=f, dur_sum=f):
    return lib.ftmi_phoneme_features(mel, ld_bin, ld_item, B, n_mels, rows, mel_len, dur, ld_dur, T,
                                     x_len, pitch, ld_pitch, P, pitch_len, fmax, pitch_out, energy_out,
                                     dur_sum, None)


def test_phoneme_features_argument_errors():
    lib = _lib.load()
    for k in ('mel', 'mel_len', 'dur', 'energy_out', 'dur_sum'):
        assert features(lib, **{k: None}) == ARG, k
    for k in ('B', 'n_mels', 'rows', 'T'):
        assert features(lib, **{k: 0}) == ARG, k
        assert features(lib, **{k: -1}) == ARG, k
    # pitch, its lengths and its output: all or none
    assert features(lib, pitch=None) == ARG and features(lib, pitch_len=None) == ARG
    assert features(lib, pitch_out=None) == ARG and features(lib, pitch=None, pitch_len=None) == ARG
    assert features(lib, P=0) == ARG
    assert features(lib, T=513, ld_dur=513) == UNSUPPORTED
    assert features(lib, ld_bin=39) == SHAPE and features(lib, ld_dur=11) == SHAPE
    assert features(lib, ld_pitch=39) == SHAPE and features(lib, ld_item=-1) == SHAPE
    for k in ('mel', 'mel_len', 'dur', 'x_len', 'pitch', 'pitch_len', 'pitch_out', 'energy_out', 'dur_sum'):
        assert features(lib, **{k: g}) == ALIGN, k


def test_moments_and_normalise_argument_errors():
    lib = _lib.load()
    assert lib.ftmi_nonzero_moments(None, 4, f, None) == ARG
    assert lib.ftmi_nonzero_moments(f, 4, None, None) == ARG
    assert lib.ftmi_nonzero_moments(f, 0, f, None) == ARG
    assert lib.ftmi_nonzero_moments(g, 4, f, None) == ALIGN
    assert lib.ftmi_nonzero_moments(f, 4, ctypes.c_void_p(260), None) == ALIGN  # doubles
    assert lib.ftmi_normalize_nonzero(None, 4, 1.0, 1.0, None) == ARG
    assert lib.ftmi_normalize_nonzero(f, 0, 1.0, 1.0, None) == ARG
    assert lib.ftmi_normalize_nonzero(g, 4, 1.0, 1.0, None) == ALIGN
