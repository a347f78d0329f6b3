"""The validation-loss entry points through ctypes, without a GPU: every argument error returns
an FTMI_E_* code on the host, before any launch (the pointers here are never dereferenced), each
workspace query answers 0 for a shape its kernel does not take, and the Python layers refuse
CPU tensors and wrong dtypes before they touch the library."""
import ctypes

import pytest
import torch

from forwardtacotron_amd import _lib

ARG, SHAPE, UNSUPPORTED, ALIGN = 1001, 1002, 1003, 1004
f, g, w8 = ctypes.c_void_p(256), ctypes.c_void_p(258), ctypes.c_void_p(264)


def l1(lib, x=f, xs=(3200, 40, 1), target=f, ts=(3200, 1, 80), B=2, C=80, L=40, lens=f, out=f, ws=f):
    return lib.ftmi_l1_loss(x, *xs, target, *ts, B, C, L, lens, out, ws, None)


def ce(lib, logits=f, ld=512, rows=100, C=512, target=f, out=f, bad=f, ws=f):
    return lib.ftmi_cross_entropy(logits, ld, rows, C, target, out, bad, ws, None)


def mol(lib, y_hat=f, ld=30, rows=100, channels=30, y=f, num_classes=65536.0, log_scale_min=-32.0,
        out=f, per_sample=f, ws=f):
    return lib.ftmi_mol_loss(y_hat, ld, rows, channels, y, num_classes, log_scale_min, out,
                             per_sample, ws, None)


def test_l1_argument_errors():
    lib = _lib.load()
    for k in ('x', 'target', 'out', 'ws'):
        assert l1(lib, **{k: None}) == ARG, k
    for k in ('B', 'C', 'L'):
        assert l1(lib, **{k: 0}) == ARG and l1(lib, **{k: -3}) == ARG, k
    # frame-major needs a channel stride >= L, channel-major a frame stride >= C; nothing else
    for bad in ((3200, 39, 1), (3200, 1, 79), (3200, 2, 2), (3200, 40, 0), (-1, 40, 1), (3200, 0, 1)):
        assert l1(lib, xs=bad) == SHAPE, bad
        assert l1(lib, ts=bad) == SHAPE, bad
    # more workgroups than one launch takes
    assert l1(lib, B=1 << 20, L=1 << 10, xs=(0, 1 << 10, 1), ts=(0, 1, 80)) == UNSUPPORTED
    for k in ('x', 'target', 'lens', 'out'):
        assert l1(lib, **{k: g}) == ALIGN, k
    assert l1(lib, ws=w8) == ALIGN
    assert l1(lib, lens=None, x=None) == ARG  # lens is optional, x is not


def test_cross_entropy_argument_errors():
    lib = _lib.load()
    for k in ('logits', 'target', 'out', 'bad', 'ws'):
        assert ce(lib, **{k: None}) == ARG, k
    for k in ('rows', 'C'):
        assert ce(lib, **{k: 0}) == ARG and ce(lib, **{k: -1}) == ARG, k
    assert ce(lib, ld=511) == SHAPE
    assert ce(lib, C=65537, ld=65537) == UNSUPPORTED
    for k in ('logits', 'target', 'out', 'bad'):
        assert ce(lib, **{k: g}) == ALIGN, k
    assert ce(lib, ws=w8) == ALIGN


def test_mol_argument_errors():
    lib = _lib.load()
    for k in ('y_hat', 'y', 'out', 'ws'):
        assert mol(lib, **{k: None}) == ARG, k
    for k in ('rows', 'channels'):
        assert mol(lib, **{k: 0}) == ARG and mol(lib, **{k: -3}) == ARG, k
    assert mol(lib, num_classes=1.0) == ARG and mol(lib, log_scale_min=float('nan')) == ARG
    assert mol(lib, channels=31, ld=31) == UNSUPPORTED   # not 3 K
    assert mol(lib, channels=99, ld=99) == UNSUPPORTED   # K = 33
    assert mol(lib, channels=96, ld=95) == SHAPE          # K = 32 is taken; the stride is short
    assert mol(lib, ld=29) == SHAPE
    for k in ('y_hat', 'y', 'out', 'per_sample'):
        assert mol(lib, **{k: g}) == ALIGN, k
    assert mol(lib, ws=w8) == ALIGN


def test_workspace_queries():
    lib = _lib.load()
    assert lib.ftmi_l1_loss_workspace_bytes(64, 80, 1400) == 64 * 44 * 8
    assert lib.ftmi_l1_loss_workspace_bytes(1, 1, 1) == 8
    for bad in ((0, 80, 10), (2, 0, 10), (2, 80, 0), (-1, 80, 10), (1 << 20, 80, 1 << 10)):
        assert lib.ftmi_l1_loss_workspace_bytes(*bad) == 0, bad
    assert lib.ftmi_cross_entropy_workspace_bytes(17, 512) == 2 * 12
    for bad in ((0, 512), (-5, 512), (10, 0), (10, 65537)):
        assert lib.ftmi_cross_entropy_workspace_bytes(*bad) == 0, bad
    assert lib.ftmi_cross_entropy_workspace_bytes(10, 65536) > 0
    assert lib.ftmi_mol_loss_workspace_bytes(129, 10) == 2 * 8
    for bad in ((0, 10), (-1, 10), (10, 0), (10, 33)):
        assert lib.ftmi_mol_loss_workspace_bytes(*bad) == 0, bad
    assert lib.ftmi_mol_loss_workspace_bytes(10, 32) > 0


def test_abi_number_unchanged():
    assert _lib.ABI_VERSION == 22 and _lib.load().ftmi_abi_version() == 22


def test_ops_refuse_cpu_tensors_and_wrong_dtypes():
    from forwardtacotron_amd import ops
    x = torch.zeros(2, 3, 4)
    with pytest.raises(RuntimeError, match='HIP device only'):
        ops.l1_loss(x, x)
    with pytest.raises(RuntimeError, match='HIP device only'):
        ops.cross_entropy(torch.zeros(4, 5), torch.zeros(4, dtype=torch.int32))
    with pytest.raises(RuntimeError, match='HIP device only'):
        ops.mol_loss(torch.zeros(4, 30), torch.zeros(4), 65536, -32.0)


def test_public_functions_refuse_cpu_tensors_and_wrong_dtypes():
    from forwardtacotron_amd import evaluate as ev
    x, lens = torch.zeros(2, 3, 4), torch.tensor([4, 2])
    with pytest.raises(RuntimeError, match='HIP device only'):
        ev.masked_l1(x, x, lens)
    with pytest.raises(RuntimeError, match='HIP device only'):
        ev.l1(x, x)
    with pytest.raises(RuntimeError, match='HIP device only'):
        ev.cross_entropy(torch.zeros(4, 5), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(RuntimeError, match='HIP device only'):
        ev.discretized_mix_logistic_loss(torch.zeros(1, 4, 30), torch.zeros(1, 4, 1))
    with pytest.raises(RuntimeError, match='HIP device only'):
        ev.mel_l1(None, torch.zeros(100), torch.zeros(100))
    with pytest.raises(ValueError, match='must be a tensor'):
        ev.l1([1.0], [2.0])
    # a wrong dtype is a TypeError wherever the tensor lives
    with pytest.raises(TypeError, match='x must be fp32'):
        ev.masked_l1(x.double(), x, lens)
    with pytest.raises(TypeError, match='target must be fp32 or int'):
        ev.l1(x, x.half())
    with pytest.raises(TypeError, match='lens must be int'):
        ev._lens(lens.float(), 2, 'cpu')
    with pytest.raises(TypeError, match='logits must be fp32'):
        ev.cross_entropy(torch.zeros(4, 5, dtype=torch.float64), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(TypeError, match='target must be int'):
        ev.cross_entropy(torch.zeros(4, 5), torch.zeros(4))
    with pytest.raises(TypeError, match='y must be fp32'):
        ev.discretized_mix_logistic_loss(torch.zeros(1, 4, 30), torch.zeros(1, 4, 1, dtype=torch.int64))
