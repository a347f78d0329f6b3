"""ftmi_run_chain's validation (no GPU needed: every case returns before any launch).

The lists here point at fabricated addresses, never at device memory: each case must be
refused by the validation pass, which runs over the whole list before the first launch.  A
list that passed would reach the entry points, so no case here is a valid list."""
import ctypes

import pytest

from forwardtacotron_amd import _lib
from forwardtacotron_amd._lib import ChainBase, ChainOp

E_ARG, E_ALIGN = 1001, 1004


def _rowdot(M=8, C=128):
    """A one-op list: rowdot over M rows of C floats; slots: 0 x, 1 w, 2 out."""
    ops = (ChainOp * 1)()
    op = ops[0]
    op.tag = _lib.CHAIN_ROWDOT
    for r in op.p:
        r.slot = -1
    for k, (slot, nbytes) in enumerate(((0, M * C * 4), (1, C * 4), (-1, 0), (2, M * 4))):
        op.p[k].slot, op.p[k].bytes, op.p[k].flags = slot, nbytes, _lib.CHAIN_ALIGN16
    op.i[0], op.i[1], op.i[2] = C, M, C
    op.f[0] = 1.0
    bases = (ChainBase * 3)()
    for b, n in zip(bases, (M * C * 4, C * 4, M * 4)):
        b.base, b.bytes = 4096, n
    return ops, bases


def _run(ops, bases, n=1, n_bases=3):
    failed = ctypes.c_int32(-7)
    rc = _lib.load().ftmi_run_chain(ops, n, bases, n_bases, ctypes.byref(failed), None)
    return rc, failed.value


def test_empty_and_null_lists():
    ops, bases = _rowdot()
    assert _run(ops, bases, n=0) == (E_ARG, -1)
    assert _run(None, bases) == (E_ARG, -1)
    assert _run(ops, None) == (E_ARG, -1)
    assert _run(ops, bases, n_bases=0) == (E_ARG, -1)
    assert _lib.load().ftmi_run_chain(ops, 0, bases, 3, None, None) == E_ARG  # failed_op optional


def _set(path, value):
    def f(ops, bases):
        obj = {'ops': ops, 'bases': bases}[path[0]]
        for p in path[1:-1]:
            obj = obj[p] if isinstance(p, int) else getattr(obj, p)
        if isinstance(path[-1], int):
            obj[path[-1]] = value
        else:
            setattr(obj, path[-1], value)
    return f


@pytest.mark.parametrize('change,code', [
    (_set(('ops', 0, 'tag'), 99), E_ARG),                        # unknown tag
    (_set(('ops', 0, 'tag'), 0), E_ARG),
    (_set(('ops', 0, 'p', 0, 'slot'), 3), E_ARG),                # slot outside the table
    (_set(('bases', 1, 'base'), None), E_ARG),                   # a slot without a base
    (_set(('ops', 0, 'p', 0, 'offset'), 16), E_ARG),             # the range ends past its slot
    (_set(('ops', 0, 'p', 0, 'offset'), -16), E_ARG),
    (_set(('ops', 0, 'p', 1, 'offset'), 1 << 40), E_ARG),        # an offset past its slot
    (_set(('ops', 0, 'p', 1, 'bytes'), -1), E_ARG),
    (_set(('bases', 0, 'bytes'), 8 * 128 * 4 - 1), E_ARG),       # a slot one byte short
    (_set(('bases', 0, 'base'), 4100), E_ALIGN),                 # a misaligned base
    (_set(('ops', 0, 'p', 3, 'bytes'), 8 * 4 - 1), E_ARG),       # output smaller than M floats
    (_set(('ops', 0, 'i', 1), -1), E_ARG),                       # a negative row count
])
def test_validation(change, code):
    ops, bases = _rowdot()
    change(ops, bases)
    assert _run(ops, bases) == (code, 0)


def test_conv_and_recurrence_write_extents():
    """The ranges a conv (y, split-K partials) and a recurrence (y, workspace) write must be
    as large as their shapes need."""
    lib = _lib.load()
    B, T, N, H = 2, 8, 32, 64
    for tag, big, small in (
            (_lib.CHAIN_CONV1D, {6: B * T * N * 4, 8: 2 * B * T * N * 4}, (6, 8)),
            (_lib.CHAIN_RNN_BIDIR, {6: B * T * 2 * H * 4, 8: lib.ftmi_rnn_workspace_bytes(B, H, 0)}, (6, 8))):
        for short in small:
            ops = (ChainOp * 1)()
            op = ops[0]
            op.tag = tag
            for r in op.p:
                r.slot = -1
            for k, n in big.items():
                op.p[k].slot, op.p[k].bytes = 0, n - (1 if k == short else 0)
            if tag == _lib.CHAIN_CONV1D:
                for j, v in enumerate((16, B, T, 16, N, 1, 0, 0, 0, 0, N, 0, 2, 2, 0)):
                    op.i[j] = v
            else:
                for j, v in enumerate((0, B, T, H, 6 * H, T, 2 * H, 2)):
                    op.i[j] = v
            bases = (ChainBase * 1)()
            bases[0].base, bases[0].bytes = 4096, 1 << 30
            assert _run(ops, bases, n_bases=1) == (E_ARG, 0), (tag, short)


def test_second_op_is_named():
    ops2 = (ChainOp * 2)()
    ops, bases = _rowdot()
    ctypes.memmove(ops2, ops, ctypes.sizeof(ChainOp))
    ctypes.memmove(ctypes.byref(ops2, ctypes.sizeof(ChainOp)), ops, ctypes.sizeof(ChainOp))
    ops2[1].p[3].offset = 4
    assert _run(ops2, bases, n=2) == (E_ARG, 1)


def test_struct_sizes_match_header():
    """The ctypes mirrors have the C layout (LP64): ref 24 bytes, op 8 + 12 refs + 16 int64 +
    2 floats, base 16."""
    assert ctypes.sizeof(_lib.ChainRef) == 24
    assert ctypes.sizeof(ChainOp) == 8 + 12 * 24 + 16 * 8 + 8
    assert ctypes.sizeof(ChainBase) == 16
