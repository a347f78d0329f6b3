"""The recurrence's kernel and grid decision, asked through ftmi_rnn_route (no GPU needed: a
host-only function that launches nothing and reads no pointer).

`_parent_launch` is the Python restatement, copied rule by rule, of the launch path the library
had before ABI 22 (the ladder of `ftmi_rnn_bidir`, `launch_rnn`, `launch_gemv`), and
`_parent_blocks` of the hand-kept second copy that `ftmi_rnn_blocks` was: the record of what
the library used to do and used to report, against which its one decision is swept.  Both read
the environment where the parent read it (the parent kept FTMI_RNN_PAD, FTMI_RNN_U64 and the
general FTMI_RNN_PSLEEP from its first call; here every call reads them)."""
import ctypes
import functools
import os
import re
from pathlib import Path

import pytest

from forwardtacotron_amd import _lib
from forwardtacotron_amd._lib import RnnRoute

HEADER = Path(__file__).resolve().parent.parent / 'include' / 'ftmi.h'
OK, E_ARG, E_UNSUPPORTED = 0, 1001, 1003
SPREAD = 0x100
NB, GV_MAXB, GV_KSEG, GV_RPT = 16, 4, 8, 2


# ---- the parent's launch path (csrc/rnn.hip before ABI 22), verbatim ------------------------
def _env(name, default):
    v = os.environ.get(name)
    return int(v) if v is not None else default


def _gemv_path(cell, B, H):
    return bool(_env('FTMI_RNN_GEMV', 1)) and B <= GV_MAXB and (
        (cell == 1 and H == 512) or (cell == 0 and H in (64, 128, 256)))


def _xcd_local_env():
    return _env('FTMI_RNN_XCD_LOCAL', 1)


def _rnn_units(cell, H, mma):
    if cell == 0 and H == 64:
        return 32 if (mma == 2 and _env('FTMI_RNN_U64', 32) == 32) else 64
    return 16


def _cst_enabled():
    return _env('FTMI_RNN_CSTORE', 1) != 0


def _cellrows_enabled():
    return _env('FTMI_RNN_CELLROWS', 1) != 0


def _legacy_nbl(cell, B, H, mma, spread, maxb):
    if (not spread or mma != 2 or cell != 0 or H != 256 or not _cst_enabled()
            or _env('FTMI_RNN_NB', 8) == 16):
        return NB
    return 8 if 2 * ((B + 7) // 8) * (H // 16) <= maxb else NB


def _u8_path(cell, B, H, mma, spread, maxb):
    if not spread or mma != 2 or not _cst_enabled() or cell != 0 or H != 256:
        return False
    if _env('FTMI_RNN_U8', 1) == 0:
        return False
    ngroups = 2 * ((B + NB - 1) // NB)
    return max(ngroups, 8) * (H // 8) <= maxb


def _u8_psleep():
    v = os.environ.get('FTMI_RNN_PSLEEP')
    return int(v) if v is not None else (3 if _cellrows_enabled() else 6)


def _launch_gemv(cell, H, U, kseg, B, xcd_local, maxb, psleep):
    BPG = H // U
    NT = (4 if cell else 3) * U // GV_RPT * kseg
    if 8 * BPG > maxb:
        return None, 0, 0, 0, psleep, E_UNSUPPORTED
    nblk = 8 * BPG if xcd_local else 2 * BPG
    nbv = {1: 1, 2: 2}.get(B, 4)
    return ('gemv', cell, H, U, nbv, kseg), NT, 1, nblk, psleep, OK


def _launch_rnn(cell, H, U, WK, MODE, CST, NBL, CR, B, nchunks, xcd_local, maxb, psleep):
    if NBL != NB:
        nchunks = (B + NBL - 1) // NBL
    BPG = H // U
    max_groups = (maxb // BPG) & ~1
    if max_groups < 2:
        return None, 0, 0, 0, psleep, E_UNSUPPORTED
    passes, first = 0, None
    for c0 in range(0, nchunks, max_groups // 2):
        nc = min(nchunks - c0, max_groups // 2)
        ngroups = 2 * nc
        nblk = ngroups * BPG
        if BPG > 1 and _env('FTMI_RNN_PAD', 1) and xcd_local and ngroups < 8 and 8 * BPG <= maxb:
            nblk = 8 * BPG
        first = nblk if first is None else first
        passes += 1
    return (('bidir', cell, H, U, WK, MODE, CST, NBL, CR), 256 if BPG == 1 else 320, passes, first,
            psleep, OK)


def _parent_launch(cell, B, H, mma, maxb):
    """(kernel coordinates, threads, passes, first-pass workgroups, psleep, status) of the
    parent's ftmi_rnn_bidir(cell, B, ., H, ..., mma) on a device of `maxb` CUs."""
    spread = bool(mma & SPREAD)
    mma &= ~SPREAD
    if (H != 512) if cell == 1 else (cell != 0 or H not in (64, 128, 256)):
        return None, 0, 0, 0, 0, E_UNSUPPORTED
    nchunks = (B + NB - 1) // NB
    xcd_local = _xcd_local_env()
    psleep_env = _env('FTMI_RNN_PSLEEP', -1)
    psleep = 3 if psleep_env < 0 else psleep_env
    if _gemv_path(cell, B, H):
        k8 = _env('FTMI_RNN_GEMV_KSEG', 0) == 8
        kseg = (8 if k8 else 16) if (cell == 1 or H == 256) else GV_KSEG
        return _launch_gemv(cell, H, 16, kseg, B, xcd_local, maxb, psleep)

    def launch(cell_, H_, U, WK, MODE, CST=False, NBL=NB, CR=False, ps=psleep):
        return _launch_rnn(cell_, H_, U, WK, MODE, CST, NBL, CR, B, nchunks, xcd_local, maxb, ps)

    def modes(cell_, H_, U, WKX, WKF):
        return launch(cell_, H_, U, WKX, mma) if mma in (1, 2) else launch(cell_, H_, U, WKF, 0)

    if cell == 0 and H == 64:
        if _rnn_units(cell, H, mma) == 32:
            return launch(0, 64, 32, 2, 2)
        return modes(0, 64, 64, 2, 4)
    if cell == 0 and H == 128:
        return modes(0, 128, 16, 4, 4)
    if mma == 2 and _cst_enabled() and ((cell == 1 and H == 512) or (cell == 0 and H == 256)):
        nb8 = _legacy_nbl(cell, B, H, mma, spread, maxb) == 8
        if _u8_path(cell, B, H, mma, spread, maxb):
            return launch(0, 256, 8, 4, 2, True, NB, _cellrows_enabled(), ps=_u8_psleep())
        if cell == 1:
            return launch(1, 512, 16, 4, 2, True, NB, _cellrows_enabled())
        return launch(0, 256, 16, 4, 2, True, 8 if nb8 else NB)
    if cell == 0 and H == 256:
        return modes(0, 256, 16, 4, 4)
    return modes(1, 512, 16, 4, 4)


def _parent_blocks(cell, B, H, mma, maxb):
    """The parent's ftmi_rnn_blocks, verbatim (its device_cu_count() is `maxb`)."""
    if B <= 0 or H <= 0 or H % 16 != 0:
        return 0
    spread = bool(mma & SPREAD)
    mma &= 0xFF
    if _gemv_path(cell, B, H):
        return (8 if _xcd_local_env() else 2) * (H // 16)
    if _u8_path(cell, B, H, mma, spread, maxb):
        ngroups = 2 * ((B + NB - 1) // NB)
        return (8 if ngroups < 8 and _xcd_local_env() else ngroups) * (H // 8)
    bpg = H // _rnn_units(cell, H, mma)
    max_groups = (maxb // bpg) & ~1
    if max_groups < 2:
        return 0
    nbl = _legacy_nbl(cell, B, H, mma, spread, maxb)
    nchunks = (B + nbl - 1) // nbl
    ngroups = 2 * min(nchunks, max_groups // 2)
    nblk = ngroups * bpg
    if bpg > 1 and ngroups < 8 and 8 * bpg <= maxb:
        nblk = 8 * bpg
    return nblk
# ---------------------------------------------------------------------------------------------


# every instantiation the library carries: rnn_gemv_kernel<cell, H, U, NBV, KSEG> for the three
# NBV of each <cell, H, U, KSEG>, and rnn_bidir_kernel<cell, H, U, WK, MODE, CST, NBL, CR>
INSTANCES = {('gemv', c, H, 16, nbv, k) for c, H, k in ((1, 512, 8), (1, 512, 16), (0, 256, 8),
                                                       (0, 256, 16), (0, 128, 8), (0, 64, 8))
             for nbv in (1, 2, 4)} | {
    ('bidir', 0, 64, 32, 2, 2, False, NB, False),
    ('bidir', 0, 64, 64, 2, 2, False, NB, False), ('bidir', 0, 64, 64, 2, 1, False, NB, False),
    ('bidir', 0, 64, 64, 4, 0, False, NB, False),
    *(('bidir', c, H, 16, 4, m, False, NB, False) for c, H in ((0, 128), (0, 256), (1, 512))
      for m in (2, 1, 0)),
    ('bidir', 0, 256, 16, 4, 2, True, NB, False), ('bidir', 0, 256, 16, 4, 2, True, 8, False),
    ('bidir', 0, 256, 8, 4, 2, True, NB, False), ('bidir', 0, 256, 8, 4, 2, True, NB, True),
    ('bidir', 1, 512, 16, 4, 2, True, NB, False), ('bidir', 1, 512, 16, 4, 2, True, NB, True)}

SWITCHES = {'GEMV': '0', 'GEMV_KSEG': '8', 'XCD_LOCAL': '0', 'PAD': '0', 'U64': '64', 'CSTORE': '0',
            'CELLROWS': '0', 'NB': '16', 'U8': '0', 'PSLEEP': '5'}
# all at their defaults, each alone, each together with GEMV=0 (B <= 4 hides them otherwise)
CONFIGS = [()] + [(n,) for n in SWITCHES] + [('GEMV', n) for n in SWITCHES if n != 'GEMV']
HS = (48, 64, 96, 128, 256, 512)
BS = (1, 2, 4, 5, 8, 16, 17, 33, 64, 65, 128, 130, 257, 512)
MMAS = (0, 1, 2, 0 | SPREAD, 1 | SPREAD, 2 | SPREAD)
CUS = (0, 256, 304, 64, 32, 8)  # 0: the device's own count, what ftmi_rnn_blocks plans for


def route(cell, B, H, mma, cus=256):
    r = RnnRoute()
    assert _lib.load().ftmi_rnn_route(cell, B, H, mma, cus, ctypes.byref(r)) == OK
    return r


def coords(r):
    if r.kernel == _lib.RNN_KERNEL_GEMV:
        return ('gemv', r.cell, r.H, r.units, r.nbv, r.kseg)
    return ('bidir', r.cell, r.H, r.units, r.wk, r.mode, bool(r.cst), r.nbl, bool(r.cr))


def launch_key(r):
    """The record in _parent_launch's terms (status alone when the launch is refused)."""
    if r.status != OK:
        return None, 0, 0, 0, 0, r.status
    return coords(r), r.threads, r.passes, r.first_blocks, r.psleep, OK


class _Switched:
    """The named switches at their non-default values, every other FTMI_RNN_* unset."""

    def __init__(self, names):
        self.set = {'FTMI_RNN_' + n: SWITCHES[n] for n in names}

    def __enter__(self):
        self.saved = {k: v for k, v in os.environ.items() if k.startswith('FTMI_RNN_')}
        for k in self.saved:
            del os.environ[k]
        os.environ.update(self.set)

    def __exit__(self, *exc):
        for k in self.set:
            del os.environ[k]
        os.environ.update(self.saved)


@functools.lru_cache(maxsize=None)
def sweep(config):
    """Every grid point under one switch configuration, computed once: (point, the record's
    launch key, its first-pass groups, the parent's launch, the parent's block count, and
    ftmi_rnn_blocks where the point plans for the device's own CUs)."""
    lib = _lib.load()
    rows = []
    with _Switched(config):
        for cell in (0, 1):
            for H in HS:
                for B in BS:
                    for mma in MMAS:
                        for cus in CUS:
                            r = route(cell, B, H, mma, cus)
                            parent = _parent_launch(cell, B, H, mma, r.cus)
                            if parent[5] != OK:
                                parent = (None, 0, 0, 0, 0, parent[5])
                            rows.append(((cell, B, H, mma, cus), launch_key(r),
                                         min(r.groups, r.groups_per_pass), parent,
                                         _parent_blocks(cell, B, H, mma, r.cus),
                                         lib.ftmi_rnn_blocks(cell, B, H, mma) if cus == 0 else None))
    assert len(rows) == 2 * 6 * 14 * 6 * 6
    return rows


def _shape_supported(cell, H):
    return (cell == 1 and H == 512) or (cell == 0 and H in (64, 128, 256))


def exempt(config, point, key, groups, parent):
    """Where the parent's ftmi_rnn_blocks did not report its own launch.  The first three are
    the disagreements the two copies had among themselves; the fourth is a shape that
    ftmi_rnn_bidir refuses outright (an H or cell without a kernel), for which the second copy
    still computed a grid and the header already promised 0."""
    cell, B, H, mma, cus = point
    bidir = key[0] is not None and key[0][0] == 'bidir'
    if ('XCD_LOCAL' in config or 'PAD' in config) and bidir and groups < 8:
        return 'unpadded'  # includes the U = 8 branch under PAD=0
    if parent[5] == E_UNSUPPORTED and _shape_supported(cell, H) and _gemv_path(cell, B, H):
        return 'gemv refusal'
    if not _shape_supported(cell, H):
        return 'no kernel'
    return None


@pytest.mark.parametrize('config', CONFIGS, ids=['+'.join(c) or 'defaults' for c in CONFIGS])
def test_route_is_the_parents_launch(config):
    """On every point the record is what the parent's launch path did, ftmi_rnn_blocks is the
    record's first-pass workgroups (0 when refused), and that is what the parent's
    ftmi_rnn_blocks reported wherever it reported its own launch."""
    with _Switched(config):
        for point, key, groups, parent, parent_blocks, abi_blocks in sweep(config):
            assert key == parent, (config, point)
            blocks = key[3]  # 0 when refused
            if abi_blocks is not None:
                assert abi_blocks == blocks, (config, point)
            if exempt(config, point, key, groups, parent) is None:
                assert parent_blocks == blocks, (config, point)


def test_no_exemption_at_the_defaults():
    """The exemptions are conditions, not measurements: at default switches on 256 CUs none of
    the three disagreements between the parent's two copies occurs, and the only points left
    out are the shapes without a kernel, where the launch is refused and the answer is 0."""
    reasons = {}
    with _Switched(()):
        for point, key, groups, parent, parent_blocks, _ in sweep(()):
            if point[4] == 256:
                reasons[point] = exempt((), point, key, groups, parent)
    assert set(reasons.values()) == {None, 'no kernel'}
    assert all(_shape_supported(p[0], p[2]) for p, why in reasons.items() if why is None)
    assert sum(why is None for why in reasons.values()) == 4 * 14 * 6  # every supported shape


def _case(config, cell, B, H, mma, cus=256):
    """(the parent's ftmi_rnn_blocks, the parent's launch, the new ftmi_rnn_blocks)."""
    with _Switched(config):
        r = route(cell, B, H, mma, cus)
        new = r.first_blocks if r.status == OK else 0
        if cus == 256:  # the count a machine without a device, and an MI355X, report
            assert _lib.load().ftmi_rnn_blocks(cell, B, H, mma) == new
        return _parent_blocks(cell, B, H, mma, cus), _parent_launch(cell, B, H, mma, cus), new


def test_left_out_xcd_local_off():
    """FTMI_RNN_XCD_LOCAL=0: launch_rnn did not pad (2 groups x 16), the copy reported 8 x 16."""
    was, launch, new = _case(('GEMV', 'XCD_LOCAL'), 0, 1, 256, 2)
    assert (was, launch[3], new) == (128, 32, 32)


def test_left_out_pad_off():
    """FTMI_RNN_PAD=0: the same for the switch the copy never read."""
    was, launch, new = _case(('PAD',), 1, 16, 512, 2)
    assert (was, launch[3], new) == (256, 64, 64)


def test_left_out_u8_under_pad_off():
    """The U = 8 branch checked FTMI_RNN_XCD_LOCAL but not FTMI_RNN_PAD."""
    was, launch, new = _case(('PAD',), 0, 17, 256, 2 | SPREAD)
    assert launch[0][3] == 8 and (was, launch[3], new) == (256, 128, 128)


def test_left_out_gemv_refusal():
    """launch_gemv refuses when a direction per XCD does not fit (8 x 16 workgroups on 64
    CUs), even with FTMI_RNN_XCD_LOCAL=0 where it would launch 2 x 16: the copy reported a
    grid for a launch that never ran."""
    for config, reported in (((), 128), (('XCD_LOCAL',), 32)):
        was, launch, new = _case(config, 0, 2, 256, 2, cus=64)
        assert (was, launch[5], new) == (reported, E_UNSUPPORTED, 0)


def test_left_out_shape_without_a_kernel():
    """H = 96: ftmi_rnn_bidir returns FTMI_E_UNSUPPORTED; the copy reported 8 x 6 workgroups."""
    was, launch, new = _case((), 0, 8, 96, 2)
    assert (was, launch[5], new) == (48, E_UNSUPPORTED, 0)


def test_every_instantiation_is_reached_and_none_is_missing():
    """The coordinates the sweep produces are exactly the library's instantiations: every
    record has its line in the launch table, and no line is dead."""
    seen = {key[0] for config in CONFIGS for _, key, *_ in sweep(config) if key[0] is not None}
    assert seen == INSTANCES
    assert len(INSTANCES) == 18 + 19


# (switch, a query (cell, B, H, mma[, cus]) that depends on it, the field that moves, its value
# with the switch unset, its value at the switch's SWITCHES value)
SWITCH_CASES = [
    ('GEMV', (1, 1, 512, 2), 'kernel', _lib.RNN_KERNEL_GEMV, _lib.RNN_KERNEL_BIDIR),
    ('GEMV_KSEG', (1, 1, 512, 2), 'kseg', 16, 8),
    ('XCD_LOCAL', (1, 1, 512, 2), 'first_blocks', 256, 64),
    ('PAD', (0, 16, 256, 2), 'first_blocks', 128, 32),
    ('U64', (0, 64, 64, 2), 'units', 32, 64),
    ('CSTORE', (1, 64, 512, 2), 'cst', 1, 0),
    ('CELLROWS', (1, 64, 512, 2), 'cr', 1, 0),
    ('NB', (0, 65, 256, 2 | SPREAD, 304), 'nbl', 8, 16),
    ('U8', (0, 64, 256, 2 | SPREAD), 'units', 8, 16),
    ('PSLEEP', (1, 64, 512, 2), 'psleep', 3, 5),
]
DEFAULTS = {'GEMV': '1', 'GEMV_KSEG': '16', 'XCD_LOCAL': '1', 'PAD': '1', 'U64': '32', 'CSTORE': '1',
            'CELLROWS': '1', 'NB': '8', 'U8': '1', 'PSLEEP': '3'}


def _fields(r):
    return tuple(getattr(r, n) for n, _ in RnnRoute._fields_)


@pytest.mark.parametrize('name,query,field,before,after', SWITCH_CASES, ids=[c[0] for c in SWITCH_CASES])
def test_switch_is_read_per_call_and_in_the_digest(name, query, field, before, after, monkeypatch):
    """Set between two calls, each switch changes the record of a shape that depends on it, and
    the digest; a second change in the same process is seen (FTMI_RNN_PAD, FTMI_RNN_U64 and
    FTMI_RNN_PSLEEP used to be kept from the first call); unset, digest and answers are back."""
    lib = _lib.load()
    for n in SWITCHES:
        monkeypatch.delenv('FTMI_RNN_' + n, raising=False)
    var = 'FTMI_RNN_' + name
    d0, r0, b0 = lib.ftmi_rnn_switches_digest(), route(*query), lib.ftmi_rnn_blocks(*query[:4])
    assert getattr(r0, field) == before
    monkeypatch.setenv(var, SWITCHES[name])
    d1, r1 = lib.ftmi_rnn_switches_digest(), route(*query)
    assert getattr(r1, field) == after and d1 != d0
    if len(query) == 4 and field == 'first_blocks':
        assert lib.ftmi_rnn_blocks(*query) == after
    monkeypatch.setenv(var, DEFAULTS[name])  # the second change
    assert getattr(route(*query), field) == before
    if name == 'PSLEEP':  # an explicit 3 is a set switch: another digest than unset
        assert lib.ftmi_rnn_switches_digest() not in (d0, d1)
    else:
        assert lib.ftmi_rnn_switches_digest() == d0
    monkeypatch.delenv(var)
    assert lib.ftmi_rnn_switches_digest() == d0 and _fields(route(*query)) == _fields(r0)
    assert lib.ftmi_rnn_blocks(*query[:4]) == b0


def test_digests_are_separate(monkeypatch):
    """A recurrence switch leaves the GEMM digest (and chain.policy_key) alone and the other
    way round: a recorded plan replays ftmi_rnn_bidir, which reads its switches itself."""
    from forwardtacotron_amd import chain
    lib = _lib.load()
    monkeypatch.delenv('FTMI_RNN_U8', raising=False)
    monkeypatch.delenv('FTMI_BANK_WALK', raising=False)
    g0, r0, k0 = lib.ftmi_gemm_switches_digest(), lib.ftmi_rnn_switches_digest(), chain.policy_key()
    monkeypatch.setenv('FTMI_RNN_U8', '0')
    assert lib.ftmi_gemm_switches_digest() == g0 and chain.policy_key() == k0
    assert lib.ftmi_rnn_switches_digest() != r0
    monkeypatch.delenv('FTMI_RNN_U8')
    monkeypatch.setenv('FTMI_BANK_WALK', '1')
    assert lib.ftmi_gemm_switches_digest() != g0 and lib.ftmi_rnn_switches_digest() == r0


def test_struct_matches_header():
    """The ctypes mirror has the header's fields in the header's order, all int32_t."""
    text = HEADER.read_text()
    body = re.search(r'typedef struct ftmi_rnn_route \{(.*?)\} ftmi_rnn_route_t;', text, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    assert re.findall(r'(\w+)\s+(\w+);', body) == [('int32_t', n) for n, _ in RnnRoute._fields_]
    assert ctypes.sizeof(RnnRoute) == 4 * len(RnnRoute._fields_)
    names = re.search(r'enum \{ (FTMI_RNN_KERNEL_NONE.*?)\};', text, re.S).group(1)
    names = re.findall(r'FTMI_(RNN_KERNEL_\w+)', re.sub(r'/\*.*?\*/', '', names, flags=re.S))
    assert [getattr(_lib, n) for n in names] == [0, 1, 2]


def test_query_argument_errors():
    lib = _lib.load()
    r = RnnRoute()
    assert lib.ftmi_rnn_route(0, 64, 256, 2, 256, None) == E_ARG
    assert lib.ftmi_rnn_route(0, 0, 256, 2, 256, ctypes.byref(r)) == E_ARG
    assert lib.ftmi_rnn_route(0, 64, 0, 2, 256, ctypes.byref(r)) == E_ARG
    assert lib.ftmi_rnn_route(0, 64, 256, 3, 256, ctypes.byref(r)) == E_ARG  # as ftmi_rnn_bidir
    assert lib.ftmi_rnn_route(0, 64, 256, 2, -1, ctypes.byref(r)) == E_ARG
    assert lib.ftmi_rnn_route(2, 64, 256, 2, 256, ctypes.byref(r)) == OK and r.status == E_UNSUPPORTED
    assert lib.ftmi_rnn_blocks(0, 0, 256, 2) == 0 and lib.ftmi_rnn_blocks(0, 64, 96, 2) == 0
