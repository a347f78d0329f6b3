"""The library's kernel decision, asked through the ftmi_*_route queries (no GPU needed:
host-only functions that launch nothing and read no pointer).

Every address here is fabricated (16-byte aligned unless a case says otherwise), never
device memory.  The `_parent_*` functions are the Python restatement of the selection rules
that `ops.py` carried before the library exported its decision, copied verbatim: the record
of what Python used to assume, against which the library's answers are swept."""
import ctypes
import os
import re
from pathlib import Path
from typing import Optional

import pytest
import torch

from forwardtacotron_amd import _lib, ops
from forwardtacotron_amd._lib import ConvArgs, GemmRoute

HEADER = Path(__file__).resolve().parent.parent / 'include' / 'ftmi.h'
FAKE = 1 << 12
E_UNSUPPORTED = 1003
SLAB_KERNELS = (_lib.ROUTE_SLAB, _lib.ROUTE_SLAB_WS, _lib.ROUTE_SLAB_PF)

# ---- the parent's mirror (forwardtacotron_amd/ops.py before ABI 21), verbatim -------------
SLAB = os.environ.get('FTMI_GEMM_SLAB', '1') != '0'


SLAB_K1_NMIN = int(os.environ.get('FTMI_SLAB_K1_NMIN', 128))  # gemm.hip slab_ok


def _parent_slab(mma: int, T: int, To: int, Cin: int, k: int, N: int, M: int) -> bool:
    """Whether ftmi_conv1d takes the slab kernel (gemm.hip slab_ok)."""
    return (SLAB and mma == 2 and To == T and Cin % 16 == 0 and k <= 16 and (k > 1 or N >= SLAB_K1_NMIN)
            and M * N * k * Cin >= int(os.environ.get('FTMI_GEMM_SLAB_MIN', 0)))


SKINNY_MMAX = 256          # gemm.hip SK_MMAX
SKINNY_MMAX_NARROW = 1024  # gemm.hip SK_MMAX_NARROW (single group, N <= 128)


def _parent_skinny(mma: int, T: int, To: int, Cin: int, k: int, M: int, N: Optional[int] = None) -> bool:
    """Whether a conv takes the weight-streaming skinny kernel (gemm.hip skinny_ok): few
    rows (B = 1 generation) — or a narrow single-group linear (N <= 128) with up to 1024
    rows — f16x3, same-length output.  N = None: a multi-group call (conv bank)."""
    rows_ok = 0 < M <= SKINNY_MMAX or (N is not None and N <= 128 and 0 < M <= SKINNY_MMAX_NARROW)
    return (os.environ.get('FTMI_GEMM_SKINNY', '1') != '0' and mma == 2 and To == T
            and Cin % 16 == 0 and k <= 16 and rows_ok)


def _parent_skinny_split(Cin: int) -> int:
    """Channel split of the skinny kernel: two 32-channel chunks per block."""
    nch = -(-Cin // 32)
    per = int(os.environ.get('FTMI_SKINNY_CPB', 2))  # chunks per block (1 or 2; A/B runs)
    return -(-nch // per)


def _parent_bank_halves(mma: int, B: int, T: int, Cin: int, K: int, Cout: int) -> bool:
    """Whether conv_bank takes the one-launch channel-halves kernel (gemm.hip
    bank_halves_ok): f16x3, one row tile of at most 128 rows (batch-1 generation, BASELINE
    config c2), Cin a multiple of 64 up to 256, even K, (K / 2)(Cout / 16) a multiple of 8 up
    to 512 (8 arrival counters per unit).
    FTMI_BANK_HALVES=0 (read per call) keeps the channel-split kernel + finish."""
    return (os.environ.get('FTMI_BANK_HALVES', '1') != '0' and mma == 2 and 0 < B * T <= 128
            and Cin % 64 == 0 and Cin <= 256 and K % 2 == 0 and Cout % 16 == 0
            and (K // 2) * (Cout // 16) % 8 == 0 and (K // 2) * (Cout // 16) <= 512 and K <= 16)


def _parent_bank_pools(m, wsp, B, T, Cin, K, Cout) -> bool:
    """The parent's ops.bank_pools after its `_gemm_mma` line (POOL_BANK at its default)."""
    return (m == 2 and wsp is not None and not _parent_skinny(m, T, T, Cin, K, B * T)
            and _parent_slab(m, T, T, Cin, K, Cout, B * T))
# -------------------------------------------------------------------------------------------


# (matrix path, split planes) as ops._gemm_mma hands them to a launch: f16x3 without its f16
# planes runs as bf16x6, which splits in-kernel without bf16 pieces
MMA_ASKED = [(0, False), (0, True), (1, False), (1, True), (2, False), (2, True)]


def _effective(mma, planes):
    """ops._gemm_mma's (m, w_split pointer) for mma in {0, 1, 2} with / without split planes
    of that path's kind."""
    if mma == 2 and not planes:
        return 1, None
    return mma, (FAKE if planes and mma else None)


def conv_args(B, T, Cin, N, k, mma, wsp, To=0, **over):
    a = ConvArgs()
    a.x, a.x_stride, a.B, a.T, a.Cin = FAKE, Cin, B, T, Cin
    a.w, a.N, a.k, a.pad = FAKE, N, k, k // 2
    a.y, a.y_stride, a.T_out, a.mma, a.w_split = FAKE, N, To, mma, wsp
    for key, v in over.items():
        setattr(a, key, v)
    return a


def conv_route(a):
    r = GemmRoute()
    assert _lib.load().ftmi_conv1d_route(ctypes.byref(a), ctypes.byref(r)) == 0
    return r


class Rows:
    """What ops.bank_pools reads of its input: shape, row stride, address."""

    def __init__(self, B, T, C, stride=None, ptr=FAKE):
        self.shape, self.row, self.ptr = (B, T, C), stride or C, ptr

    def size(self, i):
        return self.shape[i]

    def stride(self, i):
        return (self.shape[1] * self.row, self.row, 1)[i]

    def data_ptr(self):
        return self.ptr


class Planes:
    """An f16x3 split block as ops._gemm_mma sees it."""
    dtype = torch.uint8

    def data_ptr(self):
        return FAKE


def test_struct_matches_header():
    """The ctypes mirror has the C layout (LP64) and the header's field order."""
    assert ctypes.sizeof(GemmRoute) == 24
    body = re.search(r'typedef struct ftmi_gemm_route \{(.*?)\} ftmi_gemm_route;', HEADER.read_text(),
                     re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = re.findall(r'(int32_t|int64_t)\s+(\w+);', body)
    ctype = {'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64}
    assert [(n, ctype[t]) for t, n in fields] == list(GemmRoute._fields_)
    names = re.search(r'enum \{ (FTMI_ROUTE_UNSUPPORTED.*?)\};', HEADER.read_text(), re.S).group(1)
    names = re.findall(r'FTMI_(ROUTE_\w+)', re.sub(r'/\*.*?\*/', '', names, flags=re.S))
    assert [getattr(_lib, n) for n in names] == list(range(12))


MS = (1, 64, 120, 128, 129, 256, 257, 816, 1024, 1025, 12800)
CINS = (16, 48, 64, 80, 256, 512)


def test_conv_routes_agree_with_the_parent_mirror():
    """Over the grid of shapes, on operands that satisfy what the mirror left out (aligned,
    strides % 4 == 0, N % 4 == 0, M * x_stride < 2^31): the library takes the skinny kernel
    exactly where the parent's `_skinny` said so, with the split `_skinny_split` gave; the
    slab kernels exactly where `_slab` (and not `_skinny`) said so, with no required split;
    and neither elsewhere.  T is the row count (B = 1); the output has T or T + 1 frames."""
    checked = 0
    for T in MS:
        for Cin in CINS:
            for k in (1, 2, 5, 9, 16, 17):
                for N in (80, 128, 132, 256, 512):
                    for To in (T, T + 1):
                        for mma, planes in MMA_ASKED:
                            m, wsp = _effective(mma, planes)
                            r = conv_route(conv_args(1, T, Cin, N, k, m, wsp, To))
                            M = To
                            where = (T, Cin, k, N, To, mma, planes)
                            skinny = _parent_skinny(m, T, To, Cin, k, M, N)
                            slab = not skinny and _parent_slab(m, T, To, Cin, k, N, M)
                            assert (r.kernel in _lib.ROUTE_SKINNIES) == skinny, where
                            assert (r.kernel in SLAB_KERNELS) == slab, where
                            assert r.kernel != _lib.ROUTE_UNSUPPORTED and not r.pooled, where
                            if skinny:
                                assert max(r.split_k, 1) == _parent_skinny_split(Cin), where
                                assert r.ws_floats == r.split_k * M * N, where
                            else:
                                assert (r.split_k, r.ws_floats) == (0, 0), where
                            checked += 1
    assert checked == 11 * 6 * 6 * 5 * 2 * 6


def test_bank_routes_agree_with_the_parent_mirror():
    """The same for banks, unpooled and pooled: halves where `_bank_halves` said so (split 2,
    the workspace ftmi_conv_bank_halves_ws_floats gives), else skinny where `_skinny` said so
    with `_skinny_split`'s split over the K * Cout columns, else no split; the pooled bank
    never splits; and `ops.bank_pools` answers as the parent's did."""
    lib = _lib.load()
    checked = 0
    for T in MS:
        for Cin in CINS:
            for K in (2, 8, 16):
                for Cout in (16, 128, 256):
                    for mma, planes in MMA_ASKED:
                        m, wsp = _effective(mma, planes)
                        where = (T, Cin, K, Cout, mma, planes)
                        r = ops._bank_route(m, 1, T, Cin, K, Cout, wsp=wsp)
                        halves = _parent_bank_halves(m, 1, T, Cin, K, Cout)
                        skinny = not halves and _parent_skinny(m, T, T, Cin, K, T)
                        slab = not halves and not skinny and _parent_slab(m, T, T, Cin, K, Cout, T)
                        assert (r.kernel == _lib.ROUTE_BANK_HALVES) == halves, where
                        assert ops._bank_halves(m, 1, T, Cin, K, Cout) == halves, where
                        assert (r.kernel in _lib.ROUTE_SKINNIES) == skinny, where
                        assert (r.kernel in SLAB_KERNELS) == slab, where
                        assert r.kernel != _lib.ROUTE_UNSUPPORTED and not r.pooled, where
                        if halves:
                            assert r.split_k == 2, where
                            assert r.ws_floats == lib.ftmi_conv_bank_halves_ws_floats(1, T, K, Cout) > 0
                        elif skinny and _parent_skinny_split(Cin) > 1:
                            assert r.split_k == _parent_skinny_split(Cin), where
                            assert r.ws_floats == r.split_k * T * K * Cout, where
                        else:
                            assert (r.split_k, r.ws_floats) == (0, 0), where
                        # pool on: conv_bank(pool=True) passed no split and no halves flag
                        pools = _parent_bank_pools(m, wsp, 1, T, Cin, K, Cout)
                        rp = ops._bank_route(m, 1, T, Cin, K, Cout, wsp=wsp, flags=ops.BANK_POOL)
                        assert (rp.split_k, rp.ws_floats) == (0, 0), where
                        assert bool(rp.pooled) == (rp.kernel != _lib.ROUTE_UNSUPPORTED), where
                        if pools:
                            assert rp.pooled and rp.kernel in _lib.ROUTE_SLABS, where
                        w3 = Planes() if wsp is not None and m == 2 else None
                        assert ops.bank_pools(Rows(1, T, Cin), K, Cout, m, w3) == pools, where
                        checked += 1
    assert checked == 11 * 6 * 3 * 3 * 6


def test_highway_routes_agree_with_the_parent_mirror():
    """ops.highway's inline test: f16x3 with planes, C % 16 == 0, at most 1024 rows -> the
    skinny kernel through `_skinny_split(C)` partial sums (a workspace even for one split);
    elsewhere no split."""
    lib = _lib.load()
    for M in MS:
        for C in (32, 64, 256, 512):
            for mma, planes in MMA_ASKED:
                m, wsp = _effective(mma, planes)
                r = GemmRoute()
                assert lib.ftmi_highway_route(FAKE, C, M, C, FAKE, wsp, FAKE, FAKE, 2 * FAKE, C, m,
                                              None, ctypes.byref(r)) == 0
                skinny = (m == 2 and wsp is not None and C % 16 == 0 and 0 < M <= SKINNY_MMAX_NARROW)
                assert (r.kernel in _lib.ROUTE_SKINNIES) == skinny, (M, C, mma, planes)
                if skinny:
                    assert r.split_k == _parent_skinny_split(C) >= 1
                    assert r.ws_floats == r.split_k * M * 2 * C
                else:
                    assert (r.split_k, r.ws_floats) == (0, 0)


# ---- one case per condition the mirror left out -------------------------------------------
# each: a conv the parent's `_slab` called a slab launch and the library does not, and the
# pooled bank of the same defect, which the library refuses

def _not_slab(a, T, Cin, k, N):
    assert _parent_slab(2, T, T, Cin, k, N, a.B * T) and not _parent_skinny(2, T, T, Cin, k, a.B * T, N)
    r = conv_route(a)
    assert r.kernel == _lib.ROUTE_X6B_F16 and r.split_k == 0
    ok = conv_route(conv_args(a.B, T, Cin, 256, k, 2, FAKE))  # the same shape without the defect
    assert ok.kernel in SLAB_KERNELS


def _no_pooled_store(B, T, Cin, K, Cout, **at):
    r = ops._bank_route(2, B, T, Cin, K, Cout, flags=ops.BANK_POOL, **at)
    assert (r.kernel, r.pooled) == (_lib.ROUTE_UNSUPPORTED, 0)
    assert _parent_bank_pools(2, FAKE, B, T, Cin, K, Cout)
    assert ops._bank_route(2, B, T, Cin, K, 256, flags=ops.BANK_POOL).pooled  # without the defect


def test_left_out_column_count():
    """N % 4 != 0 (the slab epilogue moves float4s)."""
    _not_slab(conv_args(1, 1024, 256, 130, 5, 2, FAKE, y_stride=132), 1024, 256, 5, 130)
    _no_pooled_store(1, 1024, 256, 8, 130)
    assert not ops.bank_pools(Rows(1, 1024, 256), 8, 130, 2, Planes())


def test_left_out_output_alignment():
    """A y pointer 8 bytes off.  `bank_pools` never sees y (conv_bank allocates it, aligned
    and dense), so for the bank the library's answer is asserted on the query."""
    _not_slab(conv_args(1, 1024, 256, 256, 5, 2, FAKE, y=FAKE + 8), 1024, 256, 5, 256)
    _no_pooled_store(1, 1024, 256, 8, 256, y=FAKE + 8)


def test_left_out_output_stride():
    """y_stride % 4 != 0 (idem for the bank)."""
    _not_slab(conv_args(1, 1024, 256, 256, 5, 2, FAKE, y_stride=258), 1024, 256, 5, 256)
    _no_pooled_store(1, 1024, 256, 8, 256, ys=8 * 256 + 2)


def test_left_out_32_bit_row_offsets():
    """M * x_stride >= 2^31: 2^20 rows of the postnet's 2048-float split rows."""
    B, T = 1024, 1024
    _not_slab(conv_args(B, T, 256, 256, 5, 2, FAKE, x_stride=2048), T, 256, 5, 256)
    _no_pooled_store(B, T, 256, 8, 256, xs=2048)
    assert not ops.bank_pools(Rows(B, T, 256, stride=2048), 8, 256, 2, Planes())
    assert ops.bank_pools(Rows(B, T - 1, 256, stride=2048), 8, 256, 2, Planes())


def test_left_out_split_with_several_groups():
    """split_req > 1 with several groups: a few-row bank on split rows.  The parent passed it
    the skinny kernel's split, which the slab kernels (the only ones that stage split rows)
    refuse for a bank; the library asks for no split there, and still refuses one."""
    B, T, Cin, K, Cout = 1, 120, 128, 8, 256
    assert _parent_skinny(2, T, T, Cin, K, B * T) and _parent_skinny_split(Cin) == 2
    r = ops._bank_route(2, B, T, Cin, K, Cout, flags=ops.BANK_X_SPLIT)
    assert r.kernel in SLAB_KERNELS and (r.split_k, r.ws_floats) == (0, 0)
    rc = _lib.load().ftmi_conv_bank_split(FAKE, Cin, B, T, Cin, FAKE, FAKE, K, Cout, FAKE, FAKE, FAKE,
                                          K * Cout, 2, None, 2, FAKE, ops.BANK_X_SPLIT, None)
    assert rc == E_UNSUPPORTED  # refused on the host, before any launch


# ---- switches -----------------------------------------------------------------------------

def _conv(T, Cin, N, k):
    return lambda: conv_route(conv_args(1, T, Cin, N, k, 2, FAKE))


def _bank(T, Cin, K, Cout, flags=0):
    return lambda: ops._bank_route(2, 1, T, Cin, K, Cout, flags=flags)


def _key(r):
    return (r.kernel, r.split_k, r.ws_floats, r.pooled, r.band)


SWITCH_CASES = [
    ('FTMI_GEMM_SLAB', '0', _conv(1024, 256, 256, 5), _lib.ROUTE_SLAB_WS, _lib.ROUTE_X6B_F16),
    ('FTMI_GEMM_SLAB_MIN', str(1 << 62), _conv(1024, 256, 256, 5), _lib.ROUTE_SLAB_WS, _lib.ROUTE_X6B_F16),
    ('FTMI_GEMM_SLAB_WS', '0', _conv(1024, 256, 256, 5), _lib.ROUTE_SLAB_WS, _lib.ROUTE_SLAB),
    ('FTMI_SLAB_K1_NMIN', '64', _conv(2048, 256, 80, 1), _lib.ROUTE_X6B_F16, _lib.ROUTE_SLAB_PF),
    ('FTMI_SLAB_PF', '0', _conv(2048, 256, 256, 1), _lib.ROUTE_SLAB_PF, _lib.ROUTE_SLAB),
    ('FTMI_SLAB_BAND', '0', _conv(2048, 256, 256, 1), _lib.ROUTE_SLAB_PF, _lib.ROUTE_SLAB_PF),
    ('FTMI_GEMM_SKINNY', '0', _conv(120, 256, 256, 5), _lib.ROUTE_SKINNY, _lib.ROUTE_SLAB_WS),
    ('FTMI_SKINNY_CPB', '1', _conv(120, 256, 256, 5), _lib.ROUTE_SKINNY, _lib.ROUTE_SKINNY),
    ('FTMI_BANK_BALANCED', '0', _bank(200, 256, 8, 128), _lib.ROUTE_SKINNY_BANK, _lib.ROUTE_SKINNY),
    ('FTMI_BANK_WALK', '1', _bank(1024, 80, 8, 256, 1), _lib.ROUTE_SLAB_WS, _lib.ROUTE_BANK_WALK),
    ('FTMI_BANK_HALVES', '0', _bank(120, 256, 16, 256), _lib.ROUTE_BANK_HALVES, _lib.ROUTE_SKINNY_BANK),
]


@pytest.mark.parametrize('name,value,query,before,after', SWITCH_CASES, ids=[c[0] for c in SWITCH_CASES])
def test_switch_is_read_per_call_and_in_the_digest(name, value, query, before, after, monkeypatch):
    """Set between two calls, each routing switch changes the route of a shape that depends
    on it (the kernel; FTMI_SLAB_BAND the tile order, FTMI_SKINNY_CPB the required split) and
    the digest; both are back after the switch is unset."""
    lib = _lib.load()
    monkeypatch.delenv(name, raising=False)
    d0, r0 = lib.ftmi_gemm_switches_digest(), query()
    assert r0.kernel == before
    monkeypatch.setenv(name, value)
    d1, r1 = lib.ftmi_gemm_switches_digest(), query()
    assert r1.kernel == after and _key(r1) != _key(r0)
    assert d1 != d0
    monkeypatch.delenv(name)
    assert lib.ftmi_gemm_switches_digest() == d0 and _key(query()) == _key(r0)


def test_switch_details(monkeypatch):
    """What the two switches that keep the kernel change: the band and the split."""
    monkeypatch.delenv('FTMI_SLAB_BAND', raising=False)
    monkeypatch.delenv('FTMI_SKINNY_CPB', raising=False)
    assert _conv(2048, 256, 256, 1)().band == 2 and _conv(120, 256, 256, 5)().split_k == 4
    monkeypatch.setenv('FTMI_SLAB_BAND', '0')
    monkeypatch.setenv('FTMI_SKINNY_CPB', '1')
    assert _conv(2048, 256, 256, 1)().band == 0 and _conv(120, 256, 256, 5)().split_k == 8
    monkeypatch.setenv('FTMI_SKINNY_CPB', '7')  # beyond the kernel's two chunks per block: clamped
    assert _conv(120, 256, 256, 5)().split_k == 4


def test_policy_key_follows_the_digest(monkeypatch):
    """chain.policy_key lists no switch of its own: any routing switch changes it."""
    from forwardtacotron_amd import chain
    monkeypatch.delenv('FTMI_BANK_WALK', raising=False)
    k0 = chain.policy_key()
    monkeypatch.setenv('FTMI_BANK_WALK', '1')
    assert chain.policy_key() != k0
    monkeypatch.delenv('FTMI_BANK_WALK')
    assert chain.policy_key() == k0


def test_removed_switch_changes_nothing(monkeypatch):
    """FTMI_GEMM_X6 (the removed bf16x6 variants) is no longer read: bf16x6 with pre-split
    pieces takes x6b, without them x6, and the digest does not move."""
    lib = _lib.load()
    monkeypatch.delenv('FTMI_GEMM_X6', raising=False)

    def routes():
        return [_key(conv_route(conv_args(1, T, 256, 256, 5, 1, wsp)))
                for T in (120, 1024) for wsp in (None, FAKE)]
    d0, r0 = lib.ftmi_gemm_switches_digest(), routes()
    assert [k[0] for k in r0] == [_lib.ROUTE_X6, _lib.ROUTE_X6B_BF16] * 2
    for v in ('0', '2', '3'):
        monkeypatch.setenv('FTMI_GEMM_X6', v)
        assert lib.ftmi_gemm_switches_digest() == d0 and routes() == r0


def test_queries_return_the_entry_points_argument_errors():
    lib = _lib.load()
    r = GemmRoute()
    assert lib.ftmi_conv1d_route(None, ctypes.byref(r)) == 1001
    a = conv_args(1, 8, 16, 8, 3, 0, None)
    assert lib.ftmi_conv1d_route(ctypes.byref(a), None) == 1001
    a.x_stride = 18
    assert lib.ftmi_conv1d_route(ctypes.byref(a), ctypes.byref(r)) == 1004
    assert lib.ftmi_conv_bank_route(FAKE, 16, 1, 8, 16, FAKE, FAKE, 4, 8, FAKE, FAKE, FAKE, 32, 2, None,
                                    ops.BANK_HALVES, ctypes.byref(r)) == 1001  # not a query flag
    assert lib.ftmi_highway_route(FAKE, 32, 8, 32, FAKE, None, FAKE, FAKE, FAKE, 32, 2, None,
                                  ctypes.byref(r)) == 1001  # x == y; f16x3 without planes
    a = conv_args(1, 120, 256, 256, 5, 2, FAKE, split_k=3)  # a split without a workspace: ignored
    assert conv_route(a).split_k == 4
