"""Tensor-level wrappers over libftmi.so.

Every function takes HIP device tensors (fp32 unless stated), allocates the outputs with
torch's caching allocator (plumbing only), and enqueues ONE ftmi_* entry point on
torch's current stream.  Nothing here computes on the host or falls back to torch ops:
a CPU tensor or a missing library raises.
"""
from __future__ import annotations

import contextlib
import ctypes
import os
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib, probe
from ._lib import ConvArgs
from .probe import launch

_f32 = torch.float32

# Matrix path of the dense contractions (include/ftmi.h FTMI_MMA_*): 2 = f16x3 split
# (default; fp32-level accuracy at 5.3x the fp32 MFMA rate, activations < 65504),
# 1 = bf16x6 split (fp32-accurate, 2.7x), 0 = plain fp32 MFMA.  FTMI_MMA overrides.
MMA = int(os.environ.get('FTMI_MMA', '2'))
# the recurrences' W_hh h path (same codes; FTMI_RNN_MMA overrides)
RNN_MMA = int(os.environ.get('FTMI_RNN_MMA', '2'))

# Status word (include/ftmi.h FTMI_STATUS_*).  Every GEMM / recurrence launch ORs into a
# per-device word: bit 0 = an f16x3 accumulator became non-finite (an activation beyond the
# f16 range), bit 1 = a W_hh entry beyond the f16 range, bit 2 = a recurrence workgroup
# timed out waiting for its group (its output is invalid).  The model entry points zero it,
# run, read it once at the end: bit 2 raises RnnTimeout; bits 0-1 run the call again under
# `exact_paths()` (fp32 MFMA everywhere), which has no range limit.
STATUS_F16_RANGE, STATUS_WHH_RANGE, STATUS_RNN_TIMEOUT = 1, 2, 4
_STATUS = {}
_FORCED = []  # stack of (gemm mma, rnn mma) overrides


def status_word(device) -> torch.Tensor:
    t = _STATUS.get(device)  # fast path: an indexed torch.device seen before
    if t is not None:
        return t
    dev = torch.device(device)
    if dev.index is None:
        dev = torch.device(dev.type, torch.cuda.current_device())
    t = _STATUS.get(dev)
    if t is None:
        t = _STATUS[dev] = torch.zeros(1, device=dev, dtype=torch.int32)
    return t


def forced_exact() -> bool:
    """True inside exact_paths() (the range guard's rerun): nothing captured may replay."""
    return bool(_FORCED)


@contextlib.contextmanager
def exact_paths():
    """Run the enclosed calls on the range-unlimited fp32 MFMA paths (GEMMs and
    recurrences)."""
    _FORCED.append((0, 0))
    try:
        yield
    finally:
        _FORCED.pop()


def _gemm_mma(mma: Optional[int], w_split):
    """(matrix path, w_split pointer) of one GEMM launch.  f16x3 needs the f16 planes
    (uint8 block of split_weights_f16); without them the launch uses bf16x6, which takes
    its bf16 pieces (split_weights) or splits the weights in-kernel."""
    m = _FORCED[-1][0] if _FORCED else (MMA if mma is None else mma)
    has16 = w_split is not None and w_split.dtype == torch.uint8
    hasbf = w_split is not None and w_split.dtype == torch.bfloat16
    if m == 2 and not has16:
        m = 1
    ptr = w_split.data_ptr() if (m == 2 and has16) or (m == 1 and hasbf) else None
    return m, ptr


def _rnn_mma() -> int:
    return _FORCED[-1][1] if _FORCED else RNN_MMA


class RnnTimeout(RuntimeError):
    """A persistent recurrence could not run all its workgroups at once (another stream's
    persistent kernels held CUs): its output is invalid, so the call fails."""


def run_checked(fn, device, reduce=None):
    """fn() with the status-word checks: zero the word, run, read it (one host sync).
    A recurrence timeout reruns fn() once with the recurrences compact
    (compact_recurrences()); a second one raises RnnTimeout.  A range bit (f16x3 overflow) runs fn() again
    under exact_paths() — which calls the model's pitch / energy callbacks a second time
    (the first pass's callback outputs derive from the out-of-range predictions and are not
    reused).  reduce(word) -> word combines the status over ranks (sharded generation)
    before the decision."""
    st = status_word(device)

    def attempt():
        st.zero_()
        res = fn()
        s = st if reduce is None else reduce(st)
        w = int(s.item())
        if w & STATUS_RNN_TIMEOUT:
            raise RnnTimeout('a recurrence workgroup timed out waiting for its group (not all '
                             'workgroups co-resident): the result is invalid')
        return res, w

    try:
        out, w = attempt()
    except RnnTimeout:
        # a persistent recurrence could not seat every workgroup at once: another kernel
        # (an RCCL collective, a copy, another process) held CUs past the spin limit.  The
        # launch is rerun once in the compact form (a spread recurrence otherwise takes all
        # 256 CUs); a second timeout raises.
        with compact_recurrences():
            out, w = attempt()
    if w and not _FORCED:
        # the rerun is checked like the first pass (a timeout there raises too; its range
        # bits cannot recur on the range-unlimited paths); afterwards the word shows the
        # bits that caused it, as the call's record
        with exact_paths():
            out, _ = attempt()
        st.fill_(w)
    return out


_COMPACT = []  # non-empty: recurrences ignore `spread` (run_checked's timeout rerun)


@contextlib.contextmanager
def compact_recurrences():
    """Run the enclosed recurrences in their compact form (`spread` ignored: 16 live sequences
    per group, fewer workgroups than CUs where the shape allows)."""
    _COMPACT.append(True)
    try:
        yield
    finally:
        _COMPACT.pop()


def _num_cus() -> int:
    n = getattr(_num_cus, 'v', None)
    if n is None:
        n = _num_cus.v = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    return n


def _route(query: str, *args) -> _lib.GemmRoute:
    """The kernel the library will take for the launch these arguments describe, with the
    split and workspace floats that kernel requires (include/ftmi.h ftmi_*_route: the
    library's one decision function, host only).  Arguments the entry point refuses give an
    empty route: the launch that follows reports them."""
    r = _lib.GemmRoute()
    if getattr(_lib.load(), query)(*args, ctypes.byref(r)) != 0:
        return _lib.GemmRoute()
    return r


def _split_k(M: int, N: int, K: int, mma: int, slab: bool = False, Cin: int = 0) -> int:
    """Split K when the tile grid cannot fill the chip (x6 / h3 kernels: 2 workgroups per
    CU; slab kernel: 256 x 128 tiles, 1 per CU, split over 32-channel chunks) and K is long
    enough for the partial-sum round trip to pay."""
    if slab:
        # one workgroup per CU: model the time as (rounds of workgroups) x (steps per
        # workgroup, ~1.8 us each) + the partial-sum round trip of a split (sp x M x N fp32
        # written and read back, priced at 1 TB/s, plus 20 us for the finishing launch —
        # calibrated below)
        tiles = -(-M // 256) * -(-N // 128)
        cus = _num_cus()
        nch = -(-Cin // 32)
        k = K // Cin if Cin else 1

        # the round trip as measured in the model's phoneme phase (round 5, r5_timeline_c3:
        # 24-39 us for 2 splits of 12,800 x 256 beside the other streams — the old 5 TB/s +
        # 5 us model priced it at 15 us and split proj2 / the predictor convs where the
        # finish costs more than it saves): 1 TB/s + 20 us.  Interleaved A/B (5 / 3 rounds,
        # profiles/r5_ab_splitk*.jsonl): c3 8.12-8.20 -> 8.01-8.15, c5 11.33-11.40 ->
        # 11.19-11.26 ms/step, c2 unchanged (2.59-2.65 / 2.60-2.68)
        def t_us(sp):
            run = -(-tiles * sp // cus) * -(-nch // sp) * k * 1.8
            return run + (sp * M * N * 8 / 1e6 + 20.0 if sp > 1 else 0.0)
        return int(min(range(1, min(8, nch) + 1), key=t_us))
    if mma == 0 or K < 2048:
        return 1
    tiles = -(-M // 128) * -(-N // 128)
    slots = 2 * _num_cus()
    if tiles >= slots:
        return 1
    return int(min(8, -(-slots // tiles), K // 1024))


if hasattr(torch._C, '_cuda_getCurrentRawStream'):
    def _stream() -> int:
        """hipStream_t of torch's current stream (the raw-handle query skips the Stream
        object torch.cuda.current_stream() builds: host time on every launch)."""
        return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice())
else:  # pragma: no cover
    def _stream() -> int:
        return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _dev(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError('forwardtacotron_amd ops run on a HIP device only (got a CPU '
                               'tensor); there is no CPU fallback')


def _new(*shape, device, dtype=_f32) -> torch.Tensor:
    """torch.empty for an op's output or workspace; while a launch list is being recorded
    (chain.py) the recorder notes it, so the plan can lay it out in its one workspace."""
    t = torch.empty(*shape, device=device, dtype=dtype)
    r = probe._RECORDER
    if r is not None:
        r.allocs.append(t)
    return t


def _rows(x: torch.Tensor) -> Tuple[int, int, int, int]:
    """(B, T, C, row_stride) of a channels-last (B, T, C) view with uniformly strided rows."""
    if x.dim() != 3 or x.stride(2) != 1 or x.stride(0) != x.size(1) * x.stride(1):
        raise ValueError(f'expected a (B, T, C) channels-last view with uniform row stride, got '
                         f'shape {tuple(x.shape)} strides {x.stride()}')
    if x.dtype != _f32:
        raise TypeError('fp32 expected')
    return x.size(0), x.size(1), x.size(2), x.stride(1)


def embedding(ids: torch.Tensor, table: torch.Tensor, err: Optional[torch.Tensor] = None) -> torch.Tensor:
    """nn.Embedding forward: (B, T) int64 -> (B, T, dim)."""
    _dev(ids, table)
    ids = ids.contiguous()
    if ids.dtype != torch.int64:
        ids = ids.long()
    table = table.contiguous()
    out = _new(*ids.shape, table.size(1), device=table.device)
    n, d = ids.numel(), table.size(1)
    launch('ftmi_embedding', f'embedding[n={n},d={d}]', 0, n * 8 + 2 * n * d * 4,
           ids.data_ptr(), n, table.data_ptr(), table.size(0), d, out.data_ptr(), _ptr(err),
           _stream())
    return out


def split_weights(w: torch.Tensor) -> torch.Tensor:
    """fp32 [N][K] -> bf16 [3][N][roundup(K, 32)] pieces (w = p0 + p1 + p2 exactly), the
    pre-split operand of the bf16x6 GEMM path (`ftmi_split_weights`)."""
    _dev(w)
    if w.dim() != 2 or w.dtype != _f32 or not w.is_contiguous():
        raise ValueError('split_weights: contiguous fp32 [N][K] expected')
    N, K = w.shape
    Kp = (K + 31) // 32 * 32
    out = torch.empty(3, N, Kp, device=w.device, dtype=torch.bfloat16)
    launch('ftmi_split_weights', f'split_weights[N={N},K={K}]', 0, 4.0 * N * K + 6.0 * N * Kp,
           w.data_ptr(), N, K, out.data_ptr(), _stream())
    return out


def split_weights_f16(w: torch.Tensor, frag: bool = False) -> torch.Tensor:
    """fp32 [N][K] -> the f16x3 operand of `ftmi_split_weights_f16` (uint8 bytes: f16 planes
    [3][N][roundup(K, 32)] = (2^11 h, t, h) of the power-of-two column-scaled rows, then
    float colscale[N]).  frag: the planes in the fragment-major order of
    `ftmi_split_weights_f16_frag` (the operand of `highway_stack`)."""
    _dev(w)
    if w.dim() != 2 or w.dtype != _f32 or not w.is_contiguous():
        raise ValueError('split_weights_f16: contiguous fp32 [N][K] expected')
    N, K = w.shape
    nbytes = int(_lib.load().ftmi_split_weights_f16_bytes(N, K))
    out = torch.empty(nbytes, device=w.device, dtype=torch.uint8)
    name = 'ftmi_split_weights_f16_frag' if frag else 'ftmi_split_weights_f16'
    launch(name, f'split_weights_f16[N={N},K={K}{",frag" if frag else ""}]', 0,
           4.0 * N * K + nbytes, w.data_ptr(), N, K, out.data_ptr(), _stream())
    return out


def presplit_for(w: torch.Tensor, mma: Optional[int] = None) -> Optional[torch.Tensor]:
    """The pre-split operand of a packed weight for the matrix path `mma` (default MMA):
    f16 planes (2), bf16 pieces (1), None (0)."""
    m = MMA if mma is None else mma
    if m == 2:
        return split_weights_f16(w)
    return split_weights(w) if m == 1 else None


def split_bank_weights(w: torch.Tensor, K: int, Cin: int, Cout: int,
                       mma: Optional[int] = None) -> Optional[torch.Tensor]:
    """Pre-split blocks of a packed conv bank: group g's `presplit_for` block of the
    [Cout][(g+1) Cin] weight, back to back (the `w_split` layout of `ftmi_conv_bank`)."""
    parts, off = [], 0
    for g in range(K):
        n = Cout * Cin * (g + 1)
        blk = presplit_for(w[off:off + n].view(Cout, (g + 1) * Cin), mma)
        if blk is None:
            return None
        parts.append(blk.reshape(-1).view(torch.uint8))
        off += n
    return torch.cat(parts)


def conv1d(x: torch.Tensor, w: torch.Tensor, k: int, pad: int, *, bias=None, relu=False,
           bn=None, maxpool=False, residual=None, out=None, out_t=None, want_y=True,
           T_out: int = 0, mma: Optional[int] = None, w_split: Optional[torch.Tensor] = None,
           x_split: bool = False):
    """Fused Conv1d (+bias, ReLU, BN, residual) on a channels-last (B, T, Cin) view.

    w: packed [N][k*Cin].  Returns (y, yt) where y is (B, T_out, N) (or `out`) and yt is
    the optional (B, N, T_out) transposed copy (`out_t`).  w_split: optional
    `split_weights(w)` (bf16x6 path without the per-call weight split).  x_split: x holds
    f16x3 split rows (include/ftmi.h, e.g. conv_bank(split_out=True)); f16x3 slab kernel
    only (the C side refuses other shapes with FTMI_E_UNSUPPORTED).
    """
    _dev(x, w, bias, residual, out, out_t, w_split)
    B, T, Cin, xs = _rows(x)
    N = w.size(0)
    To = T_out or T
    if w.size(1) != k * Cin:
        raise ValueError(f'packed weight {tuple(w.shape)} does not match k={k}, Cin={Cin}')
    y = None
    if want_y:
        y = out if out is not None else _new(B, To, N, device=x.device)
        _rows(y)
    if residual is not None:
        _rows(residual)
    a = ConvArgs()
    a.x, a.x_stride, a.B, a.T, a.Cin = x.data_ptr(), xs, B, T, Cin
    a.w, a.N, a.k, a.pad = w.data_ptr(), N, k, pad
    a.bias = _ptr(bias)
    a.relu = int(relu)
    if bn is not None:
        a.bn_scale, a.bn_shift = bn[0].data_ptr(), bn[1].data_ptr()
    a.maxpool = int(maxpool)
    if residual is not None:
        a.residual, a.res_stride = residual.data_ptr(), residual.stride(1)
    if y is not None:
        a.y, a.y_stride = y.data_ptr(), y.stride(1)
    a.yt = _ptr(out_t)
    a.T_out = To
    a.mma, a.w_split = _gemm_mma(mma, w_split)
    a.status = status_word(x.device).data_ptr()
    a.x_split = int(x_split)
    M = B * To
    r = _route('ftmi_conv1d_route', ctypes.byref(a))
    if r.kernel in _lib.ROUTE_SKINNIES:  # the split is the kernel's, not a tuning choice
        sk, ws = r.split_k, r.ws_floats
    else:
        sk = _split_k(M, N, k * Cin, a.mma, r.kernel in _lib.ROUTE_SLABS, Cin)
        ws = sk * M * N
    if sk > 1:
        part = _new(ws, device=x.device)
        a.split_k, a.split_ws = sk, part.data_ptr()
    label = (f'conv1d[M={M},N={N},K={k * Cin}{",maxpool" if maxpool else ""}'
             f'{",xsplit" if x_split else ""},mma={a.mma}]')
    launch('ftmi_conv1d', label, 2.0 * M * N * k * Cin,
           4.0 * (B * T * Cin + N * k * Cin + M * N * (1 + (residual is not None))),
           ctypes.byref(a), _stream())
    return y, out_t


POOL_BANK = os.environ.get('FTMI_POOL_BANK', '1') != '0'
# the pooled bank hands proj1 its operand as f16x3 split rows (split once, not per column
# tile of proj1: c3 proj1 -2..3 %; a round-3 shell A/B loop, since replaced by tools/ab_bench.py); FTMI_SPLIT_ROWS=0: fp32 rows
SPLIT_ROWS = os.environ.get('FTMI_SPLIT_ROWS', '1') != '0'
# FTMI_SPLIT_BANK_IN=1: the bank also takes its own input split once (split_rows) instead of
# per group / column tile — measured neutral at c3 (the bank kernel saved what the extra
# split launch cost; a round-3 shell A/B loop, since replaced by tools/ab_bench.py), so off by default
SPLIT_BANK_IN = os.environ.get('FTMI_SPLIT_BANK_IN', '0') == '1'


def bank_pools(x: torch.Tensor, K: int, Cout: int, mma: Optional[int] = None, w_split=None) -> bool:
    """Whether conv_bank(pool=True) applies: the library routes the pooled bank of x (its
    address and row stride; the output and the BN vectors as conv_bank allocates them,
    16-byte aligned and dense) to a kernel that stores the CBHG maxpool itself, where the
    few-row bank takes the skinny or halves kernel instead."""
    if not POOL_BANK:
        return False
    m, wsp = _gemm_mma(mma, w_split)
    B, T, Cin = x.size(0), x.size(1), x.size(2)
    at = dict(x=x.data_ptr(), xs=x.stride(-2), wsp=wsp)
    return (_bank_route(m, B, T, Cin, K, Cout, **at).kernel in _lib.ROUTE_SLABS
            and bool(_bank_route(m, B, T, Cin, K, Cout, flags=BANK_POOL, **at).pooled))


def bank_halves_image(w_split: Optional[torch.Tensor], K: int, Cin: int,
                      Cout: int) -> Optional[torch.Tensor]:
    """The stream-order weight image of the one-launch few-row bank
    (`ftmi_conv_bank_halves_image`: every wave's weight fragments in its load order, one
    contiguous 1 KB run per wave load), built once per weights version from the f16x3 split
    blocks `split_bank_weights` made; None when those are not f16 planes or the shape has no
    halves kernel.  FTMI_BANK_IMAGE=0 (read when the weights are packed) keeps the planes."""
    if (w_split is None or w_split.dtype != torch.uint8 or not w_split.is_cuda
            or os.environ.get('FTMI_BANK_IMAGE', '1') == '0'):
        return None
    lib = _lib.load()
    n = int(lib.ftmi_conv_bank_halves_image_bytes(Cin, K, Cout))
    if n <= 0:
        return None
    img = torch.empty(n, device=w_split.device, dtype=torch.uint8)
    launch('ftmi_conv_bank_halves_image', f'bank_halves_image[K={K},Cin={Cin},Cout={Cout}]', 0,
           2.0 * n, w_split.data_ptr(), Cin, K, Cout, img.data_ptr(), _stream())
    return img


def conv_bank(x: torch.Tensor, w: torch.Tensor, K: int, Cout: int, scale: torch.Tensor,
              shift: torch.Tensor, mma: Optional[int] = None,
              w_split: Optional[torch.Tensor] = None, pool: bool = False,
              split_out: bool = False, x_split: bool = False,
              w_image: Optional[torch.Tensor] = None) -> torch.Tensor:
    """CBHG conv bank, (B, T, Cin) -> (B, T, K*Cout); pool: the maxpool(2, 1) of it
    (common_layers.py:73,100), stored by the bank kernel (see bank_pools); split_out (with
    pool): stored as f16x3 split rows for proj1 (conv1d(x_split=True)); x_split: x holds
    split rows (split_rows); w_image: `bank_halves_image(w_split, ...)`, read instead of
    w_split where the one-launch few-row kernel runs (same results bit for bit)."""
    if split_out and not pool:
        raise ValueError('split_out needs pool')
    _dev(x, w, scale, shift, w_split)
    B, T, Cin, xs = _rows(x)
    y = torch.empty(B, T, K * Cout, device=x.device, dtype=_f32)
    M = B * T
    flops = 2.0 * M * Cout * Cin * K * (K + 1) / 2
    mma, wsp = _gemm_mma(mma, w_split)
    flags = int(pool) | (BANK_Y_SPLIT * int(split_out)) | (BANK_X_SPLIT * int(x_split))
    r = _bank_route(mma, B, T, Cin, K, Cout, x=x.data_ptr(), xs=xs, w=w.data_ptr(), wsp=wsp,
                    scale=scale.data_ptr(), shift=shift.data_ptr(), y=y.data_ptr(),
                    ys=y.stride(-2), flags=flags)
    sk, part = r.split_k, None
    if r.kernel == _lib.ROUTE_BANK_HALVES:
        # the few-row bank in one launch (gemm.hip conv_bank_halves_kernel)
        part, flags = _stream_workspace('bank', r.ws_floats, x.device, _f32), BANK_HALVES
        if w_image is not None:
            _dev(w_image)
            wsp, flags = w_image.data_ptr(), BANK_HALVES | BANK_IMAGE
    elif sk > 1:  # weight-streaming kernel: partial sums, finished in order
        part = torch.empty(r.ws_floats, device=x.device, dtype=_f32)
    launch('ftmi_conv_bank_split', f'conv_bank[M={M},K={K},Cin={Cin},mma={mma}'
           f'{",pool" if pool else ""}{",split" if split_out else ""}{",xsplit" if x_split else ""}'
           ']',
           flops, 4.0 * (M * Cin + Cout * Cin * K * (K + 1) / 2 + M * K * Cout),
           x.data_ptr(), xs, B, T, Cin, w.data_ptr(), wsp, K, Cout,
           scale.data_ptr(), shift.data_ptr(), y.data_ptr(), y.stride(-2), mma,
           status_word(x.device).data_ptr(), sk, _ptr(part), flags, _stream())
    return y


BANK_COUNTERS = 4096  # include/ftmi.h FTMI_BANK_COUNTERS
# include/ftmi.h FTMI_BANK_*
BANK_POOL, BANK_Y_SPLIT, BANK_X_SPLIT, BANK_HALVES, BANK_IMAGE = 1, 2, 4, 16, 32
_FAKE = 1 << 12  # a 16-byte aligned stand-in for an address a route query never reads


def _bank_route(mma: int, B: int, T: int, Cin: int, K: int, Cout: int, *, x=_FAKE, xs=None,
                w=_FAKE, wsp=_FAKE, scale=_FAKE, shift=_FAKE, y=_FAKE, ys=None,
                flags: int = 0) -> _lib.GemmRoute:
    """ftmi_conv_bank_route of a bank; operands not given count as dense and aligned."""
    return _route('ftmi_conv_bank_route', x, Cin if xs is None else xs, B, T, Cin, w, wsp, K, Cout,
                  scale, shift, y, K * Cout if ys is None else ys, mma, None, flags)


def _bank_halves(mma: int, B: int, T: int, Cin: int, K: int, Cout: int) -> bool:
    """Whether conv_bank takes the one-launch channel-halves kernel (FTMI_ROUTE_BANK_HALVES:
    batch-1 generation, BASELINE config c2) for a dense, aligned bank of this shape."""
    return _bank_route(mma, B, T, Cin, K, Cout).kernel == _lib.ROUTE_BANK_HALVES


_STREAM_WS = {}      # (kind, device, stream handle) -> that stream's workspace of the kind
_STREAM_WS_OLD = []  # superseded ones: queued work or a captured graph may still use them


def _stream_workspace(kind: str, n: int, device, dtype=torch.uint8) -> torch.Tensor:
    """The current stream's zeroed workspace of a kind, at least n elements of dtype.  One per
    (kind, device, stream) — launches on one stream are ordered, so they may share it — kept
    alive for graph replays that captured its address; grown (a new zeroed buffer, the old
    one retired to _STREAM_WS_OLD) when too small.  The kinds:
    'bank'    FTMI_BANK_HALVES: BANK_COUNTERS fp32 counters (zero once; every launch leaves
              them zero) followed by the partial sums;
    'spread'  the spread CBHG tail's exchange bytes;
    'kv'      the attention K / V planes (ftmi_panel_proj_qkv / ftmi_attention_kv), shared by
              the layers on a stream.  The planes' pad keys T..Tp-1 are never written; the
              attention kernels zero them while staging (a stale value there, even an inf
              left by an overflowing call that reran on the exact path, never reaches the
              output)."""
    key = (kind, torch.device(device), torch.cuda.current_stream(device).cuda_stream)
    t = _STREAM_WS.get(key)
    if t is None or t.numel() < n:
        if t is not None:
            _STREAM_WS_OLD.append(t)
        t = _STREAM_WS[key] = torch.zeros(n, device=device, dtype=dtype)
    return t


def split_rows(x: torch.Tensor) -> torch.Tensor:
    """(B, T, C) fp32 rows -> the same-size buffer holding them as f16x3 split rows (per row C
    f16 heads then C scaled tails, include/ftmi.h), range-checked into the status word."""
    _dev(x)
    B, T, C, xs = _rows(x)
    y = torch.empty(B, T, C, device=x.device, dtype=_f32)
    launch('ftmi_split_rows', f'split_rows[M={B * T},C={C}]', 0.0, 8.0 * B * T * C,
           x.data_ptr(), xs, B * T, C, y.data_ptr(), y.stride(1),
           status_word(x.device).data_ptr(), _stream())
    return y


# A conv bank whose input is an embedding runs as a table gather (embed_bank) from this many
# (b, t) rows on; below it the GEMM bank (conv_bank) takes the embedded rows.  Interleaved
# A/B (tools/ab_bench.py, DESIGN.md §4 `embed_bank_kernel`): c3 (12,800 rows) 7.85-7.94 ->
# 7.56-7.77 ms/step; c2 (120 rows) 2.60-2.68 with the table bank against 2.59-2.62 without —
# inside the spread, so the few-row GEMM bank stays.
EMBED_BANK_MIN_ROWS = 256
EMBED_BANK_TILE = (16, 64)  # embed_bank.hip EB_ROWS, EB_ROWS * EB_WAVES: rows per wave / workgroup
EMBED_BANK_KMAX, EMBED_BANK_PANEL = 16, 256  # embed_bank.hip EB_KMAX, EB_PANEL


def embed_bank_taps(kmin: int, kmax: int) -> int:
    """Rows per symbol of an embed_bank table: one per (kernel size, tap)."""
    return (kmax * (kmax + 1) - kmin * (kmin - 1)) // 2


def embed_bank_table(emb: torch.Tensor, conv_weights) -> torch.Tensor:
    """The table of `embed_bank` for an embedding weight (S, Cin) and nn.Conv1d weights
    (Cout, Cin, k) of consecutive kernel sizes: [S][taps][Cout] fp32 with
    Tab[s][(k, j)] = W_k[:, :, j] . E[s], taps ordered (k ascending, j = 0..k-1) — computed
    in fp64 and rounded once.  Pack-time work (a torch einsum), once per weights version."""
    _dev(emb, *conv_weights)
    e = emb.detach().double()
    parts = [torch.einsum('ncj,sc->sjn', w.detach().double(), e) for w in conv_weights]
    return torch.cat(parts, 1).float().contiguous()


def embed_bank_ok(num_rows: int, kmin: int, kmax: int, Cout: int) -> bool:
    """Whether ftmi_embed_bank has a kernel for the shape (embed_bank.hip: kernel sizes up to
    16, Cout a multiple of 256, a table below 2 GiB); elsewhere it returns
    FTMI_E_UNSUPPORTED and the caller keeps the GEMM bank."""
    return (1 <= kmin <= kmax <= EMBED_BANK_KMAX and Cout > 0 and Cout % EMBED_BANK_PANEL == 0
            and num_rows * embed_bank_taps(kmin, kmax) * Cout * 4 < 1 << 31)


def embed_bank(ids: torch.Tensor, table: torch.Tensor, kmin: int, kmax: int, Cout: int,
               scale: torch.Tensor, shift: torch.Tensor, pool: bool = False,
               split_out: bool = False) -> torch.Tensor:
    """Conv bank (kernel sizes kmin..kmax, pad k//2, ReLU then folded BN) of the embedded ids
    as a gather of `embed_bank_table` rows summed in tap order: (B, T) int64 ->
    (B, T, G*Cout), G = kmax - kmin + 1.  pool: the CBHG maxpool(2, 1) of it; split_out: stored
    as f16x3 split rows (range-checked into the status word).  An id outside the table
    contributes zero rows, like `embedding`'s zero row."""
    _dev(ids, table, scale, shift)
    ids = ids.contiguous()
    if ids.dtype != torch.int64:
        ids = ids.long()
    B, T = ids.shape
    G, taps = kmax - kmin + 1, embed_bank_taps(kmin, kmax)
    if table.dim() != 3 or table.size(1) != taps or table.size(2) != Cout or table.dtype != _f32 \
            or not table.is_contiguous():
        raise ValueError(f'embed_bank: table {tuple(table.shape)} is not contiguous fp32 '
                         f'[S][{taps}][{Cout}]')
    if scale.numel() != G * Cout or shift.numel() != G * Cout:
        raise ValueError('embed_bank: scale / shift must hold G*Cout values')
    y = torch.empty(B, T, G * Cout, device=table.device, dtype=_f32)
    M = B * T
    launch('ftmi_embed_bank', f'embed_bank[M={M},{f"K={kmax}" if kmin == 1 else f"k={kmin}-{kmax}"},'
           f'Cout={Cout}{",pool" if pool else ""}{",split" if split_out else ""}]',
           1.0 * M * taps * Cout, 4.0 * M * taps * Cout + 8.0 * M + 4.0 * M * G * Cout,
           ids.data_ptr(), B, T, table.data_ptr(), table.size(0), kmin, kmax, Cout,
           scale.data_ptr(), shift.data_ptr(), y.data_ptr(), y.stride(-2),
           int(pool) | (2 * int(split_out)), status_word(table.device).data_ptr(), _stream())
    return y


def highway(x: torch.Tensor, w12: torch.Tensor, b1: torch.Tensor, b2: torch.Tensor,
            out: Optional[torch.Tensor] = None, mma: Optional[int] = None,
            w_split: Optional[torch.Tensor] = None) -> torch.Tensor:
    _dev(x, w12, b1, b2, out, w_split)
    B, T, C, xs = _rows(x)
    y = out if out is not None else torch.empty(B, T, C, device=x.device, dtype=_f32)
    M = B * T
    mma, wsp = _gemm_mma(mma, w_split)
    at = (x.data_ptr(), xs, M, C, w12.data_ptr(), wsp, b1.data_ptr(), b2.data_ptr(), y.data_ptr(),
          y.stride(1), mma, status_word(x.device).data_ptr())
    r = _route('ftmi_highway_route', *at)
    sk, part = r.split_k, None
    if sk:  # weight-streaming kernel: partials + the highway finish
        part = torch.empty(r.ws_floats, device=x.device, dtype=_f32)
    launch('ftmi_highway_split', f'highway[M={M},C={C},mma={mma}]', 2.0 * M * 2 * C * C,
           4.0 * (2 * M * C + 2 * C * C), *at, sk, _ptr(part), _stream())
    return y


HS_C, HS_NPASS, HS_MAXL = 256, 512, 8  # highway_stack.hip highway_stack_kernel shape limits
# The fused stack below FTMI_HS_MIN rows falls back to the per-layer launches.  Round 4
# moved the default 256 -> 64: at c2 (the prenet's 120 rows) the one launch replaces four
# skinny GEMMs + four finish launches, c2 2.81 / 2.96 / 2.83 -> 2.80 / 2.81 / 2.80 ms per
# step (tools/ab_bench.py, 3 interleaved rounds, profiles/r4_ab_c2_env.jsonl)
HS_MIN_ROWS = int(os.environ.get('FTMI_HS_MIN', 64))


def highway_stack_ok(M: int, Cp: int, C: int, L: int, n_out: int, splits) -> bool:
    """Whether `highway_stack` applies: the f16x3 path is the one in force (not inside
    exact_paths()), every weight has its f16 planes, and the shapes fit the kernel."""
    if os.environ.get('FTMI_HS', '1') == '0' or (_FORCED and _FORCED[-1][0] != 2):
        return False
    if not _FORCED and MMA != 2:
        return False
    return (C == HS_C and 0 < Cp <= C and Cp % 4 == 0 and L <= HS_MAXL
            and n_out % HS_NPASS == 0 and M >= max(HS_MIN_ROWS, 1)
            and all(w is not None and w.dtype == torch.uint8 for w in splits))


def highway_stack(x: torch.Tensor, pre_split: torch.Tensor, C: int, hw_splits, b1s, b2s,
                  out_split: Optional[torch.Tensor], b_out: Optional[torch.Tensor], n_out: int,
                  want_h: bool = False, spread: bool = True):
    """CBHG pre_highway -> highways -> GRU input projection in one launch
    (`ftmi_highway_stack`; models/common_layers.py:110-115).  x: (B, T, Cp) channels-last;
    every weight block is `split_weights_f16(w, frag=True)`.  spread=False keeps the
    one-workgroup-per-64-rows kernel where the spread one would apply (its workgroups must
    be co-resident: the caller decides).  Returns (y (B, T, n_out) or None, h (B, T, C) or
    None)."""
    _dev(x, pre_split, out_split, b_out, *hw_splits, *b1s, *b2s)
    B, T, Cp, xs = _rows(x)
    M = B * T
    L = len(hw_splits)
    y = torch.empty(B, T, n_out, device=x.device, dtype=_f32) if out_split is not None else None
    h = torch.empty(B, T, C, device=x.device, dtype=_f32) if want_h else None
    arr = ctypes.c_void_p * max(L, 1)
    w_arr = arr(*[w.data_ptr() for w in hw_splits])
    b1_arr = arr(*[b.data_ptr() for b in b1s])
    b2_arr = arr(*[b.data_ptr() for b in b2s])
    flops = 2.0 * M * C * (Cp + L * 2 * C + n_out)
    nbytes = 4.0 * M * (Cp + n_out + (C if want_h else 0))
    args = (x.data_ptr(), xs, M, Cp, C, pre_split.data_ptr(), L, ctypes.addressof(w_arr),
            ctypes.addressof(b1_arr), ctypes.addressof(b2_arr), _ptr(out_split), _ptr(b_out),
            n_out if out_split is not None else 0, _ptr(y), y.stride(1) if y is not None else 0,
            _ptr(h), h.stride(1) if h is not None else 0, status_word(x.device).data_ptr())
    if spread and hs_spread_blocks(M, n_out if out_split is not None else 0) > 0:
        nws = int(_lib.load().ftmi_highway_stack_spread_ws_bytes(M))
        ws = _stream_workspace('spread', max(nws, 16), x.device)
        launch('ftmi_highway_stack_spread', f'highway_stack_spread[M={M},Cp={Cp},L={L},N={n_out}]',
               flops, nbytes, *args, ws.data_ptr(), _stream())
    else:
        launch('ftmi_highway_stack', f'highway_stack[M={M},Cp={Cp},L={L},N={n_out}]', flops,
               nbytes, *args, _stream())
    return y, h


def hs_spread_blocks(M: int, n_out: int = 0) -> int:
    """Workgroups of the spread CBHG tail (`ftmi_highway_stack_spread`) for M rows, or 0 when
    `highway_stack` runs the one-workgroup-per-64-rows kernel: M <= 1024 rows, n_out <= 1536,
    all of them resident at once.  FTMI_HS_SPREAD=0 (read per call) keeps that kernel."""
    if os.environ.get('FTMI_HS_SPREAD', '1') == '0' or n_out > 1536:
        return 0
    n = int(_lib.load().ftmi_highway_stack_spread_blocks(M))
    return n if 0 < n <= _num_cus() else 0


PANEL_N = 256  # highway_stack.hip panel_proj_kernel: output columns per panel (LayerNorm width)


def panel_ok(K: int, N: int, ln: bool, split) -> bool:
    """Whether `panel_proj` applies: the f16x3 path is in force (not inside exact_paths()),
    the weight has its fragment-major f16 planes, and the shape fits the kernel
    (FTMI_PANEL=0 keeps the slab GEMM + LayerNorm launches)."""
    if os.environ.get('FTMI_PANEL', '1') == '0' or (_FORCED and _FORCED[-1][0] != 2):
        return False
    if not _FORCED and MMA != 2:
        return False
    return (split is not None and split.dtype == torch.uint8 and K % 4 == 0
            and N % PANEL_N == 0 and (N == PANEL_N or not ln))


def panel_proj(x: torch.Tensor, w_frag: torch.Tensor, N: int, bias: Optional[torch.Tensor] = None,
               residual: Optional[torch.Tensor] = None, ln=None,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = [LayerNorm](x W^T + bias [+ residual]) in one launch (`ftmi_panel_proj`): the k = 1
    projections of a FastPitch FFT block (models/fast_pitch.py:56-91) with their residual
    add and norm.  x: (B, T, K) channels-last; w_frag: split_weights_f16(W, frag=True);
    ln: (gamma, beta, eps) or None.  out may be the residual (in place), never x."""
    _dev(x, w_frag, bias, residual)
    B, T, K, xs = _rows(x)
    M = B * T
    y = out if out is not None else torch.empty(B, T, N, device=x.device, dtype=_f32)
    rs = 0
    if residual is not None:
        if tuple(residual.shape) != (B, T, N):
            raise ValueError(f'residual shape {tuple(residual.shape)} != {(B, T, N)}')
        rs = _rows(residual)[3]
    if tuple(y.shape) != (B, T, N):
        raise ValueError(f'out shape {tuple(y.shape)} != {(B, T, N)}')
    _rows(y)
    g, b, eps = ln if ln is not None else (None, None, 0.0)
    launch('ftmi_panel_proj', f'panel_proj[M={M},K={K},N={N}{",ln" if ln is not None else ""}]',
           2.0 * M * N * K, 4.0 * M * (K + N * (2 if residual is not None else 1)),
           x.data_ptr(), xs, M, K, w_frag.data_ptr(), N, _ptr(bias), _ptr(residual), rs,
           _ptr(g), _ptr(b), float(eps), y.data_ptr(), y.stride(1),
           status_word(x.device).data_ptr(), _stream())
    return y


def kv_fused_ok(T: int, d: int, heads: int, w_frag) -> bool:
    """Whether FastPitch's in_proj + attention take ftmi_panel_proj_qkv + ftmi_attention_kv
    (the split pass folded into the projection): f16x3 in force, the attention would
    presplit (T > 256), d = 256, head_dim 64 / 128.  FTMI_KV_FUSED=0 turns it off."""
    return (os.environ.get('FTMI_KV_FUSED', '1') != '0' and panel_ok(d, 3 * d, False, w_frag)
            and ATTN_PRESPLIT and T > 256 and d == PANEL_N and d % heads == 0
            and d // heads in (64, 128))


def panel_proj_qkv(x: torch.Tensor, w_frag: torch.Tensor, d: int, heads: int,
                   bias: Optional[torch.Tensor] = None):
    """in_proj with the attention's K / V split folded in (`ftmi_panel_proj_qkv`): returns
    (q rows (B, T, d), the K / V plane workspace) for attention_kv."""
    _dev(x, w_frag, bias)
    B, T, K, xs = _rows(x)
    q = torch.empty(B, T, d, device=x.device, dtype=_f32)
    nws = int(_lib.load().ftmi_attention_workspace_bytes(B, T, heads, d // heads))
    ws = _stream_workspace('kv', nws, x.device)
    launch('ftmi_panel_proj_qkv', f'panel_proj[M={B * T},K={K},N={3 * d},qkv]',
           2.0 * B * T * 3 * d * K, 4.0 * B * T * (K + d) + 2.0 * nws / 4 * 2,
           x.data_ptr(), xs, B, T, K, w_frag.data_ptr(), d, _ptr(bias), heads, q.data_ptr(),
           q.stride(1), ws.data_ptr(), nws, status_word(x.device).data_ptr(), _stream())
    return q, ws


def attention_kv(q: torch.Tensor, ws: torch.Tensor, heads: int,
                 key_padding_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """attention on Q rows with K / V from panel_proj_qkv's workspace (`ftmi_attention_kv`)."""
    _dev(q, ws, key_padding_mask)
    B, T, d, rs = _rows(q)
    hd = d // heads
    out = torch.empty(B, T, d, device=q.device, dtype=_f32)
    kpm = None
    if key_padding_mask is not None:
        kpm = key_padding_mask.to(torch.uint8).contiguous()
    launch('ftmi_attention_kv', f'attention[B={B},T={T},H={heads},hd={hd},mma=2,kv]',
           4.0 * B * heads * T * T * hd, 4.0 * (B * T * d * 2),
           q.data_ptr(), rs, B, T, heads, hd, _ptr(kpm), float(np.float32(np.sqrt(1.0 / hd))),
           out.data_ptr(), out.stride(1), status_word(q.device).data_ptr(), ws.data_ptr(),
           ws.numel(), _stream())
    return out


RNN_SPREAD = 0x100  # include/ftmi.h FTMI_RNN_SPREAD


def rnn_blocks(cell: int, B: int, H: int, mma: Optional[int] = None) -> int:
    """Persistent workgroups one ftmi_rnn_bidir launch occupies (ftmi_rnn_blocks)."""
    m = _rnn_mma() if mma is None else mma
    return int(_lib.load().ftmi_rnn_blocks(cell, B, H, m))


def rnn_bidir(cell: int, xp: torch.Tensor, H: int, w_hh: torch.Tensor, b_hh: Optional[torch.Tensor],
              T: Optional[int] = None, index: Optional[torch.Tensor] = None,
              xp_zero: Optional[torch.Tensor] = None, lengths: Optional[torch.Tensor] = None,
              pad_value: float = 0.0, check: bool = False,
              ws: Optional[torch.Tensor] = None, mma: Optional[int] = None,
              spread: bool = False) -> torch.Tensor:
    """Bidirectional GRU (cell=0) / LSTM (cell=1) recurrence -> (B, T, 2H).

    xp: (B, T_src, 2*G*H) input projections; index: (B, T) int32 frame -> row map.
    check=True synchronises and raises RnnTimeout if a workgroup gave up waiting.
    mma: matrix path of W_hh h (default RNN_MMA; exact_paths() forces fp32).
    spread: FTMI_RNN_SPREAD — the recurrence may occupy every CU (fewer sequences per
    workgroup group, lower step latency); only for a recurrence that runs alone (the
    decoder LSTM, the postnet GRU), never beside other persistent recurrences.
    """
    mma = (_rnn_mma() if mma is None or _FORCED else mma)
    if lengths is not None:  # host-side lengths (as pack_padded_sequence takes) are fine
        lengths = lengths.to(device=xp.device, dtype=torch.int32).contiguous()
    _dev(xp, w_hh, b_hh, index, xp_zero, lengths)
    B, T_src, _, xs = _rows(xp)
    T = T if T is not None else T_src
    y = _new(B, T, 2 * H, device=xp.device)
    lib = _lib.load()
    need = int(lib.ftmi_rnn_workspace_bytes(B, H, cell)) // 4 + 4
    if ws is None or ws.numel() < need:
        ws = _new(need, device=xp.device, dtype=torch.int32)
    if index is not None:
        assert index.dtype == torch.int32 and index.is_contiguous() and index.shape == (B, T)
    G = 4 if cell else 3
    label = f'rnn_bidir[{"lstm" if cell else "gru"},B={B},T={T},H={H},mma={mma}]'
    # recurrent contraction W_hh h per step and direction; bytes: xp rows read per frame,
    # W_hh once, y written once
    launch('ftmi_rnn_bidir', label, 2.0 * B * T * 2 * G * H * H,
           4.0 * (B * T * 2 * G * H + 2 * G * H * H + B * T * 2 * H),
           cell, B, T, H, xp.data_ptr(), xs, T_src, _ptr(index), _ptr(xp_zero),
           w_hh.data_ptr(), _ptr(b_hh), _ptr(lengths), float(pad_value), y.data_ptr(), y.stride(1),
           int(mma) | (RNN_SPREAD if spread and not _COMPACT else 0), status_word(xp.device).data_ptr(),
           ws.data_ptr(), _stream())
    if check:
        torch.cuda.current_stream().synchronize()
        off = int(lib.ftmi_rnn_error_offset(B)) // 4
        if int(ws[off].item()) != 0:
            raise RnnTimeout('ftmi_rnn_bidir: a workgroup timed out waiting for its group')
    return y


def duration_counts(dur: torch.Tensor, apply_fill: bool, fill_value: float = 2.0):
    """In place: fill-2 rule (optional) + clip; returns (offsets (B,T+1), totals (B,), fill_flag)."""
    _dev(dur)
    if dur.dtype != _f32 or not dur.is_contiguous() or dur.dim() != 2:
        raise ValueError('dur must be a contiguous (B, T) fp32 tensor')
    B, T = dur.shape
    offsets = torch.empty(B, T + 1, device=dur.device, dtype=torch.int32)
    totals = torch.empty(B, device=dur.device, dtype=torch.int32)
    flag = torch.empty(1, device=dur.device, dtype=torch.int32)
    launch('ftmi_duration_counts', f'duration_counts[B={B},T={T}]', 0, B * T * 12,
           dur.data_ptr(), B, T, int(apply_fill), float(fill_value),
           offsets.data_ptr(), totals.data_ptr(), flag.data_ptr(), _stream())
    return offsets, totals, flag


def duration_trunc_sum(dur: torch.Tensor) -> torch.Tensor:
    """sum_{b,t} int64(trunc(dur)) as a device int64[1] (the fill-2 rule's statistic)."""
    _dev(dur)
    if dur.dtype != _f32 or not dur.is_contiguous() or dur.dim() != 2:
        raise ValueError('dur must be a contiguous (B, T) fp32 tensor')
    B, T = dur.shape
    out = torch.empty(1, device=dur.device, dtype=torch.int64)
    launch('ftmi_duration_trunc_sum', f'duration_trunc_sum[B={B},T={T}]', 0, 4.0 * B * T,
           dur.data_ptr(), B, T, out.data_ptr(), _stream())
    return out


def duration_counts_global(dur: torch.Tensor, global_sum: torch.Tensor, fill_value: float = 2.0):
    """duration_counts with the fill-2 decision taken on a batch-global sum (device int64[1])."""
    _dev(dur, global_sum)
    if dur.dtype != _f32 or not dur.is_contiguous() or dur.dim() != 2:
        raise ValueError('dur must be a contiguous (B, T) fp32 tensor')
    B, T = dur.shape
    offsets = torch.empty(B, T + 1, device=dur.device, dtype=torch.int32)
    totals = torch.empty(B, device=dur.device, dtype=torch.int32)
    flag = torch.empty(1, device=dur.device, dtype=torch.int32)
    launch('ftmi_duration_counts_global', f'duration_counts[B={B},T={T}]', 0, B * T * 12,
           dur.data_ptr(), B, T, global_sum.data_ptr(), float(fill_value), offsets.data_ptr(),
           totals.data_ptr(), flag.data_ptr(), _stream())
    return offsets, totals, flag


def _lens(lengths: torch.Tensor, B: int, device) -> torch.Tensor:
    """Per-item lengths as the kernels take them: device int32 [B], contiguous."""
    if lengths.numel() != B:
        raise ValueError(f'lengths holds {lengths.numel()} values for a batch of {B}')
    return lengths.to(device=device, dtype=torch.int32).contiguous()


def duration_counts_rows(dur: torch.Tensor, x_len: torch.Tensor, apply_fill: bool = True,
                         fill_value: float = 2.0):
    """duration_counts decided per item (x_len: (B,) valid positions of each row).  In place:
    duration 0 from x_len[b] on, the fill-2 rule on each row's own valid positions, the clip;
    returns (offsets (B, T+1), totals (B,), fill_flags (B,))."""
    _dev(dur, x_len)
    if dur.dtype != _f32 or not dur.is_contiguous() or dur.dim() != 2:
        raise ValueError('dur must be a contiguous (B, T) fp32 tensor')
    B, T = dur.shape
    x_len = _lens(x_len, B, dur.device)
    offsets = torch.empty(B, T + 1, device=dur.device, dtype=torch.int32)
    totals = torch.empty(B, device=dur.device, dtype=torch.int32)
    flags = torch.empty(B, device=dur.device, dtype=torch.int32)
    launch('ftmi_duration_counts_rows', f'duration_counts_rows[B={B},T={T}]', 0, B * T * 12,
           dur.data_ptr(), B, T, x_len.data_ptr(), int(apply_fill), float(fill_value),
           offsets.data_ptr(), totals.data_ptr(), flags.data_ptr(), _stream())
    return offsets, totals, flags


FILL_ROWS, FILL_TIME_LAST, FILL_SPLIT_ROWS = 0, 1, 2  # include/ftmi.h FTMI_FILL_*


def fill_tail(x: torch.Tensor, lengths: torch.Tensor, reach: int = -1, value: float = 0.0,
              time_last: bool = False, split: bool = False) -> torch.Tensor:
    """In place: `value` in rows [lengths[b], min(T, lengths[b] + reach)) of every item of a
    channels-last (B, T, C) view (reach < 0: the whole tail).  time_last: x is (B, C, T) with
    unit frame stride; split: the rows hold f16x3 split rows (conv_bank(split_out=True))."""
    _dev(x, lengths)
    if time_last:
        if split:
            raise ValueError('fill_tail: split rows are channels-last')
        # a single channel's stride is whatever the view says: the item stride counts
        stride = x.stride(1) if x.dim() == 3 and x.size(1) > 1 else x.stride(0)
        if (x.dim() != 3 or x.dtype != _f32 or x.stride(2) != 1
                or x.stride(0) != x.size(1) * stride):
            raise ValueError(f'fill_tail: expected a (B, C, T) fp32 view with unit frame stride '
                             f'and uniform channel stride, got shape {tuple(x.shape)} strides '
                             f'{x.stride()}')
        B, C, T = x.shape
        mode = FILL_TIME_LAST
    else:
        B, T, C, stride = _rows(x)
        mode = FILL_SPLIT_ROWS if split else FILL_ROWS
    lengths = _lens(lengths, B, x.device)
    n = T if reach < 0 else min(reach, T)
    launch('ftmi_fill_tail', f'fill_tail[B={B},T={T},C={C},reach={reach},mode={mode}]', 0,
           4.0 * B * n * C, x.data_ptr(), stride, B, T, C, lengths.data_ptr(), int(reach),
           float(value), mode, _stream())
    return x


def maxpool_rows(x: torch.Tensor, lengths: torch.Tensor) -> torch.Tensor:
    """The CBHG maxpool of (B, T, C) rows whose items end at lengths[b]: max(x[t-1], x[t])
    below it, zero rows from there on."""
    _dev(x, lengths)
    B, T, C, xs = _rows(x)
    lengths = _lens(lengths, B, x.device)
    y = torch.empty(B, T, C, device=x.device, dtype=_f32)
    launch('ftmi_maxpool_rows', f'maxpool_rows[M={B * T},C={C}]', 0, 8.0 * B * T * C,
           x.data_ptr(), xs, B, T, C, lengths.data_ptr(), y.data_ptr(), y.stride(1), _stream())
    return y


def lr_index(offsets: torch.Tensor, T_mel: int) -> torch.Tensor:
    _dev(offsets)
    B, T1 = offsets.shape
    index = torch.empty(B, T_mel, device=offsets.device, dtype=torch.int32)
    launch('ftmi_lr_index', f'lr_index[B={B},T_mel={T_mel}]', 0, 4.0 * B * (T1 + T_mel),
           offsets.data_ptr(), B, T1 - 1, T_mel, index.data_ptr(), _stream())
    return index


def length_regulate(x: torch.Tensor, index: torch.Tensor) -> torch.Tensor:
    _dev(x, index)
    B, T, C, xs = _rows(x)
    T_mel = index.size(1)
    y = torch.empty(B, T_mel, C, device=x.device, dtype=_f32)
    launch('ftmi_length_regulate', f'length_regulate[B={B},T={T},T_mel={T_mel},C={C}]', 0,
           4.0 * (B * T * C + B * T_mel * (C + 1)),
           x.data_ptr(), xs, B, T, C, index.data_ptr(), T_mel, y.data_ptr(), y.stride(1), _stream())
    return y


def series_proj_add(x: torch.Tensor, pitch: torch.Tensor, wp, bp, ps: float, energy: torch.Tensor,
                    we, be, es: float) -> torch.Tensor:
    """In place on x (B, T, C): x += proj(pitch)*ps ; x += proj(energy)*es."""
    _dev(x, pitch, energy, wp, bp, we, be)
    B, T, C, xs = _rows(x)
    pitch = pitch.reshape(B, T).to(_f32).contiguous()
    energy = energy.reshape(B, T).to(_f32).contiguous()
    launch('ftmi_series_proj_add', f'series_proj_add[B={B},T={T},C={C}]', 14.0 * B * T * C,
           4.0 * (2 * B * T * C + 2 * B * T + 8 * C),
           x.data_ptr(), xs, B, T, C, pitch.data_ptr(), wp.data_ptr(),
           bp.data_ptr(), float(ps), energy.data_ptr(), we.data_ptr(), be.data_ptr(), float(es),
           _stream())
    return x


def rowdot(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], alpha: float) -> torch.Tensor:
    """(x . w + bias) / alpha over the last dim: (B, T, C) -> (B, T)."""
    _dev(x, w, bias)
    B, T, C, xs = _rows(x)
    out = _new(B, T, device=x.device)
    launch('ftmi_rowdot', f'rowdot[M={B * T},C={C}]', 2.0 * B * T * C, 4.0 * (B * T * (C + 1) + C),
           x.data_ptr(), xs, B * T, C, w.data_ptr(), _ptr(bias), float(alpha),
           out.data_ptr(), _stream())
    return out


# --------------------------------------------------------------------------------------
# FastPitch transformer (csrc/transformer.hip)

def _check_pe(pe: torch.Tensor, rows: int, width: int, what: str) -> None:
    """The kernels read pe[t, :width] for t < rows as contiguous fp32 rows of that width."""
    if (pe.dim() != 2 or pe.dtype != _f32 or not pe.is_contiguous() or pe.size(1) != width
            or pe.size(0) < rows):
        raise ValueError(f'{what}: pe must be contiguous fp32 rows (>= {rows}, {width}), got '
                         f'{pe.dtype} shape {tuple(pe.shape)} strides {pe.stride()}')


def embedding_posenc(ids: torch.Tensor, table: torch.Tensor, pe: torch.Tensor,
                     scale: torch.Tensor) -> torch.Tensor:
    """(B, T) ids -> table[ids] + scale * pe[:T]  (B, T, dim)."""
    _dev(ids, table, pe, scale)
    B, T = ids.shape
    dim = table.size(1)
    _check_pe(pe, T, dim, 'embedding_posenc')
    ids = ids.contiguous().to(torch.int64)
    out = torch.empty(B, T, dim, device=ids.device, dtype=_f32)
    launch('ftmi_embedding_posenc', f'embedding_posenc[n={B * T},d={dim}]', B * T * dim * 2.0,
           8.0 * B * T + 12.0 * B * T * dim,
           ids.data_ptr(), B, T, table.data_ptr(), table.size(0), dim, pe.data_ptr(),
           scale.data_ptr(), out.data_ptr(), None, _stream())
    return out


def lr_posenc(x: torch.Tensor, index: torch.Tensor, pe: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """LengthRegulator expansion (index map) + scale * pe[:T_mel]: (B, T_mel, C)."""
    _dev(x, index, pe, scale)
    B, T, C, xs = _rows(x)
    T_mel = index.size(1)
    _check_pe(pe, T_mel, C, 'lr_posenc')
    y = torch.empty(B, T_mel, C, device=x.device, dtype=_f32)
    launch('ftmi_lr_posenc', f'lr_posenc[B={B},T_mel={T_mel},C={C}]', 2.0 * B * T_mel * C,
           4.0 * (B * T * C + B * T_mel * (2 * C + 1)),
           x.data_ptr(), xs, B, T, C, index.data_ptr(), T_mel, pe.data_ptr(), scale.data_ptr(),
           y.data_ptr(), y.stride(1), _stream())
    return y


def layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _dev(x, gamma, beta, out)
    B, T, C, xs = _rows(x)
    y = out if out is not None else torch.empty(B, T, C, device=x.device, dtype=_f32)
    launch('ftmi_layernorm', f'layernorm[M={B * T},C={C}]', 8.0 * B * T * C, 8.0 * B * T * C,
           x.data_ptr(), xs, B * T, C, gamma.data_ptr(), beta.data_ptr(), float(eps),
           y.data_ptr(), y.stride(1), _stream())
    return y


ATTN_PRESPLIT = os.environ.get('FTMI_ATTN_PRESPLIT', '1') != '0'


def attention(qkv: torch.Tensor, heads: int, key_padding_mask: Optional[torch.Tensor] = None,
              mma: Optional[int] = None, presplit: Optional[bool] = None) -> torch.Tensor:
    """Self-attention core of nn.MultiheadAttention on packed in_proj rows (B, T, 3d).
    mma: 2 = f16x3 contractions (default, MMA), 0 = fp32 MFMA (exact_paths(), MMA 0/1).
    presplit (f16x3; default: ATTN_PRESPLIT and T > 512): K and V split once into f16
    planes in a workspace instead of per query tile (identical results; measured at c5's
    postnet T = 1400: 825 -> 618 us incl. the split pass, slower at T = 200)."""
    _dev(qkv, key_padding_mask)
    m = _FORCED[-1][0] if _FORCED else (MMA if mma is None else mma)
    m = 2 if m == 2 else 0
    B, T, C3, rs = _rows(qkv)
    d = C3 // 3
    hd = d // heads
    out = torch.empty(B, T, d, device=qkv.device, dtype=_f32)
    kpm = None
    if key_padding_mask is not None:
        kpm = key_padding_mask.to(torch.uint8).contiguous()
    qscale = float(np.float32(np.sqrt(1.0 / hd)))
    ws, nws = None, 0
    if presplit is None:  # the transposed kernel with the split pass against its in-kernel
        # split (tools/attn_short_ab.py, B = 64, masked): T 300-400 0.91-0.95x, T 600 1.01x,
        # T 1000 1.01-1.06x, T 1400 1.02-1.08x
        presplit = ATTN_PRESPLIT and T > 512
    if m == 2 and presplit:
        nws = int(_lib.load().ftmi_attention_workspace_bytes(B, T, heads, hd))
        ws = torch.empty(nws, device=qkv.device, dtype=torch.uint8)
    launch('ftmi_attention', f'attention[B={B},T={T},H={heads},hd={hd},mma={m}]',
           4.0 * B * heads * T * T * hd, 4.0 * (B * T * C3 + B * T * d),
           qkv.data_ptr(), rs, B, T, heads, hd, 0, d, 2 * d, _ptr(kpm), qscale,
           out.data_ptr(), out.stride(1), m, status_word(qkv.device).data_ptr(), _ptr(ws), nws,
           _stream())
    return out


# ---- WaveRNN vocoder (csrc/wavernn.hip) --------------------------------------------------

def wr_stretch_conv(x: torch.Tensor, scale: int, w: torch.Tensor, W_out: Optional[int] = None,
                    crop0: int = 0) -> torch.Tensor:
    """Stretch2d(scale, 1) + Conv2d(1, 1, (1, 2 scale + 1), pad (0, scale)) along time on
    (B, W, C) rows -> (B, W_out, C) (default W * scale; crop0 = first output sample)."""
    _dev(x, w)
    x = x.contiguous()
    w = w.reshape(-1).float().contiguous()
    B, W, C = x.shape
    if w.numel() != 2 * scale + 1:
        raise ValueError(f'smoothing kernel of {w.numel()} taps for scale {scale}')
    W_out = W * scale if W_out is None else W_out
    y = torch.empty(B, W_out, C, device=x.device, dtype=_f32)
    launch('ftmi_wr_stretch_conv', f'wr_stretch_conv[B={B},W={W},C={C},s={scale}]',
           2.0 * B * W_out * C * (2 * scale + 1), 4.0 * (B * W * C + B * W_out * C),
           x.data_ptr(), W * C, B, W, C, scale, w.data_ptr(), y.data_ptr(), W_out * C, W_out, crop0,
           _stream())
    return y


def wavernn(args, B: int, L: int, flops: float, device, entry='wavernn', rows='B') -> None:
    """Enqueue ftmi_wavernn (args: a filled _lib.WaveRNNArgs; the caller keeps every buffer
    alive) — or ftmi_<entry>, whose probe label calls the B rows `rows`.  The status word
    pointer is set here."""
    args.status = status_word(device).data_ptr()
    mode = 'forward' if args.xin else 'generate'
    launch(f'ftmi_{entry}', f'{entry}[{mode},{rows}={B},L={L},NC={args.n_classes}]', flops,
           4.0 * B * L * (1 + (args.n_classes if args.logits else 0)), ctypes.byref(args), _stream())


def wavernn_route(n_folds: int):
    """[(NBV, NI, first fold, folds)]: the launches ftmi_wavernn / ftmi_wavernn_packed issue for
    n_folds folds under the current environment, as the library decides them."""
    n, buf = ctypes.c_int32(0), (ctypes.c_int32 * (4 * max(n_folds, 0)))()  # room: a fold per launch
    _lib.call('ftmi_wavernn_route', n_folds, buf, n_folds, ctypes.byref(n))
    return [tuple(buf[4 * i:4 * i + 4]) for i in range(n.value)]


def wavernn_workspace(device) -> torch.Tensor:
    n = int(_lib.load().ftmi_wavernn_workspace_bytes())
    return torch.empty(n // 4, device=device, dtype=torch.int32)


def wr_unfold(samples: torch.Tensor, target: int, overlap: int, batched: bool, mu_law: bool,
              n_classes: int, wave_len: int, fade_len: int) -> torch.Tensor:
    """generate's tail in float64 on the device: (B, L) samples -> (wave_len,) wave
    (fade_len: the final linear fade-out, 20 hop in generate, 0 for none)."""
    _dev(samples)
    samples = samples.contiguous()
    B, L = samples.shape
    out = torch.empty(wave_len, device=samples.device, dtype=torch.float64)
    launch('ftmi_wr_unfold', f'wr_unfold[B={B},L={L}]', 0, 4.0 * B * L + 8.0 * wave_len,
           samples.data_ptr(), B, L, target, overlap, int(batched), int(mu_law), n_classes,
           wave_len, fade_len, out.data_ptr(), _stream())
    return out


def _check_wr_table(query: str, what: str, cols, tbl: np.ndarray, *args) -> None:
    """The library's row check of a host table (ftmi_wr_check_folds / ftmi_wr_check_items), for a
    table that goes to the device: there the library cannot read it back."""
    tbl, bad = np.ascontiguousarray(tbl), ctypes.c_int32(-1)
    try:
        _lib.call(query, tbl.ctypes.data, tbl.shape[0], *args, ctypes.byref(bad))
    except _lib.FtmiError:
        if bad.value < 0:  # not a row: the call's own arguments
            raise
        raise ValueError(f'{what} {bad.value} out of range: '
                         f'{dict(zip(cols, tbl[bad.value].tolist()))}') from None


def check_wr_folds(folds: np.ndarray, L: int, n_out_rows: int, n_mel_rows: int, bias_row: int,
                   hop: int) -> None:
    """The row checks ftmi_wavernn_packed makes on a host table (csrc/wavernn.hip check_fold)."""
    f = np.asarray(folds)
    if f.ndim != 2 or f.shape[1] != len(_lib.WR_FOLD_COLS) or f.dtype != np.int32 or f.shape[0] == 0:
        raise ValueError(f'fold table: int32 (n, {len(_lib.WR_FOLD_COLS)}) expected, got {f.dtype} {f.shape}')
    _check_wr_table('ftmi_wr_check_folds', 'fold descriptor', _lib.WR_FOLD_COLS, f, L, n_out_rows,
                    n_mel_rows, bias_row, hop)


def wavernn_packed(args, folds: np.ndarray, launch_steps, flops: float, device, host_table=False):
    """Enqueue ftmi_wavernn_packed (args: a filled _lib.WaveRNNPackedArgs without the table; the
    caller keeps every buffer alive).  folds: host int32 (n, 8) table (_lib.WR_FOLD_COLS),
    checked here and handed over as device memory (host_table: handed over as it is, for the
    library to check and stage); launch_steps: per-launch step counts or None.  Returns the
    table handed over (to be kept until the stream has run the call)."""
    folds = np.ascontiguousarray(folds, dtype=np.int32)
    if host_table:
        tbl = folds
        args.folds = folds.ctypes.data
    else:
        check_wr_folds(folds, args.L, args.n_out_rows, args.n_mel_rows, args.bias_row, args.hop)
        tbl = torch.from_numpy(folds).to(device)
        args.folds = tbl.data_ptr()
    args.n_folds = folds.shape[0]
    if launch_steps is not None:
        steps = (ctypes.c_int32 * len(launch_steps))(*[int(v) for v in launch_steps])  # alive to the end
        if len(launch_steps) != len(wavernn_route(folds.shape[0])):
            raise ValueError('launch_steps: one entry per launch (wavernn_route)')
        args.launch_steps = ctypes.cast(steps, ctypes.c_void_p).value
    wavernn(args, folds.shape[0], args.L, flops, device, 'wavernn_packed', 'F')
    return tbl


def wr_unfold_packed(samples: torch.Tensor, items: np.ndarray, target: int, overlap: int,
                     batched: bool, mu_law: bool, n_classes: int, fade_len: int) -> torch.Tensor:
    """ftmi_wr_unfold of every utterance of a packed (F, L) sample matrix in one launch ->
    flat float64 waves; items: host int32 (n, 4) table (_lib.WR_ITEM_COLS), checked here by the
    library's row check and handed over as device memory."""
    _dev(samples)
    samples = samples.contiguous()
    F, L = samples.shape
    it = np.ascontiguousarray(items, dtype=np.int32)
    if it.ndim != 2 or it.shape[1] != len(_lib.WR_ITEM_COLS) or it.shape[0] == 0:
        raise ValueError(f'item table: int32 (n, {len(_lib.WR_ITEM_COLS)}) expected, got {it.shape}')
    out_len = int((it[:, 3].astype(np.int64) + it[:, 2]).max())  # the flat output ends with its last wave
    _check_wr_table('ftmi_wr_check_items', 'item', _lib.WR_ITEM_COLS, it, F, L, target, overlap,
                    int(batched), fade_len, out_len)
    tbl = torch.from_numpy(it).to(samples.device)
    out = torch.empty(out_len, device=samples.device, dtype=torch.float64)
    launch('ftmi_wr_unfold_packed', f'wr_unfold_packed[F={F},L={L},items={it.shape[0]}]', 0,
           4.0 * F * L + 8.0 * out_len, samples.data_ptr(), F, L, tbl.data_ptr(), it.shape[0], target,
           overlap, int(batched), int(mu_law), n_classes, fade_len, out.data_ptr(), out_len, _stream())
    return out


# ---- Tacotron decoder loop (csrc/tacotron.hip) ---------------------------------------------

TACO_MAX_TOKENS, TACO_MAX_BATCH = 512, 2  # include/ftmi.h FTMI_TACO_MAX_*


def tacotron_decoder_workspace(B: int, T: int, device) -> torch.Tensor:
    n = int(_lib.load().ftmi_tacotron_decoder_workspace_bytes(B, T))
    if n == 0:
        raise _lib.FtmiError(
            f'the Tacotron decoder launch takes 1..{TACO_MAX_TOKENS} tokens and up to '
            f'{TACO_MAX_BATCH} items per launch (got T={T}, B={B}): FTMI_E_UNSUPPORTED')
    return torch.empty(n // 4, device=device, dtype=torch.int32)


def tacotron_decoder(args, device) -> None:
    """Enqueue ftmi_tacotron_decoder (args: a filled _lib.TacoArgs; the caller keeps every
    buffer alive).  The status word pointer is set here."""
    args.status = status_word(device).data_ptr()
    mode = 'forward' if args.pre_gi else 'generate'
    n = (args.steps + args.r - 1) // args.r
    # per step: the 20 MB of weights' multiply-adds that are live (mel_proj: 80 r rows)
    flops = 2.0 * args.B * n * (768 * 640 + 256 * 256 + 512 * 512 + 4 * 2048 * 512
                                + 80 * args.r * 512 + 2 * args.T * 256)
    launch('ftmi_tacotron_decoder', f'tacotron_decoder[{mode},B={args.B},T={args.T},r={args.r},n={n}]',
           flops, 4.0 * args.B * n * (80 * args.r + args.T), ctypes.byref(args), _stream())


# ---- Alignment: durations and attention scores (csrc/align.hip) ------------------------------

_ALIGN_WS = {}  # (device, stream) -> uint8 workspace, grown on demand


def align_workspace(B: int, rows: int, T: int, device) -> torch.Tensor:
    """The direction workspace of ftmi_align_dijkstra, cached per device and stream (it is
    scratch: nothing in it outlives a launch)."""
    n = int(_lib.load().ftmi_align_workspace_bytes(B, rows, T))
    if n == 0:
        raise _lib.FtmiError(f'the alignment kernels take 1..{TACO_MAX_TOKENS} tokens and at least '
                             f'one row and item (got B={B}, rows={rows}, T={T}): FTMI_E_UNSUPPORTED')
    dev = torch.device(device)
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device(), _stream())
    ws = _ALIGN_WS.get(key)
    if ws is None or ws.numel() < n:
        ws = _ALIGN_WS[key] = torch.empty(n, device=device, dtype=torch.uint8)
    return ws


def _align_args(att: torch.Tensor, mel_len: torch.Tensor, x_len: Optional[torch.Tensor]):
    """(B, rows, T, ld_row, ld_item) of a (B, rows, T) fp32 attention with unit column stride;
    the length vectors must be int32 [B] on att's device."""
    _dev(att, mel_len, x_len)
    if att.dim() != 3 or att.dtype != _f32 or 0 in att.shape:
        raise ValueError(f'att must be a non-empty (B, rows, T) fp32 tensor, got shape '
                         f'{tuple(att.shape)} {att.dtype}')
    B, rows, T = att.shape
    # a stride of a size-1 dimension is never used
    ld_row = att.stride(1) if rows > 1 else T
    ld_item = att.stride(0) if B > 1 else 0
    if (T > 1 and att.stride(2) != 1) or ld_row < T or ld_item < 0:
        raise ValueError(f'att needs unit column stride and a row stride >= T, got shape '
                         f'{tuple(att.shape)} strides {att.stride()}')
    for name, v in (('mel_len', mel_len), ('x_len', x_len)):
        if v is not None and (v.dtype != torch.int32 or v.shape != (B,) or not v.is_contiguous()
                              or v.device != att.device):
            raise ValueError(f'{name} must be a contiguous int32 [{B}] tensor on {att.device}')
    return B, rows, T, ld_row, ld_item


def align_dijkstra(att: torch.Tensor, mel_len: torch.Tensor, x_len: Optional[torch.Tensor] = None,
                   want_cost: bool = False, workspace: Optional[torch.Tensor] = None):
    """Shortest-monotone-path durations (ftmi_align_dijkstra): int32 (B, T) and, with
    want_cost, the path costs as float64 [B] (else None).  The lengths are NOT checked here
    (the kernel clamps them); forwardtacotron_amd.align validates them."""
    B, rows, T, ld_row, ld_item = _align_args(att, mel_len, x_len)
    ws = align_workspace(B, rows, T, att.device) if workspace is None else workspace
    dur = torch.empty(B, T, device=att.device, dtype=torch.int32)
    cost = torch.empty(B, device=att.device, dtype=torch.float64) if want_cost else None
    launch('ftmi_align_dijkstra', f'align_dijkstra[B={B},rows={rows},T={T}]', 3.0 * B * rows * T,
           5.0 * B * rows * T, att.data_ptr(), ld_row, ld_item, B, rows, T, mel_len.data_ptr(),
           _ptr(x_len), dur.data_ptr(), _ptr(cost), ws.data_ptr(), _stream())
    return dur, cost


def align_count(att: torch.Tensor, mel_len: torch.Tensor,
                x_len: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Attention-peak-count durations (ftmi_align_count): int32 (B, T)."""
    B, rows, T, ld_row, ld_item = _align_args(att, mel_len, x_len)
    dur = torch.empty(B, T, device=att.device, dtype=torch.int32)
    launch('ftmi_align_count', f'align_count[B={B},rows={rows},T={T}]', 0, 4.0 * B * rows * T,
           att.data_ptr(), ld_row, ld_item, B, rows, T, mel_len.data_ptr(), _ptr(x_len),
           dur.data_ptr(), _stream())
    return dur


def attention_score(att: torch.Tensor, mel_len: torch.Tensor, r: int = 1):
    """(loc_score, sharp_score), fp32 [B] each (ftmi_attention_score)."""
    B, rows, T, ld_row, ld_item = _align_args(att, mel_len, None)
    if r < 1:
        raise ValueError(f'r must be >= 1, got {r}')
    loc = torch.empty(B, device=att.device, dtype=_f32)
    sharp = torch.empty(B, device=att.device, dtype=_f32)
    launch('ftmi_attention_score', f'attention_score[B={B},rows={rows},T={T}]', 0,
           4.0 * B * rows * T, att.data_ptr(), ld_row, ld_item, B, rows, T, mel_len.data_ptr(),
           int(r), loc.data_ptr(), sharp.data_ptr(), _stream())
    return loc, sharp


# ---- Phoneme-level pitch and energy (csrc/align.hip) -----------------------------------------

def phoneme_features(mel: torch.Tensor, mel_len: torch.Tensor, dur: torch.Tensor,
                     x_len: Optional[torch.Tensor] = None, pitch: Optional[torch.Tensor] = None,
                     pitch_len: Optional[torch.Tensor] = None, pitch_max_freq: float = 600.0):
    """Per-token means of the frame energy and of the voiced frame pitch
    (ftmi_phoneme_features): mel (B, n_mels, rows) fp32 with unit frame stride, dur (B, T) int32,
    pitch (B, P) fp32 with pitch_len, or both None -> (pitch_char or None, energy_char, dur_sum):
    fp32 (B, T), fp32 (B, T), int32 [B].  The lengths are NOT checked here (the kernel clamps
    them); forwardtacotron_amd.align validates them and compares dur_sum with mel_len."""
    _dev(mel, mel_len, dur, x_len, pitch, pitch_len)
    if mel.dim() != 3 or mel.dtype != _f32 or 0 in mel.shape:
        raise ValueError(f'mel must be a non-empty (B, n_mels, rows) fp32 tensor, got shape '
                         f'{tuple(mel.shape)} {mel.dtype}')
    B, n_mels, rows = mel.shape
    if dur.dim() != 2 or dur.dtype != torch.int32 or dur.size(0) != B or dur.size(1) == 0:
        raise ValueError(f'dur must be a ({B}, T) int32 tensor, got shape {tuple(dur.shape)} {dur.dtype}')
    T = dur.size(1)
    # a stride of a size-1 dimension is never used
    ld_bin = mel.stride(1) if n_mels > 1 else rows
    ld_item = mel.stride(0) if B > 1 else 0
    ld_dur = dur.stride(0) if B > 1 else T
    if (rows > 1 and mel.stride(2) != 1) or ld_bin < rows or ld_item < 0:
        raise ValueError(f'mel needs unit frame stride and a bin stride >= rows, got shape '
                         f'{tuple(mel.shape)} strides {mel.stride()}')
    if (T > 1 and dur.stride(1) != 1) or ld_dur < T:
        raise ValueError(f'dur needs unit column stride and a row stride >= T, got strides {dur.stride()}')
    if (pitch is None) != (pitch_len is None):
        raise ValueError('pitch and pitch_len come together')
    P = ld_pitch = 0
    if pitch is not None:
        if pitch.dim() != 2 or pitch.dtype != _f32 or pitch.size(0) != B or pitch.size(1) == 0:
            raise ValueError(f'pitch must be a ({B}, P) fp32 tensor, got shape {tuple(pitch.shape)} '
                             f'{pitch.dtype}')
        P = pitch.size(1)
        ld_pitch = pitch.stride(0) if B > 1 else P
        if (P > 1 and pitch.stride(1) != 1) or ld_pitch < P:
            raise ValueError(f'pitch needs unit column stride and a row stride >= P, got strides '
                             f'{pitch.stride()}')
    for name, v in (('mel_len', mel_len), ('x_len', x_len), ('pitch_len', pitch_len)):
        if v is not None and (v.dtype != torch.int32 or v.shape != (B,) or not v.is_contiguous()
                              or v.device != mel.device):
            raise ValueError(f'{name} must be a contiguous int32 [{B}] tensor on {mel.device}')
    energy_out = torch.empty(B, T, device=mel.device, dtype=_f32)
    pitch_out = None if pitch is None else torch.empty(B, T, device=mel.device, dtype=_f32)
    dur_sum = torch.empty(B, device=mel.device, dtype=torch.int32)
    launch('ftmi_phoneme_features', f'phoneme_features[B={B},rows={rows},T={T}]',
           30.0 * B * n_mels * rows, 4.0 * B * (n_mels + 1) * rows, mel.data_ptr(), ld_bin, ld_item,
           B, n_mels, rows, mel_len.data_ptr(), dur.data_ptr(), ld_dur, T, _ptr(x_len), _ptr(pitch),
           ld_pitch, P, _ptr(pitch_len), float(pitch_max_freq), _ptr(pitch_out),
           energy_out.data_ptr(), dur_sum.data_ptr(), _stream())
    return pitch_out, energy_out, dur_sum


def _flat_f32(values: torch.Tensor) -> int:
    _dev(values)
    if values.dtype != _f32 or not values.is_contiguous() or values.numel() == 0:
        raise ValueError(f'values must be a non-empty contiguous fp32 tensor, got shape '
                         f'{tuple(values.shape)} {values.dtype}')
    return values.numel()


def nonzero_moments(values: torch.Tensor) -> torch.Tensor:
    """float64 [3] on the device: the count of non-zero entries of `values`, their mean and
    their population standard deviation (ftmi_nonzero_moments); 0, 0, 0 without any."""
    n = _flat_f32(values)
    out = torch.empty(3, device=values.device, dtype=torch.float64)
    launch('ftmi_nonzero_moments', f'nonzero_moments[n={n}]', 4.0 * n, 8.0 * n,
           values.data_ptr(), n, out.data_ptr(), _stream())
    return out


def normalize_nonzero(values: torch.Tensor, mean: float, std: float) -> torch.Tensor:
    """values = (values - mean) / std in place where values != 0, in fp32
    (ftmi_normalize_nonzero).  Returns values."""
    n = _flat_f32(values)
    launch('ftmi_normalize_nonzero', f'normalize_nonzero[n={n}]', 2.0 * n, 8.0 * n,
           values.data_ptr(), n, float(mean), float(std), _stream())
    return values


# ---- Validation losses (csrc/eval.hip) --------------------------------------------------------

_EVAL_WS = {}  # (device, stream) -> uint8 workspace of per-workgroup partials, grown on demand


def eval_workspace(nbytes: int, device, what: str) -> torch.Tensor:
    """The partial-sum workspace of the loss kernels, cached per device and stream (scratch:
    nothing in it outlives an entry point).  nbytes == 0 is the query's answer for a shape the
    kernels do not take."""
    if nbytes <= 0:
        raise _lib.FtmiError(f'{what}: FTMI_E_UNSUPPORTED (the workspace query returned 0)')
    dev = torch.device(device)
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device(), _stream())
    ws = _EVAL_WS.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = _EVAL_WS[key] = torch.empty(nbytes, device=device, dtype=torch.uint8)
    return ws


def _l1_strides(t: torch.Tensor, name: str) -> Tuple[int, int, int]:
    """(item, channel, frame) strides of a (B, C, L) operand of ftmi_l1_loss: frame-major or
    channel-major planes.  A stride of a size-1 dimension is never used, so it is replaced by
    the one a contiguous tensor would have."""
    B, C, L = t.shape
    s_b, s_c, s_t = t.stride()
    if L == 1:
        s_t = 1
    if C == 1:
        s_c = L if s_t == 1 else 1
    if B == 1:
        s_b = 0
    if s_b < 0 or not ((s_t == 1 and s_c >= L) or (s_c == 1 and s_t >= C)):
        raise ValueError(f'{name} needs unit frame stride with a channel stride >= L, or unit channel '
                         f'stride with a frame stride >= C, got shape {tuple(t.shape)} strides '
                         f'{t.stride()}')
    return s_b, s_c, s_t


def l1_loss(x: torch.Tensor, target: torch.Tensor, lens: Optional[torch.Tensor] = None,
            out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Masked (lens: int32 [B], frames t < lens[b] count) or plain mean |x - target| of two fp32
    (B, C, L) tensors (ftmi_l1_loss) -> 0-d fp32 on the device, or `out` (one fp32 element)."""
    _dev(x, target, lens, out)
    for name, t in (('x', x), ('target', target)):
        if t.dim() != 3 or t.dtype != _f32 or 0 in t.shape:
            raise ValueError(f'{name} must be a non-empty (B, C, L) fp32 tensor, got shape '
                             f'{tuple(t.shape)} {t.dtype}')
    if x.shape != target.shape or x.device != target.device:
        raise ValueError(f'x and target must agree in shape and device, got {tuple(x.shape)} and '
                         f'{tuple(target.shape)}')
    B, C, L = x.shape
    xs, ts = _l1_strides(x, 'x'), _l1_strides(target, 'target')
    if lens is not None and (lens.dtype != torch.int32 or lens.shape != (B,)
                             or not lens.is_contiguous() or lens.device != x.device):
        raise ValueError(f'lens must be a contiguous int32 [{B}] tensor on {x.device}')
    if out is None:
        out = torch.empty((), device=x.device, dtype=_f32)
    elif out.dtype != _f32 or out.numel() != 1 or out.device != x.device:
        raise ValueError('out must hold one fp32 element on the device of x')
    ws = eval_workspace(int(_lib.load().ftmi_l1_loss_workspace_bytes(B, C, L)), x.device,
                        f'l1_loss[B={B},C={C},L={L}]')
    n = float(B) * C * L
    launch('ftmi_l1_loss', f'l1_loss[B={B},C={C},L={L}]', 3.0 * n, 8.0 * n, x.data_ptr(), *xs,
           target.data_ptr(), *ts, B, C, L, _ptr(lens), out.data_ptr(), ws.data_ptr(), _stream())
    return out


def _loss_rows(t: torch.Tensor, name: str) -> Tuple[int, int, int]:
    """(rows, C, ld) of a (rows, C) fp32 matrix with unit column stride and a row stride >= C."""
    if t.dim() != 2 or t.dtype != _f32 or 0 in t.shape:
        raise ValueError(f'{name} must be a non-empty (rows, C) fp32 tensor, got shape '
                         f'{tuple(t.shape)} {t.dtype}')
    rows, C = t.shape
    ld = t.stride(0) if rows > 1 else C
    if (C > 1 and t.stride(1) != 1) or ld < C:
        raise ValueError(f'{name} needs unit column stride and a row stride >= C, got shape '
                         f'{tuple(t.shape)} strides {t.stride()}')
    return rows, C, ld


def cross_entropy(logits: torch.Tensor, target: torch.Tensor):
    """(loss, bad): the mean cross-entropy of fp32 (rows, C) logits against int32 [rows] labels
    as a 0-d fp32 tensor, and a 0-d int32 count of labels outside [0, C), which add nothing to
    the sum (ftmi_cross_entropy).  The caller reads `bad` with the loss; nothing syncs here."""
    _dev(logits, target)
    rows, C, ld = _loss_rows(logits, 'logits')
    if (target.dtype != torch.int32 or target.shape != (rows,) or not target.is_contiguous()
            or target.device != logits.device):
        raise ValueError(f'target must be a contiguous int32 [{rows}] tensor on {logits.device}')
    label = f'cross_entropy[rows={rows},C={C}]'
    ws = eval_workspace(int(_lib.load().ftmi_cross_entropy_workspace_bytes(rows, C)), logits.device,
                        label)
    out = torch.empty((), device=logits.device, dtype=_f32)
    bad = torch.empty((), device=logits.device, dtype=torch.int32)
    launch('ftmi_cross_entropy', label, 4.0 * rows * C, 4.0 * rows * (C + 1), logits.data_ptr(), ld,
           rows, C, target.data_ptr(), out.data_ptr(), bad.data_ptr(), ws.data_ptr(), _stream())
    return out, bad


def mol_loss(y_hat: torch.Tensor, y: torch.Tensor, num_classes: float, log_scale_min: float,
             per_sample: bool = False):
    """(loss, per_sample or None): the discretized mixture-of-logistics loss of fp32 (rows, 3 K)
    parameters against fp32 [rows] samples (ftmi_mol_loss): 0-d fp32, and with per_sample the
    fp32 [rows] values of reduce=False."""
    _dev(y_hat, y)
    rows, C, ld = _loss_rows(y_hat, 'y_hat')
    if C % 3 != 0:
        raise ValueError(f'y_hat needs 3 K columns, got {C}')
    if (y.dtype != _f32 or y.shape != (rows,) or not y.is_contiguous() or y.device != y_hat.device):
        raise ValueError(f'y must be a contiguous fp32 [{rows}] tensor on {y_hat.device}')
    label = f'mol_loss[rows={rows},K={C // 3}]'
    ws = eval_workspace(int(_lib.load().ftmi_mol_loss_workspace_bytes(rows, C // 3)), y_hat.device,
                        label)
    out = torch.empty((), device=y_hat.device, dtype=_f32)
    ps = torch.empty(rows, device=y_hat.device, dtype=_f32) if per_sample else None
    launch('ftmi_mol_loss', label, 60.0 * rows * C, 4.0 * rows * (C + 1 + bool(per_sample)),
           y_hat.data_ptr(), ld, rows, C, y.data_ptr(), float(num_classes), float(log_scale_min),
           out.data_ptr(), _ptr(ps), ws.data_ptr(), _stream())
    return out, ps
