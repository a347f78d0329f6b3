"""Launch lists: a module's kernel chain issued by one `ftmi_run_chain` call.

From Python every launch costs a `torch.empty`, a ctypes argument block, a label and (under
a KernelProbe) two events — tens of microseconds each, which at batch 64 is what bounds the
phoneme phase of `generate()`: its last predictor starts when the host gets round to it.
A plan replaces a chain's launches with one foreign call.

No kernel-selection rule lives here or in C++.  A plan is RECORDED: the first call at a key
runs the module's ordinary per-op path (`ops.*`, which decides split-K, skinny / slab,
matrix path, recurrence form as always) with a recorder that notes every launch's arguments
and every tensor the ops allocate.  The recorded device pointers are then rewritten as
(slot, byte offset, extent) references — ids, status word, packed weights, output, and ONE
workspace in which the intermediates are laid out by lifetime — and the list is kept on the
module, keyed like its weight packs.  Later calls at the key allocate the workspace and the
output, patch three bases and make one call: the same kernels with the same arguments in
the same order, so the results are bit-identical to the per-op path.

One chain is issued this way: a SeriesPredictor (embedding, three convs, GRU, head).  The
prenet chain (CBHG.forward_ids + the LSTM input projection) was built as a second list and
measured: it did not separate from the predictors' lists alone, so it
issues per op.

A module keeps at most MAX_PLANS plans (least recently used dropped).  Recording costs one
per-op pass plus the rewrite (tools/chain_build_cost.py measures it), so a caller whose
shapes never repeat pays that on top of every call: FTMI_CHAIN=0 is the setting for it.
A plan's op and base arrays are patched in place per call: one host thread per module at a
time (as everywhere in this package: neither the packs (common_layers.cached_pack) nor the
captured phases (phase_graph) are locked either).

FTMI_CHAIN=0 (or chain.CHAIN = False) keeps the per-op path: per-kernel profiling, A/B.
"""
from __future__ import annotations

import ctypes
import os
from typing import List, Optional

import torch

from . import _lib, ops, probe
from ._lib import ChainBase, ChainOp, FtmiError
from .common_layers import cached_pack

CHAIN = os.environ.get('FTMI_CHAIN', '1') != '0'
BUILDS = 0  # plans built so far (tests count them)
ALIGN = 256  # workspace offsets (the kernels need 16)

MAX_PLANS = 16  # per module
SLOT_IDS, SLOT_WS, SLOT_STATUS, SLOT_OUT = 0, 1, 2, 3  # further outputs, then the weights
_TAGS = {'ftmi_embedding': _lib.CHAIN_EMBEDDING, 'ftmi_conv1d': _lib.CHAIN_CONV1D,
         'ftmi_rnn_bidir': _lib.CHAIN_RNN_BIDIR, 'ftmi_rowdot': _lib.CHAIN_ROWDOT}
_INTS = (_lib.c_int, _lib.c_int64)


class Recorder:
    """What probe.launch and ops._new note while a plan's per-op pass runs."""

    def __init__(self):
        self.launches = []  # (entry point, label, flops, bytes, args)
        self.allocs = []    # tensors the ops allocated (kept alive: no address is reused)

    def __enter__(self):
        if probe._RECORDER is not None:
            raise RuntimeError('a launch list is already being recorded')
        probe._RECORDER = self
        return self

    def __exit__(self, *exc):
        probe._RECORDER = None
        return False


def _typed_args(name: str, args):
    """(type, value) of one recorded launch's arguments in the entry point's order, the
    stream left out; a by-reference argument block (ftmi_conv_args) is flattened."""
    types = _lib.SIGNATURES[name][1]
    out = []
    for t, v in zip(types[:-1], args[:-1]):
        if isinstance(t, type) and issubclass(t, ctypes._Pointer):
            blk = v._obj
            out += [(ft, getattr(blk, fn)) for fn, ft in blk._fields_]
        else:
            out.append((t, v))
    return out


def _flatten(pack) -> List[torch.Tensor]:
    if isinstance(pack, torch.Tensor):
        return [pack]
    if isinstance(pack, (tuple, list)):
        return [t for p in pack for t in _flatten(p)]
    return []


def _span(t: torch.Tensor):
    return t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()


class Plan:
    """One recorded chain: the op list, the base table and the workspace layout."""

    def __init__(self, rec: Recorder, ids: torch.Tensor, outs, weights, label: str):
        global BUILDS
        launches = rec.launches
        for l in launches:
            if l[0] not in _TAGS:
                raise FtmiError(f'launch list: {l[0]} has no chain op')
        n = len(launches)
        if n == 0:
            raise FtmiError('launch list: nothing was recorded')
        BUILDS += 1
        status = ops.status_word(ids.device)
        inter = [t for t in rec.allocs if not any(t is o for o in outs)]
        # which launches touch which intermediate: first / last use give its lifetime
        spans = [_span(t) for t in inter]
        first, last = [None] * len(inter), [None] * len(inter)
        typed = []
        for k, (name, _, _, _, args) in enumerate(launches):
            ta = _typed_args(name, args)
            typed.append(ta)
            for t, v in ta:
                if t is _lib.P and v:
                    for j, (lo, hi) in enumerate(spans):
                        if lo <= v < hi:
                            first[j] = k if first[j] is None else first[j]
                            last[j] = k
        # lay the intermediates out: lowest offset free of every intermediate still live
        # (one stream, launches in order: a range is free once its last reader is queued)
        offs, sizes, placed = [0] * len(inter), [0] * len(inter), []
        total = 0
        for j, t in enumerate(inter):
            if first[j] is None:
                continue
            size = -(-(spans[j][1] - spans[j][0]) // ALIGN) * ALIGN
            busy = sorted((o, o + s) for o, s, l in placed if l >= first[j])
            off = 0
            for lo, hi in busy:
                if off + size <= lo:
                    break
                off = max(off, hi)
            offs[j], sizes[j] = off, size
            placed.append((off, size, last[j]))
            total = max(total, off + size)
        self.ws_bytes = max(total, ALIGN)
        # fixed regions: (lo, hi, slot); weights get their slots as they are met
        self.keep = [status] + list(weights)  # the packs the list points into stay alive
        wspans = [_span(t) for t in weights]
        wslot = {}
        fixed = [(*_span(ids), SLOT_IDS), (*_span(status), SLOT_STATUS)]
        fixed += [(*_span(o), SLOT_OUT + j) for j, o in enumerate(outs)]
        bases = [(0, ids.numel() * 8), (0, self.ws_bytes), _base(status)]
        bases += [(0, o.numel() * o.element_size()) for o in outs]

        def resolve(v):
            for j, (lo, hi) in enumerate(spans):
                if lo <= v < hi:
                    return SLOT_WS, offs[j] + v - lo, sizes[j] - (v - lo)
            for lo, hi, slot in fixed:
                if lo <= v < hi:
                    return slot, v - lo, hi - v
            for j, (lo, hi) in enumerate(wspans):
                if lo <= v < hi:
                    if j not in wslot:
                        wslot[j] = len(bases)
                        bases.append((lo, hi - lo))
                    return wslot[j], v - lo, hi - v
            raise FtmiError('launch list: a recorded pointer belongs to no known tensor')

        self.ops = (ChainOp * n)()
        self.names = []
        self.float_ops = {}
        flops = nbytes = 0.0
        for k, (name, lbl, fl, nb, _) in enumerate(launches):
            op = self.ops[k]
            op.tag = _TAGS[name]
            for ref in op.p:
                ref.slot = -1
            self.names.append(lbl)
            self.float_ops.setdefault(name, k)
            flops += fl
            nbytes += nb
            np_ = ni = nf = 0
            for t, v in typed[k]:
                if t is _lib.P:
                    ref = op.p[np_]
                    np_ += 1
                    if not v:
                        continue
                    ref.slot, ref.offset, ref.bytes = resolve(v)
                    # the executor demands alignment only of the workspace it lays out itself
                    # (a misaligned one is refused before anything runs); what the caller
                    # owns (ids, outputs, weights) is held to the entry points' own checks,
                    # exactly as on the per-op path
                    ref.flags = _lib.CHAIN_ALIGN16 if ref.slot == SLOT_WS else 0
                elif t in _INTS:
                    op.i[ni] = int(v)
                    ni += 1
                else:
                    op.f[nf] = float(v)
                    nf += 1
        self.n = n
        self.n_bases = len(bases)
        self.bases = (ChainBase * self.n_bases)()
        for b, (ptr, size) in zip(self.bases, bases):
            b.base, b.bytes = ptr or None, size
        self.out_shapes = [tuple(o.shape) for o in outs]
        self.out_shape = self.out_shapes[0]
        self.label, self.flops, self.nbytes = label, flops, nbytes
        self.failed = ctypes.c_int32(-1)
        self.alpha_op = None  # index of the op whose f[0] is the per-call alpha

    def run(self, ids: torch.Tensor, alpha: Optional[float] = None,
            ws: Optional[torch.Tensor] = None):
        """One call of the chain on torch's current stream; returns its output (a tuple when
        the chain has several).  alpha: the head's divisor (the one argument that changes
        from call to call at a key); ws: a caller-owned workspace of at least `ws_bytes`
        bytes (default: a fresh one from torch's allocator)."""
        if ids.numel() * 8 != self.bases[SLOT_IDS].bytes or ids.dtype != torch.int64:
            raise ValueError('launch list: ids do not have the shape the list was built for')
        if alpha is not None and self.alpha_op is not None:
            self.ops[self.alpha_op].f[0] = alpha
        if ws is None:
            ws = torch.empty(self.ws_bytes, device=ids.device, dtype=torch.uint8)
        b = self.bases
        b[SLOT_IDS].base = ids.data_ptr()
        b[SLOT_WS].base = ws.data_ptr()
        outs = []
        for j, shape in enumerate(self.out_shapes):
            o = torch.empty(shape, device=ids.device, dtype=torch.float32)
            b[SLOT_OUT + j].base = o.data_ptr()
            outs.append(o)
        self.launch()
        return outs[0] if len(outs) == 1 else tuple(outs)

    def launch(self) -> None:
        try:
            probe.launch('ftmi_run_chain', self.label, self.flops, self.nbytes, self.ops, self.n,
                         self.bases, self.n_bases, ctypes.byref(self.failed), ops._stream())
        except FtmiError as e:
            k = self.failed.value
            what = self.names[k] if 0 <= k < self.n else 'the list'
            raise FtmiError(f'{e} (op {k}: {what})') from None


def _base(t: torch.Tensor):
    return t.data_ptr(), t.numel() * t.element_size()


def policy_key():
    """Everything besides the shape and the weights that the per-op path's choices read: a
    change of any builds another plan.  The library's routing switches enter as its own
    digest of them (ftmi_gemm_switches_digest), so none is listed here.  The recurrences'
    switches (ftmi_rnn_switches_digest) need no place in it: a plan records the ftmi_rnn_bidir
    call, not its kernel, and the replayed call reads them itself."""
    return (ops.MMA, ops.RNN_MMA, ops._FORCED[-1] if ops._FORCED else None, bool(ops._COMPACT),
            _lib.load().ftmi_gemm_switches_digest())


def _plans(mod):
    """The module's plans of its current weights: they live on the module next to its packs
    and are dropped with them (load_state_dict, .to, in-place updates change the pack key)."""
    return cached_pack(mod, '_ftmi_chain', dict)


def _lookup(plans, key):
    plan = plans.pop(key, None)
    if plan is not None:
        plans[key] = plan  # most recently used last
    return plan


def _store(plans, key, plan) -> None:
    while len(plans) >= MAX_PLANS:
        plans.pop(next(iter(plans)))
    plans[key] = plan


def _ids(x: torch.Tensor) -> torch.Tensor:
    ids = x.contiguous()
    return ids if ids.dtype == torch.int64 else ids.long()


def _predictor_key(mod, ids):
    return (tuple(ids.shape), ids.device, mod.rnn.spread, policy_key())


def cached_plan(mod, ids: torch.Tensor) -> Optional[Plan]:
    """The plan a SeriesPredictor call with these ids would run now, or None if it would
    record one."""
    return _plans(mod).get(_predictor_key(mod, _ids(ids)))


def series_predictor(mod, x: torch.Tensor, alpha: float) -> torch.Tensor:
    """SeriesPredictor.forward_bt through its launch list: embedding, three BatchNormConv
    (with their split-K finishes), the GRU input projection, the recurrence and the head."""
    ops._dev(x, mod.embedding.weight)
    ids = _ids(x)
    plans, key = _plans(mod), _predictor_key(mod, ids)
    plan = _lookup(plans, key)
    if plan is None:
        # the packs first: building one launches its own (unrecorded) split kernels
        weights = [mod.embedding.weight.detach()] + _flatten(
            [m.packed_weights() for m in (*mod.convs, mod.rnn, mod)])
        with Recorder() as rec:
            out = mod._forward_ops(ids, alpha)
        B, T = ids.shape
        plan = Plan(rec, ids, [out], weights, f'series_predictor[B={B},T={T},H={mod.rnn.hidden}]')
        plan.alpha_op = plan.float_ops['ftmi_rowdot']
        _store(plans, key, plan)
        return out  # the recording pass ran the chain per op: its result is this call's
    return plan.run(ids, alpha)

