"""The phoneme phase of `generate()` as a HIP graph — one protocol for every model.

A model's phoneme phase (predictors, prenet, duration counts) is tens to hundreds of
launches from Python over four streams; as a graph it is one replay, which matters where
the kernels are short (batch 1: the host issue rate, not the device, sets the phase's
length).  Both models' phases return one record, `Phase`; `phoneme_phase` is the way into
either (the graph where it may be used, else the eager phase) and `replay` holds what the
graphs share; a model brings its phase function, its key part (`policy`) and the eager
finish of a split graph.

Keyed on (device, x shape, alpha, the callbacks' identity, the model's `policy`: its matrix
paths); a key is captured the SECOND time it is seen (a one-off shape — gen_forward.py's
sentences of different lengths — stays eager: capture costs ~3 eager phases), sightings
are forgotten once 64 x CACHE keys have been seen (a new lambda per call), and CACHE
captured phases are kept per model, least recently used dropped.  A capture that fails (a
callback that syncs or leaves the device) marks the key eager for good.

The default identity and callbacks marked `graph_safe` are captured with the phase.  Any
other callback — gen_forward.py's plain `lambda x: x * amp` — splits it: the graph holds
everything but the callbacks and the one launch that reads their outputs (series_proj_add);
after each replay the callbacks run eagerly on the predictors' outputs (fresh tensors, on
the caller's stream), as the reference calls them, and the model's `finish` issues that
launch.  The split graph is keyed 'split', without the callbacks' identity (they are not
in it).

Static buffers: x is copied in, dur / pitch / energy are cloned out (they go back to the
caller); h and offsets are consumed by this call's decoder — the next replay waits for the
decoder's completion event (entry['done'], recorded by the `consumed` callable that
`phoneme_phase` hands out with the record), so calls on different streams never overwrite
buffers a decoder still reads.

An entry keeps every weight pack of the model alive (common_layers.held_packs: the
captured kernels point into them) and the model-wide weights key of its capture: after
each replay (while it runs) the key is compared with the model's, and on a change
(load_state_dict, .to(), in-place updates) every captured phase is dropped and the call
falls back to the eager phase (the stale replay read the old, still-held packs; its
outputs are discarded).
"""
from __future__ import annotations

from typing import Callable, NamedTuple, Optional, Union

import torch

from .common_layers import held_packs, weights_key

CACHE = 8  # captured phases kept per model (least recently used dropped)


class Phase(NamedTuple):
    """What a model's phoneme phase hands to its decoder.  dur (B, T), pitch and energy
    (B, 1, T) go back to the caller: replay clones them out of the static buffers."""
    dur: torch.Tensor
    pitch: torch.Tensor
    energy: torch.Tensor
    h: torch.Tensor  # the rows the decoder reads; a split graph's finish adds into them
    offsets: torch.Tensor  # the LengthRegulator offsets of ops.duration_counts
    t_mel: Union[int, torch.Tensor]  # max(totals): on the device while captured, else an int
    index: Optional[torch.Tensor] = None  # the LR index map where the phase queued it already


def _identity(t: torch.Tensor) -> torch.Tensor:
    """The default pitch / energy callback (the reference's `lambda x: x`)."""
    return t


def graph_safe(fn: Callable[[torch.Tensor], torch.Tensor]) -> Callable[[torch.Tensor], torch.Tensor]:
    """Mark a pitch / energy callback as safe to capture in the phoneme-phase HIP graph: a
    pure function of its tensor argument made of device-side torch ops, whose behaviour
    does not change between calls (no Python-side state it reads changes: closure
    variables, attributes, scalars).  gen_forward.py's `lambda x: x * amp` is, for the run's
    fixed `amp`.  An unmarked callback runs eagerly on every call, as the reference calls
    it (`models/forward_tacotron.py:258-261`); returns fn."""
    fn._ftmi_graph_safe = True
    return fn


def _graphable(fn) -> bool:
    return fn is _identity or getattr(fn, '_ftmi_graph_safe', False) is True


def replay(model, phase_fn, finish, policy, x, alpha, pitch_fn, energy_fn):
    """One phoneme phase of `model` from its captured graph (see the module docstring).
    phase_fn(sx, alpha, pitch_fn, energy_fn, capture=True): the model's phase on the static
    input sx without a host sync, returning a Phase with t_mel on the device (pitch_fn =
    energy_fn = None: the split graph — raw predictor outputs, their projections not added
    to h).  finish(phase): the launch a split graph leaves out, on the Phase that holds the
    callbacks' results.  policy: the model's part of the key.  Returns (Phase with t_mel
    read to the host, entry) or None (run the eager phase)."""
    cache = model.__dict__.setdefault('_ftmi_graphs', {})
    seen = model.__dict__.setdefault('_ftmi_graph_seen', {})
    split = not (_graphable(pitch_fn) and _graphable(energy_fn))
    fns = ('split',) if split else (pitch_fn, energy_fn)
    key = (x.device, tuple(x.shape), float(alpha), *fns, *policy)
    ent = cache.pop(key, None)
    fresh = False
    if ent is None:
        n = seen.get(key, 0)
        if n < 0:
            return None  # capture failed before: eager for good
        if len(seen) >= 64 * CACHE:  # e.g. a new lambda per call: forget sightings
            seen.clear()
        seen[key] = n + 1
        if n == 0:
            return None  # first sighting: eager
        cap = (None, None) if split else fns
        wkey = weights_key(model)
        sx = x.clone()
        try:
            phase_fn(sx, alpha, *cap, capture=True)  # warm-up
            torch.cuda.synchronize(x.device)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                outs = phase_fn(sx, alpha, *cap, capture=True)
        except Exception:  # pylint: disable=broad-except
            torch.cuda.synchronize(x.device)
            seen[key] = -1
            return None
        ent = {'g': g, 'sx': sx, 'outs': outs, 'wkey': wkey, 'packs': held_packs(model),
               'done': torch.cuda.Event()}
        ent['done'].record(torch.cuda.current_stream(x.device))
        fresh = True
        while len(cache) >= CACHE:
            cache.pop(next(iter(cache)))
    cache[key] = ent  # most recently used last
    main = torch.cuda.current_stream(x.device)
    main.wait_event(ent['done'])  # the previous decoder is done with the static buffers
    ent['sx'].copy_(x)
    ent['g'].replay()
    if not fresh and weights_key(model) != ent['wkey']:
        main.synchronize()  # the stale replay must finish before its graph is freed
        cache.clear()
        return None
    phase = ent['outs']
    t_host = torch.empty((), dtype=phase.t_mel.dtype, pin_memory=True)
    t_host.copy_(phase.t_mel, non_blocking=True)
    t_ready = torch.cuda.Event()
    t_ready.record(main)
    dur, pitch, energy = phase.dur.clone(), phase.pitch.clone(), phase.energy.clone()
    if split:  # the callbacks on the predictors' outputs, then their projections
        pitch, energy = pitch_fn(pitch), energy_fn(energy)
    phase = phase._replace(dur=dur, pitch=pitch, energy=energy)
    if split:
        finish(phase)
    t_ready.synchronize()
    return phase._replace(t_mel=int(t_host)), ent


def _nothing() -> None:
    pass


def phoneme_phase(model, phase_fn, finish, policy, x, alpha, pitch_fn, energy_fn, batch=None,
                  graph=True):
    """One phoneme phase of `model`: from its graph where `graph` allows one (and x is no
    shard of a larger batch), else eager.  phase_fn(x, alpha, pitch_fn, energy_fn, batch,
    capture) is the model's phase, returning a Phase; finish and policy as in `replay`.
    Returns (Phase, consumed): call consumed() on the decoder's stream once everything that
    reads phase.h / phase.offsets is queued (the next replay of a graph waits for it)."""
    r = None
    if graph and batch is None:
        r = replay(model, phase_fn, finish, policy, x, alpha, pitch_fn, energy_fn)
    if r is None:
        return phase_fn(x, alpha, pitch_fn, energy_fn, batch), _nothing
    phase, ent = r
    return phase, lambda: ent['done'].record(torch.cuda.current_stream(x.device))
