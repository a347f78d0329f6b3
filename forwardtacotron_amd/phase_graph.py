"""The phoneme phase of `generate()` as a HIP graph — one protocol for every model.

A model's phoneme phase (predictors, prenet, duration counts) is tens to hundreds of
launches from Python over four streams; as a graph it is one replay, which matters where
the kernels are short (batch 1: the host issue rate, not the device, sets the phase's
length).  `replay` holds what ForwardTacotron and FastPitch share; a model brings its key
part, its capture function and the eager finish of a split graph.

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
caller); everything else in the phase tuple is consumed by this call's decoder — the next
replay waits for the decoder's completion event (generate() records entry['done']), so
calls on different streams never overwrite buffers a decoder still reads.

An entry keeps every weight pack of the model alive (common_layers.held_packs: the
captured kernels point into them) and the model-wide weights key of its capture: after
each replay (while it runs) the key is compared with the model's, and on a change
(load_state_dict, .to(), in-place updates) every captured phase is dropped and the call
falls back to the eager phase (the stale replay read the old, still-held packs; its
outputs are discarded).
"""
from __future__ import annotations

from typing import Callable

import torch

from .common_layers import held_packs, weights_key

CACHE = 8  # captured phases kept per model (least recently used dropped)
TMAX = 5   # a phase tuple is (dur, pitch, energy, ..., T_mel at TMAX, ...)


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


def replay(model, x, alpha, pitch_fn, energy_fn, policy, capture, finish):
    """One phoneme phase of `model` from its captured graph (see the module docstring).
    capture(sx, pitch_fn, energy_fn): the model's phase on the static input sx without a
    host sync, returning the eager phase's tuple with max(totals) on the device at TMAX
    (pitch_fn = energy_fn = None: the split graph — raw predictor outputs, their
    projections not added).  finish(phase): the launch a split graph leaves out, on the
    phase tuple that holds the callbacks' results.  Returns (phase tuple with T_mel read to
    the host, entry) or None (run the eager phase)."""
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
            capture(sx, *cap)  # warm-up
            torch.cuda.synchronize(x.device)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                outs = capture(sx, *cap)
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
    phase = list(ent['outs'])
    t_host = torch.empty((), dtype=phase[TMAX].dtype, pin_memory=True)
    t_host.copy_(phase[TMAX], non_blocking=True)
    t_ready = torch.cuda.Event()
    t_ready.record(main)
    phase[:3] = [t.clone() for t in phase[:3]]
    if split:  # the callbacks on the predictors' outputs, then their projections
        phase[1], phase[2] = pitch_fn(phase[1]), energy_fn(phase[2])
        finish(phase)
    t_ready.synchronize()
    phase[TMAX] = int(t_host)
    return phase, ent
