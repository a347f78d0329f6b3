"""Attention scores and duration extraction on the HIP path: the step between Tacotron's
teacher-forced pass and ForwardTacotron / FastPitch training (`train_tacotron.py:129-171`,
create_align_features; `utils/metrics.py`, attention_score; `utils/duration_extraction.py`,
extract_durations_with_dijkstra / extract_durations_per_count).

The attention stays on the device: scores and durations are each one launch over the whole
batch (csrc/align.hip).  The Dijkstra extraction is the reference's grid graph solved as a
three-predecessor fp64 dynamic programme; its path cost equals scipy's distance bit for bit
and its path equals scipy's wherever the shortest path is unique ("Alignment").
"""
from __future__ import annotations

import itertools
import pickle
from pathlib import Path
from typing import Dict, Iterable, Optional, Tuple, Union

import numpy as np
import torch

from . import ops
from .gta import to_device

METHODS = ('dijkstra', 'count')


def _lengths(v, B: int, hi: int, name: str, device, lo: int = 1) -> torch.Tensor:
    """v (int, sequence or tensor) as a validated int32 [B] tensor on `device`: every value
    in [lo, hi], else ValueError (checked on the host before any launch)."""
    t = torch.as_tensor(v).detach().cpu().reshape(-1)
    if t.dtype.is_floating_point or t.dtype == torch.bool:
        raise ValueError(f'{name} must hold integers, got {t.dtype}')
    if t.numel() != B:
        raise ValueError(f'{name} must hold {B} value(s), got {t.numel()}')
    if int(t.min()) < lo or int(t.max()) > hi:
        raise ValueError(f'{name} must lie in [{lo}, {hi}], got {t.tolist()}')
    return t.to(torch.int32).to(device)


def _att3(att: torch.Tensor) -> Tuple[torch.Tensor, bool]:
    if not isinstance(att, torch.Tensor) or att.dim() not in (2, 3):
        raise ValueError('att must be a (B, rows, T) or (rows, T) tensor')
    if not att.is_cuda:
        raise RuntimeError('forwardtacotron_amd.align runs on a HIP device only (got a CPU '
                           'tensor); there is no CPU fallback')
    if att.dtype != torch.float32:
        raise TypeError(f'att must be fp32, got {att.dtype}')
    single = att.dim() == 2
    att = att.unsqueeze(0) if single else att
    if att.size(2) > 1 and att.stride(2) != 1 or att.size(1) > 1 and att.stride(1) < att.size(2):
        att = att.contiguous()
    return att, single


def attention_score(att: torch.Tensor, mel_lens, r: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
    """`utils/metrics.py:4-31`: att (B, rows, T), mel_lens [B] -> (loc_score, sharp_score),
    fp32 [B] on att's device.  loc_score: the share of the first mel_len // r decoder steps
    whose attention peak moved by at most r tokens; sharp_score: the mean peak height, the
    masked sum divided by the padded length `rows` like the reference's torch.mean."""
    att, single = _att3(att)
    if single:
        raise ValueError('attention_score takes a batch (B, rows, T), like the reference')
    if int(r) < 1:
        raise ValueError(f'r must be >= 1, got {r}')
    B = att.size(0)
    ml = _lengths(mel_lens, B, 2 ** 31 - 1, 'mel_lens', att.device)
    return ops.attention_score(att, ml, int(r))


def extract_durations(att: torch.Tensor, mel_len, x_len=None, method: str = 'dijkstra',
                      return_cost: bool = False):
    """Durations per token from an attention matrix.  att (B, rows, T) fp32 on the device,
    mel_len [B] in [1, rows], x_len [B] in [1, T] (None: T) -> int32 (B, T) with
    sum(dur[b]) == mel_len[b] and zeros from x_len[b] on.  One item as (rows, T) with scalar
    lengths returns (T,), like the reference functions.

    method 'dijkstra': `extract_durations_with_dijkstra` over att[:mel_len, :x_len];
    'count': `extract_durations_per_count`.  return_cost (dijkstra only): also the path
    costs, float64 [B] — scipy's dist_matrix[-1]."""
    if method not in METHODS:
        raise ValueError(f'method must be one of {METHODS}, got {method!r}')
    if return_cost and method != 'dijkstra':
        raise ValueError("return_cost needs method='dijkstra'")
    att, single = _att3(att)
    B, rows, T = att.shape
    if not 1 <= T <= ops.TACO_MAX_TOKENS:
        raise ValueError(f'the alignment kernels take 1..{ops.TACO_MAX_TOKENS} tokens, got {T}')
    ml = _lengths(mel_len, B, rows, 'mel_len', att.device)
    xl = None if x_len is None else _lengths(x_len, B, T, 'x_len', att.device)
    if method == 'dijkstra':
        dur, cost = ops.align_dijkstra(att, ml, xl, want_cost=return_cost)
    else:
        dur, cost = ops.align_count(att, ml, xl), None
    if single:
        dur, cost = dur[0], (None if cost is None else cost[0])
    return (dur, cost) if return_cost else dur


def create_align_features(model, train_set: Iterable[Dict[str, object]],
                          val_set: Iterable[Dict[str, object]], alg_path: Union[str, Path],
                          data_path: Union[str, Path], dijkstra: bool = True) -> int:
    """`train_tacotron.py:129-171` without the pitch / energy averaging: the teacher-forced
    pass over every batch of both sets, then scores and durations on the device.  Every
    item's dur[:x_len] is saved as {item_id}.npy (int32) under alg_path, and
    {item_id: (loc_score, sharp_score)} as att_score_dict.pkl under data_path.  Every item
    of a batch is processed with its own x_len (the reference's loader has batch size 1 and
    it reads item 0 only: identical there).  Returns the item count."""
    assert model.r == 1, f'Reduction factor of tacotron must be 1 for creating alignment features! ' \
                         f'Reduction factor was: {model.r}'
    model.eval()
    device = next(model.parameters()).device
    alg_path, data_path = Path(alg_path), Path(data_path)
    att_score_dict = {}
    method = 'dijkstra' if dijkstra else 'count'
    n = 0
    for batch in itertools.chain(train_set, val_set):
        batch = to_device(batch, device)
        with torch.no_grad():
            _, _, att = model(batch['x'], batch['mel'])
        loc, sharp = attention_score(att, batch['mel_len'], r=1)
        dur = extract_durations(att, batch['mel_len'], batch['x_len'], method=method)
        loc, sharp, dur = loc.cpu().numpy(), sharp.cpu().numpy(), dur.cpu().numpy()
        for j, item_id in enumerate(batch['item_id']):
            att_score_dict[item_id] = (float(loc[j]), float(sharp[j]))
            np.save(str(alg_path / f'{item_id}.npy'), dur[j, :int(batch['x_len'][j])],
                    allow_pickle=False)
            n += 1
    with open(data_path / 'att_score_dict.pkl', 'wb') as f:
        pickle.dump(att_score_dict, f, protocol=pickle.HIGHEST_PROTOCOL)
    return n
