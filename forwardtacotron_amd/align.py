"""Attention scores, duration extraction and phoneme-level pitch / energy on the HIP path: the
step between Tacotron's teacher-forced pass and ForwardTacotron / FastPitch training
(`train_tacotron.py:23-175`: normalize_values, extract_pitch_energy, create_align_features;
`utils/metrics.py`, attention_score; `utils/duration_extraction.py`,
extract_durations_with_dijkstra / extract_durations_per_count).

The attention stays on the device: scores and durations are each one launch over the whole
batch (csrc/align.hip).  The Dijkstra extraction is the reference's grid graph solved as a
three-predecessor fp64 dynamic programme; its path cost equals scipy's distance bit for bit
and its path equals scipy's wherever the shortest path is unique ("Alignment").
The phoneme means are one more launch over the batch, fp64 sums rounded to fp32 once; the data
set's pitch mean / std and the normalisation run on the device as well.
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


def _features_device(t: torch.Tensor, name: str, dims: Tuple[int, ...], dtype) -> None:
    if not isinstance(t, torch.Tensor) or t.dim() not in dims:
        raise ValueError(f'{name} must be a tensor with {" or ".join(map(str, dims))} dimensions')
    if not t.is_cuda:
        raise RuntimeError('forwardtacotron_amd.align runs on a HIP device only (got a CPU '
                           'tensor); there is no CPU fallback')
    if t.dtype != dtype:
        raise TypeError(f'{name} must be {dtype}, got {t.dtype}')


def phoneme_pitch_energy(mel: torch.Tensor, mel_len, dur: torch.Tensor, x_len=None,
                         pitch: Optional[torch.Tensor] = None, pitch_len=None,
                         pitch_max_freq: float = 600.0):
    """The per-utterance part of `train_tacotron.py:57-86`: phoneme-wide means of the frame
    energy ‖exp(mel[:, t])‖₂ and of the voiced raw pitch (v != 0 and v < pitch_max_freq) over
    each token's duration.  mel (B, n_mels, rows) fp32 log-mel on the device, mel_len [B] in
    [1, rows], dur (B, T) int32 with sum(dur[b, :x_len[b]]) == mel_len[b] (else ValueError
    naming the items, the reference's assert), x_len [B] in [1, T] (None: T), pitch (B, P) fp32
    with pitch_len [B] in [0, P] (None: P), or no pitch at all
    -> (pitch_char, energy_char), fp32 (B, T) on the device; pitch_char is None without pitch.
    Like the reference's loop, tokens from mel_len on keep 0.  One item as (n_mels, rows), (T,)
    and (P,) with scalar lengths returns (T,) vectors.  One launch over the batch."""
    _features_device(mel, 'mel', (2, 3), torch.float32)
    single = mel.dim() == 2
    _features_device(dur, 'dur', (1,) if single else (2,), torch.int32)
    if pitch is not None:
        _features_device(pitch, 'pitch', (1,) if single else (2,), torch.float32)
    elif pitch_len is not None:
        raise ValueError('pitch_len without pitch')
    if single:
        mel, dur, pitch = mel[None], dur[None], (None if pitch is None else pitch[None])
    B, n_mels, rows = mel.shape
    T = dur.size(1) if dur.size(0) == B else 0
    if not 1 <= T <= ops.TACO_MAX_TOKENS:
        raise ValueError(f'the alignment kernels take 1..{ops.TACO_MAX_TOKENS} tokens and one dur '
                         f'row per item, got dur {tuple(dur.shape)} for {B} item(s)')
    if mel.size(2) > 1 and mel.stride(2) != 1 or mel.size(1) > 1 and mel.stride(1) < rows:
        mel = mel.contiguous()
    if T > 1 and dur.stride(1) != 1 or B > 1 and dur.stride(0) < T:
        dur = dur.contiguous()
    ml = _lengths(mel_len, B, rows, 'mel_len', mel.device)
    xl = None if x_len is None else _lengths(x_len, B, T, 'x_len', mel.device)
    pl = None
    if pitch is not None:
        if pitch.size(0) != B or pitch.size(1) < 1:
            raise ValueError(f'pitch must hold one non-empty row per item, got {tuple(pitch.shape)}')
        P = pitch.size(1)
        if P > 1 and pitch.stride(1) != 1 or B > 1 and pitch.stride(0) < P:
            pitch = pitch.contiguous()
        pl = _lengths([P] * B if pitch_len is None else pitch_len, B, P, 'pitch_len', mel.device, lo=0)
    pc, ec, dsum = ops.phoneme_features(mel, ml, dur, xl, pitch, pl, float(pitch_max_freq))
    bad = torch.nonzero(dsum != ml).flatten().tolist()  # the one host synchronisation
    if bad:
        raise ValueError(f'sum of durations does not match mel_len for item(s) {bad}: '
                         f'{dsum[bad].tolist()} vs {ml[bad].tolist()}')
    if single:
        pc, ec = (None if pc is None else pc[0]), ec[0]
    return pc, ec


def normalize_values(values) -> Tuple[float, float]:
    """`train_tacotron.py:23-32` on the device, in place: the mean and population std over the
    non-zero entries of `values` (one fp32 device tensor or a list of them), then every
    non-zero entry becomes (v - mean) / std in fp32 and zeros stay 0.  Returns (mean, std) as
    the fp32 values the normalisation used: the fp64 moments rounded once.  ValueError when no
    entry is non-zero (the reference would write NaNs)."""
    vs = [values] if isinstance(values, torch.Tensor) else list(values)
    if not vs:
        raise ValueError('normalize_values: nothing to normalise')
    for v in vs:
        _features_device(v, 'values', tuple(range(1, 9)), torch.float32)
        if not v.is_contiguous():
            raise ValueError('normalize_values works in place and takes contiguous tensors')
    vs = [v for v in vs if v.numel()]
    if not vs:
        raise ValueError('normalize_values: no non-zero value')
    flat = vs[0].reshape(-1) if len(vs) == 1 else torch.cat([v.reshape(-1) for v in vs])
    cnt, mean, std = ops.nonzero_moments(flat).tolist()
    if cnt == 0:
        raise ValueError('normalize_values: no non-zero value')
    mean, std = float(np.float32(mean)), float(np.float32(std))
    for v in vs:
        ops.normalize_nonzero(v, mean, std)
    return mean, std


def extract_pitch_energy(dataset, alg_path: Union[str, Path], mel_path: Union[str, Path],
                         raw_pitch_path: Union[str, Path], save_path_pitch: Union[str, Path],
                         save_path_energy: Union[str, Path], pitch_max_freq: float,
                         batch_size: int = 32, device='cuda') -> Tuple[float, float]:
    """`train_tacotron.py:37-104` on the HIP path.  dataset: the [(item_id, mel_len)] list of
    train_dataset.pkl + val_dataset.pkl.  Per item {item_id}.npy is read from alg_path
    (durations [T]), mel_path (log-mel (n_mels, L), L >= mel_len) and raw_pitch_path (frame
    pitch [P]); items go to the device padded into batches of batch_size, and every phoneme
    pitch stays there until the data set's mean and std are known.  Writes {item_id}.npy, fp32
    [T], under save_path_energy (as computed) and save_path_pitch (normalised); returns the
    pitch (mean, std)."""
    alg_path, mel_path, raw_pitch_path = Path(alg_path), Path(mel_path), Path(raw_pitch_path)
    save_path_pitch, save_path_energy = Path(save_path_pitch), Path(save_path_energy)
    dataset = list(dataset)
    if not dataset or batch_size < 1:
        raise ValueError('extract_pitch_energy needs a non-empty data set and batch_size >= 1')
    pending = []  # (item ids, token counts, pitch_char (B, T) on the device)
    for k in range(0, len(dataset), batch_size):
        ids, mls = zip(*dataset[k:k + batch_size])
        durs = [np.load(alg_path / f'{i}.npy', allow_pickle=False).astype(np.int32) for i in ids]
        mels = [np.load(mel_path / f'{i}.npy', allow_pickle=False).astype(np.float32) for i in ids]
        pits = [np.load(raw_pitch_path / f'{i}.npy', allow_pickle=False).astype(np.float32) for i in ids]
        for i, m, L in zip(ids, mels, mls):
            if m.ndim != 2 or m.shape[0] != mels[0].shape[0] or m.shape[1] < L:
                raise ValueError(f'{i}: mel {m.shape} does not hold {mels[0].shape[0]} bins x {L} frames')
        B, n_mels = len(ids), mels[0].shape[0]
        mel = np.zeros((B, n_mels, max(mls)), np.float32)
        dur = np.zeros((B, max(len(d) for d in durs)), np.int32)
        pit = np.zeros((B, max(1, max(len(p) for p in pits))), np.float32)
        for j in range(B):
            mel[j, :, :mls[j]] = mels[j][:, :mls[j]]
            dur[j, :len(durs[j])] = durs[j]
            pit[j, :len(pits[j])] = pits[j]
        try:
            pc, ec = phoneme_pitch_energy(
                torch.from_numpy(mel).to(device), list(mls), torch.from_numpy(dur).to(device),
                [len(d) for d in durs], torch.from_numpy(pit).to(device), [len(p) for p in pits],
                pitch_max_freq)
        except ValueError as e:
            raise ValueError(f'items {list(ids)}: {e}') from e
        ec = ec.cpu().numpy()
        for j, i in enumerate(ids):
            np.save(str(save_path_energy / f'{i}.npy'), ec[j, :len(durs[j])], allow_pickle=False)
        pending.append((ids, [len(d) for d in durs], pc))
    mean, std = normalize_values([pc for _, _, pc in pending])
    for ids, ts, pc in pending:
        pc = pc.cpu().numpy()
        for j, i in enumerate(ids):
            np.save(str(save_path_pitch / f'{i}.npy'), pc[j, :ts[j]], allow_pickle=False)
    return mean, std


def create_align_features(model, train_set: Iterable[Dict[str, object]],
                          val_set: Iterable[Dict[str, object]], alg_path: Union[str, Path],
                          data_path: Union[str, Path], dijkstra: bool = True,
                          pitch_max_freq: Optional[float] = None, dataset=None,
                          mel_path: Union[str, Path, None] = None,
                          raw_pitch_path: Union[str, Path, None] = None,
                          phon_pitch_path: Union[str, Path, None] = None,
                          phon_energy_path: Union[str, Path, None] = None,
                          batch_size: int = 32) -> int:
    """`train_tacotron.py:129-175`: the teacher-forced pass over every batch of both sets, then
    scores and durations on the device.  Every item's dur[:x_len] is saved as {item_id}.npy
    (int32) under alg_path, and {item_id: (loc_score, sharp_score)} as att_score_dict.pkl under
    data_path.  Every item of a batch is processed with its own x_len (the reference's loader
    has batch size 1 and it reads item 0 only: identical there).  With pitch_max_freq given
    (then dataset and the four folders are required) it ends like the reference, with
    extract_pitch_energy over `dataset` reading the durations just written; without it no
    pitch or energy file is touched.  Returns the item count."""
    assert model.r == 1, f'Reduction factor of tacotron must be 1 for creating alignment features! ' \
                         f'Reduction factor was: {model.r}'
    features = (dataset, mel_path, raw_pitch_path, phon_pitch_path, phon_energy_path)
    if pitch_max_freq is None:
        if any(v is not None for v in features):
            raise ValueError('the pitch / energy arguments need pitch_max_freq')
    elif any(v is None for v in features):
        raise ValueError('pitch_max_freq needs dataset, mel_path, raw_pitch_path, phon_pitch_path '
                         'and phon_energy_path')
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
    if pitch_max_freq is not None:
        extract_pitch_energy(dataset, alg_path, mel_path, raw_pitch_path, phon_pitch_path,
                             phon_energy_path, pitch_max_freq, batch_size=batch_size, device=device)
    return n
