"""Validation losses and checkpoint evaluation on the HIP path: the step the reference runs
after every epoch to pick a checkpoint (`trainer/forward_trainer.py:146-171`,
`trainer/taco_trainer.py:120-135`, `trainer/voc_trainer.py:142-158` and the generated-versus-target
mel distance of `:188-193`), with the losses they call (`trainer/common.py:69-78` MaskedL1,
F.l1_loss, F.cross_entropy, `utils/distribution.py:16-84` discretized_mix_logistic_loss).

Every loss is one entry point of csrc/eval.hip: fp64 sums in a fixed order, rounded to fp32 once,
so a checkpoint's score repeats bit for bit.  The functions take HIP tensors only; there is no CPU
fallback.  Evaluation is inference: nothing here has a backward pass.
"""
from __future__ import annotations

import math
from typing import Dict, Iterable, Optional, Tuple

import torch

from . import align, ops
from .gta import to_device

_f32 = torch.float32
_INT32_MAX = 2 ** 31 - 1


def _need(t, name: str, dtypes: str = '') -> None:
    """A tensor of the named kind ('fp32', 'int', 'fp32 or int').  The types of all arguments are
    judged before _hip looks at where they live, so a wrong dtype is a TypeError on any device."""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f'{name} must be a tensor')
    is_int = not (t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool)
    if dtypes and not (('fp32' in dtypes and t.dtype == _f32) or ('int' in dtypes and is_int)):
        raise TypeError(f'{name} must be {dtypes}, got {t.dtype}')


def _hip(*ts) -> None:
    for t in ts:
        if not t.is_cuda:
            raise RuntimeError('forwardtacotron_amd.evaluate runs on a HIP device only (got a CPU '
                               'tensor); there is no CPU fallback')


def _values(t: torch.Tensor, name: str) -> torch.Tensor:
    """fp32 as it is; an integer tensor (the collate's int64 durations) converted on the device,
    refused where a magnitude of 2^24 or more would not survive fp32."""
    if t.dtype == _f32:
        return t
    if t.numel() and int(t.abs().max()) >= 2 ** 24:
        raise ValueError(f'{name} holds an integer of magnitude >= 2^24, which fp32 cannot represent')
    return t.to(_f32)


def _lens(lens, B: int, device) -> torch.Tensor:
    """Lengths as int32 [B] on the device, converted there (the kernel clamps them into [0, L])."""
    _need(lens, 'lens', 'int')
    _hip(lens)
    if lens.shape != (B,):
        raise ValueError(f'lens must hold {B} value(s), got shape {tuple(lens.shape)}')
    if lens.dtype != torch.int32:
        lens = lens.clamp(-1, _INT32_MAX).to(torch.int32)
    return lens.contiguous()


def _l1(x, target, lens, out=None) -> torch.Tensor:
    _need(x, 'x', 'fp32')
    _need(target, 'target', 'fp32 or int')
    _hip(x, target)
    if x.dim() != 3 or x.shape != target.shape:
        raise ValueError(f'x and target must be (B, C, L) tensors of one shape, got {tuple(x.shape)} '
                         f'and {tuple(target.shape)}')
    target = _values(target, 'target')
    return ops.l1_loss(x, target, None if lens is None else _lens(lens, x.size(0), x.device), out)


def masked_l1(x: torch.Tensor, target: torch.Tensor, lens: torch.Tensor,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`trainer/common.py:69-78`: x, target (B, C, L), lens [B] -> the sum of |x - target| over
    the frames t < lens[b], divided by C * sum(min(lens, L)), as a 0-d fp32 device tensor.
    Unlike the reference's 0/1 mask, frames at t >= lens[b] are not read at all: a NaN in the
    padding does not reach the result.  All lengths 0 gives NaN, the reference's 0/0."""
    if lens is None:
        raise ValueError('masked_l1 needs lens; l1 is the unmasked mean')
    return _l1(x, target, lens, out)


def l1(x: torch.Tensor, target: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """F.l1_loss of two tensors of one shape (any rank up to (B, C, L)): 0-d fp32 on the device."""
    _need(x, 'x', 'fp32')
    _need(target, 'target', 'fp32 or int')
    _hip(x, target)
    if x.shape != target.shape or not 1 <= x.dim() <= 3:
        raise ValueError(f'x and target must agree in shape, with 1 to 3 dimensions, got '
                         f'{tuple(x.shape)} and {tuple(target.shape)}')
    while x.dim() < 3:
        x, target = x.unsqueeze(0), target.unsqueeze(0)
    return _l1(x, target, None, out)


def cross_entropy(logits: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """F.cross_entropy with class axis 1: logits (N, C) with target (N,), or (N, C, d1, ...) with
    target (N, d1, ...), integer labels -> the mean over all positions, 0-d fp32 on the device.
    A label outside [0, C) raises ValueError (read back together with the loss)."""
    _need(logits, 'logits', 'fp32')
    _need(target, 'target', 'int')
    _hip(logits, target)
    if logits.dim() < 2 or target.shape != logits.shape[:1] + logits.shape[2:]:
        raise ValueError(f'logits (N, C, ...) need target (N, ...), got {tuple(logits.shape)} and '
                         f'{tuple(target.shape)}')
    C = logits.size(1)
    rows = logits.movedim(1, -1)
    rows = rows.reshape(-1, C)  # a view when the class axis already has unit stride
    if C > 1 and rows.stride(1) != 1:
        rows = rows.contiguous()
    tgt = target.reshape(-1)
    if tgt.dtype != torch.int32:
        tgt = tgt.clamp(-1, _INT32_MAX).to(torch.int32)  # out of range stays out of range
    loss, bad = ops.cross_entropy(rows, tgt.contiguous())
    n_bad = int(bad)
    if n_bad:
        raise ValueError(f'{n_bad} label(s) outside [0, {C})')
    return loss


def discretized_mix_logistic_loss(y_hat: torch.Tensor, y: torch.Tensor, num_classes: int = 65536,
                                  log_scale_min: Optional[float] = None,
                                  reduce: bool = True) -> torch.Tensor:
    """`utils/distribution.py:16-84`: y_hat (B, L, 3 K) mixture parameters, y (B, L, 1) samples
    in [-1, 1] -> the negative mean log-likelihood as a 0-d fp32 device tensor, or with
    reduce=False the per-sample values (B, L, 1)."""
    _need(y_hat, 'y_hat', 'fp32')
    _need(y, 'y', 'fp32')
    _hip(y_hat, y)
    if log_scale_min is None:
        log_scale_min = float(math.log(1e-14))
    if y_hat.dim() != 3 or y_hat.size(2) % 3 != 0 or 0 in y_hat.shape:
        raise ValueError(f'y_hat must be (B, L, 3 K), got {tuple(y_hat.shape)}')
    B, L, C = y_hat.shape
    if y.shape != (B, L, 1):
        raise ValueError(f'y must be ({B}, {L}, 1), got {tuple(y.shape)}')
    rows = y_hat.reshape(B * L, C)
    if C > 1 and rows.stride(1) != 1:
        rows = rows.contiguous()
    loss, ps = ops.mol_loss(rows, y.reshape(B * L).contiguous(), num_classes, log_scale_min,
                            per_sample=not reduce)
    return loss if reduce else ps.view(B, L, 1)


def _batches(val_set):
    batches = val_set if hasattr(val_set, '__len__') else list(val_set)
    if len(batches) == 0:
        raise ValueError('val_set is empty')
    return batches


def _host_sum(rows) -> float:
    """The reference's `total += loss.item()`: Python floats added in batch order."""
    total = 0
    for v in rows:
        total += v
    return total


def evaluate_forward(model, val_set: Iterable[Dict[str, object]]) -> Dict[str, object]:
    """`trainer/forward_trainer.py:146-171` for ForwardTacotron and FastPitch: the teacher-forced
    pass over every collated batch (gta.collate_tts) and four masked L1 losses, averaged over
    the batches.  mel_loss (mel + mel_post) and dur_loss are floats; pitch_loss and energy_loss
    are 0-d tensors on the model's device, as in the reference.  The per-batch losses stay on
    the device until one copy after the last batch."""
    model.eval()
    device = next(model.parameters()).device
    batches = _batches(val_set)
    n = len(batches)
    losses = torch.empty(n, 5, device=device, dtype=_f32)
    for i, batch in enumerate(batches):
        batch = to_device(batch, device)
        with torch.no_grad():
            pred = model(batch)
            masked_l1(pred['mel'], batch['mel'], batch['mel_len'], losses[i, 0])
            masked_l1(pred['mel_post'], batch['mel'], batch['mel_len'], losses[i, 1])
            masked_l1(pred['dur'].unsqueeze(1), batch['dur'].unsqueeze(1), batch['x_len'], losses[i, 2])
            masked_l1(pred['pitch'], batch['pitch'].unsqueeze(1), batch['x_len'], losses[i, 3])
            masked_l1(pred['energy'], batch['energy'].unsqueeze(1), batch['x_len'], losses[i, 4])
    host = losses.cpu().tolist()
    pitch = energy = 0  # the reference adds these as fp32 device tensors, in batch order
    for i in range(n):
        pitch = pitch + losses[i, 3]
        energy = energy + losses[i, 4]
    return {'mel_loss': _host_sum(r[0] + r[1] for r in host) / n,
            'dur_loss': _host_sum(r[2] for r in host) / n,
            'pitch_loss': pitch / n, 'energy_loss': energy / n}


def evaluate_tacotron(model, val_set: Iterable[Dict[str, object]]) -> Tuple[float, float]:
    """`trainer/taco_trainer.py:120-135`: (val_loss, val_att_score), the batch average of
    l1(m1_hat, mel) + l1(m2_hat, mel) and of the mean attention sharpness."""
    model.eval()
    device = next(model.parameters()).device
    batches = _batches(val_set)
    n = len(batches)
    losses = torch.empty(n, 3, device=device, dtype=_f32)
    for i, batch in enumerate(batches):
        batch = to_device(batch, device)
        with torch.no_grad():
            m1_hat, m2_hat, attention = model(batch['x'], batch['mel'])
            l1(m1_hat, batch['mel'], losses[i, 0])
            l1(m2_hat, batch['mel'], losses[i, 1])
            _, sharp = align.attention_score(attention, batch['mel_len'])
            losses[i, 2] = torch.mean(sharp)
    host = losses.cpu().tolist()
    return _host_sum(r[0] + r[1] for r in host) / n, _host_sum(r[2] for r in host) / n


def evaluate_wavernn(model, val_set: Iterable[Dict[str, object]]) -> float:
    """`trainer/voc_trainer.py:142-158`: the batch average of the teacher-forced loss, the
    cross-entropy of the logits in RAW mode and the mixture-of-logistics loss in MOL mode.
    Batches hold 'x' (B, L) input samples, 'y' (B, L) labels (RAW) or samples (MOL), 'mel'."""
    model.eval()
    device = next(model.parameters()).device
    if model.mode not in ('RAW', 'MOL'):
        raise RuntimeError(f'Unknown model mode value - {model.mode}')
    batches = _batches(val_set)
    n = len(batches)
    losses = torch.empty(n, device=device, dtype=_f32)
    for i, batch in enumerate(batches):
        batch = to_device(batch, device)
        x, y, m = batch['x'], batch['y'], batch['mel']
        with torch.no_grad():
            y_hat = model(x, m)
            if model.mode == 'RAW':
                # F.cross_entropy(y_hat.transpose(1, 2).unsqueeze(-1), y.unsqueeze(-1))
                losses[i] = cross_entropy(y_hat.transpose(1, 2).unsqueeze(-1), y.unsqueeze(-1))
            else:
                losses[i] = discretized_mix_logistic_loss(y_hat, y.float().unsqueeze(-1))
    return _host_sum(losses.cpu().tolist()) / n


def mel_l1(dsp, wav_a: torch.Tensor, wav_b: torch.Tensor) -> float:
    """The metric that ranks WaveRNN checkpoints (`trainer/voc_trainer.py:188-193`): the L1
    distance between the un-normalised mel spectrograms of two signals (L,) of one length, both
    computed on the device."""
    _need(wav_a, 'wav_a', 'fp32')
    _need(wav_b, 'wav_b', 'fp32')
    _hip(wav_a, wav_b)
    if wav_a.dim() != 1 or wav_a.shape != wav_b.shape:
        raise ValueError(f'two signals (L,) of one length expected, got {tuple(wav_a.shape)} and '
                         f'{tuple(wav_b.shape)}')
    mel_a = dsp.wav_to_mel(wav_a, normalize=False)
    mel_b = dsp.wav_to_mel(wav_b, normalize=False)
    return float(l1(mel_a, mel_b))
