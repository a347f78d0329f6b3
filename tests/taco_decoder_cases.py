"""Decoder-level cases for the Tacotron decoder launch (csrc/tacotron.hip) — test
infrastructure only, no tests in here.

The model-level goldens (tests/test_gpu_tacotron.py) stop at 70 tokens and r = 5 and run the
f16x3 encoder and postnet around the decoder.  The cases here hand the decoder launch and the
CPU oracle (tests/taco_torch_cpu.py `decoder_step`, pinned to the reference by
tests/test_oracle_tacotron.py) the SAME fp32 encoder rows, so the comparison isolates the
decoder, at the sizes its code takes other paths: tokens 256..511 (a workgroup's second
token), r up to 20 (1600 live mel_proj rows, seven per workgroup), the attention peak on the
location window's edges and on tokens 0 / 255 / 256 / T-1, and a stop rule that a single value
of the step's r frames decides.

Inputs: enc = tanh(N(0, 1)), enc_proj = enc @ encoder_proj.weight^T once in fp32 on the CPU,
teacher frames 3 N(0, 1) - 4.  Weights: the synthetic `decoder.*` tensors.

Bounds: drift = max |oracle fp32 - oracle fp64| on the case; |d mel| <= max(1e-4, 10 drift),
|d attn| <= max(1e-5, 10 drift) — the convention tests/test_gpu_tacotron.py takes from the
goldens, measured on the reference arithmetic, never on the kernel.

Planted defects (oracle only, tests/test_tacotron_decoder_cases.py): DEFECTS below.
"""
from __future__ import annotations

import contextlib
import functools
import json
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

import taco_torch_cpu as TC

GOLDEN = Path(__file__).resolve().parent / 'golden'
N_MELS, MAX_R, D = 80, TC.MAX_R, 256
NEVER, ALWAYS = -1e9, 1e9  # stop thresholds: nothing is below / everything is below

# name: mode, B, T, r, frames (forced: teacher frames; free: the `steps` argument), seed,
# peaks (per item: the token the step-0 argmax is rolled onto, None = as drawn), thr (free)
CASES = {
    'forced_t512_r20': dict(mode='forced', B=2, T=512, r=20, frames=80, seed=1, peaks=(511, 256)),
    'forced_t257_r7': dict(mode='forced', B=2, T=257, r=7, frames=40, seed=2, peaks=(256, 0)),
    'forced_t256_r13': dict(mode='forced', B=2, T=256, r=13, frames=39, seed=3, peaks=(255, 255)),
    'forced_t255_r3': dict(mode='forced', B=1, T=255, r=3, frames=20, seed=4, peaks=(254,)),
    # item 0 on the window's left edge for 12 steps (cum grows there); item 1 on the right edge,
    # which also takes the case's argmax past token 255 (with both items on token 0 no step
    # of this case would leave the first token pass)
    'forced_t300_r3': dict(mode='forced', B=2, T=300, r=3, frames=36, seed=5, peaks=(0, 299)),
    'forced_t1_r3': dict(mode='forced', B=1, T=1, r=3, frames=12, seed=6, peaks=None),
    'forced_t2_r1': dict(mode='forced', B=2, T=2, r=1, frames=6, seed=7, peaks=(1, 1)),
    'forced_t31_r2': dict(mode='forced', B=1, T=31, r=2, frames=10, seed=8, peaks=(15,)),
    'free_t512_r1': dict(mode='free', B=1, T=512, r=1, frames=30, seed=9, peaks=(300,), thr=NEVER),
    'free_t384_r20': dict(mode='free', B=1, T=384, r=20, frames=60, seed=10, peaks=(383,), thr=NEVER),
    'stop_r10': dict(mode='free', B=1, T=40, r=10, frames=200, seed=11, peaks=None, thr=ALWAYS,
                     want=(30, 3)),
    'stop_r11': dict(mode='free', B=1, T=40, r=11, frames=200, seed=12, peaks=None, thr=ALWAYS,
                     want=(22, 2)),
    'stop_r20': dict(mode='free', B=1, T=40, r=20, frames=200, seed=13, peaks=None, thr=ALWAYS,
                     want=(40, 2)),
    # "single loud value": mel_proj row (mel 79, j = r - 2), i.e. live row a = n_live - 2,
    # scaled in this case's copy of the weights; seed, scale and thr found by
    # `search_loud()` on the fp64 oracle and fixed here.
    # The scaled value of steps 0..6 is 12.4, 20.2, 25.5, 27.5, 28.2, 24.6, 12.3 and the
    # largest other value 19.95: steps 4 and 5 (t = 12, 15) stay loud through it alone, step 6
    # stops (21 frames, 7 attention rows).  The scale multiplies the row's fp32 drift into the
    # case's mel bound, so the table takes the smallest scale the search found (every margin
    # is 1.8 or more).
    'stop_loud_r3': dict(mode='free', B=1, T=40, r=3, frames=150, seed=108, peaks=None,
                         thr=22.0, loud=dict(mel=79, scale=2.0), want=(21, 7)),
}
LOUD_MARGIN = 1e-2

DEFECTS = {
    'a': 'tokens >= 256 read the enc_proj row of token - 256',
    'b': 'the location-conv output shifted by one token',
    'c': 'the location input padded by wrap-around instead of zeros',
    'd': 'cum not accumulated: the window sees att twice',
    'e': 'live row a taken as j*80 + mel instead of mel*r + j (the fed-back frame is picked '
         'from the gathered rows by mel*r + r-1)',
    'f': 'live rows a >= 1024 returned as zero',
    'g': 'the stop test looks only at the last of the r frames',
    'h': 'the stop test is t >= 10',
}


@functools.lru_cache(maxsize=None)
def _decoder_arrays():
    from forwardtacotron_amd.synthetic import synthetic_array
    keys = json.loads((GOLDEN / 'tacotron_state_dict_keys.json').read_text())
    return {k: synthetic_array(k, shape, dt, 0, 'tacotron') for k, shape, dt in keys
            if k.startswith('decoder.') or k == 'encoder_proj.weight'}


@functools.lru_cache(maxsize=8)
def decoder_sd(dtype=torch.float32, loud=None):
    """{key: tensor} of the `decoder.*` tensors and encoder_proj.weight, shared and read-only.
    loud = (mel, scale, r): mel_proj row mel*20 + r-2 scaled IN FP32 (what the device gets),
    then cast."""
    sd = {k: torch.from_numpy(v.copy()) for k, v in _decoder_arrays().items()}
    if loud is not None:
        sd['decoder.mel_proj.weight'][loud_row(loud)] *= loud[1]
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


def loud_row(loud):
    mel, _, r = loud
    return mel * MAX_R + r - 2


def _loud(c):
    return (c['loud']['mel'], c['loud']['scale'], c['r']) if c.get('loud') else None


class Case:
    """The fp32 inputs both sides receive: enc (B, T, 256), enc_proj, and (forced) the teacher
    frames m (B, 80, frames) with prenet_in (B, n, 80) as Tacotron._forward prepares it."""

    def __init__(self, name):
        c = CASES[name]
        self.name, self.cfg = name, c
        self.mode, self.B, self.T, self.r, self.frames = c['mode'], c['B'], c['T'], c['r'], c['frames']
        self.n = (self.frames + self.r - 1) // self.r
        self.thr = c.get('thr')
        self.loud = _loud(c)
        g = torch.Generator().manual_seed(1000 + c['seed'])
        enc = torch.tanh(torch.randn(self.B, self.T, D, generator=g))
        enc_proj = F.linear(enc, decoder_sd()['encoder_proj.weight'])
        self.m = self.prenet_in = None
        if self.mode == 'forced':
            self.m = 3.0 * torch.randn(self.B, N_MELS, self.frames, generator=g) - 4.0
            self.prenet_in = prenet_in_of(self.m, self.r)
        if c['peaks'] is not None:
            enc, enc_proj = place_peak(enc, enc_proj, c['peaks'])
        self.enc, self.enc_proj = enc.contiguous(), enc_proj.contiguous()

    def sd(self, dtype):
        return decoder_sd(dtype, self.loud)


def prenet_in_of(m, r):
    """Tacotron._forward: the frame fed to step s is m[:, :, s r - 1], the zero <GO> frame for
    s = 0.  m (B, 80, F) -> (B, n, 80)."""
    B, _, Fr = m.shape
    n = (Fr + r - 1) // r
    m_cl = m.transpose(1, 2).float()
    out = torch.zeros(B, n, N_MELS)
    if n > 1:
        out[:, 1:] = m_cl[:, r - 1:(n - 1) * r:r]
    return out


def step0_attention(enc, enc_proj, dtype=torch.float64):
    """The step-0 attention weights (B, T): cum = att = ctx = 0 and the <GO> frame, so they
    depend on each token's own enc_proj row only."""
    sd = decoder_sd(dtype)
    e, ep = enc.to(dtype), enc_proj.to(dtype)
    st = TC.DecoderState(sd, e)
    with torch.no_grad():
        _, att = TC.decoder_step(sd, st, e, ep, torch.zeros(enc.size(0), N_MELS, dtype=dtype), 1)
    return att


def place_peak(enc, enc_proj, peaks):
    """Roll each item's rows along T so that its step-0 argmax sits on token peaks[b]."""
    at = step0_attention(enc, enc_proj).argmax(1)
    enc, enc_proj = enc.clone(), enc_proj.clone()
    for b, p in enumerate(peaks):
        sh = int(p) - int(at[b])
        enc[b], enc_proj[b] = torch.roll(enc[b], sh, 0), torch.roll(enc_proj[b], sh, 0)
    return enc, enc_proj


# ---------------------------------------------------------------------------------------
# planted defects

class _FProxy:
    """torch.nn.functional with conv1d (decoder_step's only one: the location conv) replaced."""

    def __init__(self, conv1d):
        self.conv1d = conv1d

    def __getattr__(self, name):
        return getattr(F, name)


@contextlib.contextmanager
def _location_conv(fn):
    if fn is None:
        yield
        return
    old = TC.F
    TC.F = _FProxy(fn)
    try:
        yield
    finally:
        TC.F = old


def _conv_shifted(loc, w, padding):
    out = F.conv1d(loc, w, padding=padding)
    return F.pad(out, (1, 0))[..., :-1]


def _conv_wrapped(loc, w, padding):
    T = loc.size(-1)
    idx = torch.arange(-padding, T + padding) % T
    return F.conv1d(loc[..., idx], w)


def _conv_att_twice(loc, w, padding):
    return F.conv1d(loc[:, [1, 1]], w, padding=padding)


_CONV_DEFECTS = {'b': _conv_shifted, 'c': _conv_wrapped, 'd': _conv_att_twice}


def _live_index(r):
    return torch.arange(N_MELS).unsqueeze(1) * r + torch.arange(r).unsqueeze(0)  # a = mel r + j


def _frames_out(fr, r, defect):
    if defect == 'f':
        fr = fr.masked_fill(_live_index(r) >= 1024, 0.0)
    return fr


def _last_frame(fr, r, defect):
    """The frame fed back, (B, 80).  Defect e: the gathered rows are laid out j*80 + mel and
    picked at mel*r + r-1."""
    if defect == 'e':
        flat = fr.transpose(1, 2).reshape(fr.size(0), -1)
        return flat[:, torch.arange(N_MELS) * r + r - 1]
    return fr[:, :, -1]


def _enc_proj_used(enc_proj, defect):
    if defect == 'a' and enc_proj.size(1) > 256:
        enc_proj = enc_proj.clone()
        enc_proj[:, 256:] = enc_proj[:, :enc_proj.size(1) - 256]
    return enc_proj


def _pack(mels, attns, extra):
    mel = torch.cat(mels, 2).transpose(1, 2).contiguous()  # (B, n r, 80): the launch's layout
    return dict(mel=mel.double().numpy(), attn=torch.stack(attns, 1).double().numpy(),
                steps=len(attns), **extra)


def run_forced(case, dtype, defect=None):
    """Teacher-forced loop over decoder_step -> dict(mel (B, n r, 80), attn (B, n, T), steps)."""
    sd = case.sd(dtype)
    enc, ep = case.enc.to(dtype), _enc_proj_used(case.enc_proj.to(dtype), defect)
    pin = case.prenet_in.to(dtype)
    st = TC.DecoderState(sd, enc)
    mels, attns = [], []
    with torch.no_grad(), _location_conv(_CONV_DEFECTS.get(defect)):
        for s in range(case.n):
            fr, att = TC.decoder_step(sd, st, enc, ep, pin[:, s], case.r)
            mels.append(_frames_out(fr, case.r, defect))
            attns.append(att)
    return _pack(mels, attns, {})


def run_free(case, dtype, defect=None, thr=None):
    """Free-running loop with the reference's stop rule, (frames < thr).all() and t > 10 with
    t = s r -> dict(mel, attn, steps, trace (steps, 80, r): every step's frames)."""
    thr = case.thr if thr is None else thr
    sd = case.sd(dtype)
    enc, ep = case.enc.to(dtype), _enc_proj_used(case.enc_proj.to(dtype), defect)
    st = TC.DecoderState(sd, enc)
    last = torch.zeros(1, N_MELS, dtype=dtype)
    mels, attns = [], []
    with torch.no_grad(), _location_conv(_CONV_DEFECTS.get(defect)):
        for t in range(0, case.frames, case.r):
            fr, att = TC.decoder_step(sd, st, enc, ep, last, case.r)
            fr = _frames_out(fr, case.r, defect)
            mels.append(fr)
            attns.append(att)
            last = _last_frame(fr, case.r, defect)
            seen = fr[:, :, -1] if defect == 'g' else fr
            if bool((seen < thr).all()) and (t >= 10 if defect == 'h' else t > 10):
                break
    return _pack(mels, attns, dict(trace=torch.cat(mels, 0).double().numpy()))


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


@functools.lru_cache(maxsize=None)
def oracle(name, dtype=torch.float64, defect=None):
    """The oracle's result on a case; computed once per (case, dtype, defect), read-only."""
    c = case(name)
    out = (run_forced if c.mode == 'forced' else run_free)(c, dtype, defect)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def drift(name):
    a, b = oracle(name, torch.float32), oracle(name, torch.float64)
    assert a['steps'] == b['steps'], (name, a['steps'], b['steps'])
    return (float(np.abs(a['mel'] - b['mel']).max()), float(np.abs(a['attn'] - b['attn']).max()))


def bounds(name):
    """(mel bound, attn bound) = (max(1e-4, 10 drift), max(1e-5, 10 drift))."""
    dm, da = drift(name)
    return max(1e-4, 10 * dm), max(1e-5, 10 * da)


def decided_steps(attn, attn_bound):
    """attn (B, n, T) -> bool (B, n): the top two weights differ by more than 10 bounds
    (T = 1: the argmax is decided)."""
    if attn.shape[-1] == 1:
        return np.ones(attn.shape[:2], dtype=bool)
    top = np.sort(attn, -1)
    return (top[..., -1] - top[..., -2]) > 10 * attn_bound


def loud_conditions(name):
    """The "single loud value" conditions on the fp64 oracle -> dict of the figures; raises
    AssertionError where one fails."""
    c = case(name)
    o = oracle(name)
    r, thr = c.r, c.thr
    tr = o['trace']  # (steps, 80, r)
    mel, j = c.loud[0], r - 2
    row = tr[:, mel, j]
    others = tr.copy()
    others[:, mel, j] = -np.inf
    others_margin = float(thr - others.max())
    row_margin = float(np.abs(row - thr).min())
    s_stop = o['steps'] - 1
    late = [s for s in range(o['steps']) if s * r > 10]
    alone = [s for s in late if row[s] >= thr]  # loud only through the scaled value
    assert others_margin >= LOUD_MARGIN, others_margin
    assert row_margin >= LOUD_MARGIN, row_margin
    assert s_stop >= 6 and s_stop * r > 10 and row[s_stop] < thr, (s_stop, row)
    assert late[:len(alone)] == alone and len(alone) >= 1 and s_stop == late[len(alone)], (late, alone)
    assert (s_stop + 1) * r < c.frames  # the rule ended the run, not the step limit
    return dict(steps=o['steps'], others_margin=others_margin, row_margin=row_margin,
                alone=len(alone))


def search_loud(seeds=range(14, 200), scales=(2.0, 3.0, 4.0), mel=79, T=40, r=3, frames=60):
    """The CPU search that fixed stop_loud_r3's seed, scale and thr.  The scaled row is not fed
    back (j = r - 2), so one unscaled run per seed gives every scale's values; thr is the next
    whole number at least 0.5 above every other value; kept where the stop comes at step 6..9
    and the scaled value stays a whole unit away from thr."""
    out = []
    for seed in seeds:
        CASES['_probe'] = dict(mode='free', B=1, T=T, r=r, frames=frames, seed=seed, peaks=None,
                               thr=NEVER, loud=dict(mel=mel, scale=1.0))
        tr = run_free(Case('_probe'), torch.float64)['trace']
        others = tr.copy()
        others[:, mel, r - 2] = -np.inf
        thr = float(np.ceil(others.max() + 0.5))
        late = [s for s in range(len(tr)) if s * r > 10]
        for scale in scales:
            row = tr[:, mel, r - 2] * scale
            below = [s for s in late if row[s] < thr]
            if below and 6 <= below[0] <= 9 and np.abs(row[:below[0] + 1] - thr).min() >= 1.0:
                out.append((seed, scale, thr, below[0], row[:below[0] + 1].round(2).tolist()))
    CASES.pop('_probe', None)
    return out
