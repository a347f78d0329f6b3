"""Launch-shape and off-default-config cases for the WaveRNN kernels (csrc/wavernn.hip) — test
infrastructure only, no tests in here.

tests/test_gpu_wavernn.py compares exact logits at one launch shape (B = 2, L = 512, the
default config, uniform smoothing taps).  The cases here hand the kernel and the CPU oracle
(oracle/wr_torch_cpu.py, pinned to the reference by tests/test_oracle_wavernn.py) the SAME fp32
weights and inputs at the shapes where the launch takes other paths: one and two instances,
8 / 16 folds per instance, uneven fold splits, a second launch (fold0 = 32), zero-conditioned
fold padding, fewer than 512 classes, MOL, L = 1 / 2 / 3, one upsampling layer, small hops.

Weights: the synthetic recipe (`load_synthetic(kind='wavernn')`) on `small_config(...)`, with
the smoothing taps `upsample.up_layers.*.weight` redrawn U(0.2, 1.8) / k from the case's seed
(a trained checkpoint's taps are not uniform; uniform ones hide their order).
Inputs: mels = N(0, 1) - 4, x = U(-1, 1) from PCG64(seed); x[:, :3] = -1, 0, +1 exactly.

Teacher-forced folds: the kernel takes `xin` with `batched = 1` (set up as `generate_samples`
does); its step t reads xin[:, t], while the oracle's `generate(forced=x)` feeds x[:, t - 1] to
step t (zero at t = 0).  The kernel therefore gets `xk` = x shifted right by one step.

Bound per case: drift = max |oracle fp32 - oracle fp64| on the same fp32 inputs, bound =
max(1e-4, 10 drift) — the decoder cases' rule (tests/taco_decoder_cases.py); the margin of 10
covers the kernel's re-associated conditioning (float64 products of the linear layers) and the
mantissa bit each exchanged value carries as its tag.  The fp64 logits are the reference.

Planted defects (oracle inputs only, tests/test_wavernn_cases.py): DEFECTS below.
"""
from __future__ import annotations

import contextlib
import functools

import numpy as np
import torch
import torch.nn.functional as F

from forwardtacotron_amd.synthetic import default_config, load_synthetic
from forwardtacotron_amd.wavernn import WaveRNN
from oracle import wr_torch_cpu as wr

N_MELS, AUX = 80, 32
PER_LAUNCH = 32  # folds per launch (csrc/wavernn.hip WR_NBMAX)

# name: factors, bits (None: MOL), B, T (mel frames), fold (target, overlap) or None
CASES = {
    'b1': dict(factors=(2, 3), bits=9, B=1, T=9),
    'b3': dict(factors=(2, 3), bits=9, B=3, T=9),
    'b16': dict(factors=(2, 3), bits=9, B=16, T=9),
    'b17': dict(factors=(2, 3), bits=9, B=17, T=9),
    'b32': dict(factors=(2, 3), bits=9, B=32, T=9),
    'b33': dict(factors=(2, 3), bits=9, B=33, T=9),
    'b35': dict(factors=(2, 3), bits=9, B=35, T=9),
    'nc256': dict(factors=(2, 3), bits=8, B=3, T=9),
    'nc16': dict(factors=(2, 3), bits=4, B=5, T=9),
    'nc2': dict(factors=(3,), bits=1, B=3, T=5),
    'l1': dict(factors=(1,), bits=9, B=2, T=5),
    'l2': dict(factors=(1,), bits=9, B=2, T=6),
    'mol3': dict(factors=(2, 3), bits=None, B=3, T=9),
    'mol17': dict(factors=(2, 3), bits=None, B=17, T=9),
    'hop256': dict(factors=(4, 8, 8), bits=9, B=3, T=6),
    # teacher-forced folds of ONE utterance (B is the fold count)
    'fold42': dict(factors=(2, 3), bits=9, B=42, T=21, fold=(2, 1)),
    'fold2': dict(factors=(2, 3), bits=9, B=2, T=9, fold=(20, 5)),
}
# the launches (NBV, NI, fold0, B) each case must produce (restated host loop: launches())
LAUNCHES = {
    'b1': [(8, 1, 0, 1)], 'b3': [(8, 2, 0, 3)], 'b16': [(8, 2, 0, 16)], 'b17': [(16, 2, 0, 17)],
    'b32': [(16, 2, 0, 32)], 'b33': [(16, 2, 0, 32), (8, 1, 32, 1)],
    'b35': [(16, 2, 0, 32), (8, 2, 32, 3)], 'nc256': [(8, 2, 0, 3)], 'nc16': [(8, 2, 0, 5)],
    'nc2': [(8, 2, 0, 3)], 'l1': [(8, 2, 0, 2)], 'l2': [(8, 2, 0, 2)], 'mol3': [(8, 2, 0, 3)],
    'mol17': [(16, 2, 0, 17)], 'hop256': [(8, 2, 0, 3)],
    'fold42': [(16, 2, 0, 32), (8, 2, 32, 10)], 'fold2': [(8, 2, 0, 2)],
}

DEFECTS = {
    'frame_shift': 'the conditioning frame of sample g taken as (g + 1) // hop',
    'mel_mod32': "item b fed item (b mod 32)'s mels",
    'pad_nonzero': 'non-zero mel rows at the padded positions of the last fold',
    'taps0_reversed': 'the taps of the first smoother reversed',
    'taps1_reversed': 'the taps of the second smoother reversed',
    'smoothers_swapped': 'the two smoothers swapped (each with its own length as padding)',
    'x_zero': 'the input samples zeroed',
    'a1_zero': 'aux slice a1 (the I layer) zeroed',
    'a2_zero': 'aux slice a2 (rnn2) zeroed',
    'a3_zero': 'aux slice a3 (fc1) zeroed',
    'a4_zero': 'aux slice a4 (fc2) zeroed',
    'inactive_class_finite': 'fc3 rows past n_classes enter the Gumbel argmax with a finite logit',
}


# ---------------------------------------------------------------------------------------
# configs and weights

def small_config(factors, bits, mode='RAW'):
    """default_config() with the upsampling factors, mode and bits replaced; hop_length is
    the factors' product (the reference config keeps the two equal)."""
    cfg = default_config()
    cfg['vocoder']['model']['upsample_factors'] = [int(f) for f in factors]
    cfg['vocoder']['model']['mode'] = mode
    cfg['dsp']['bits'] = int(bits)
    cfg['dsp']['hop_length'] = int(np.prod(factors))
    return cfg


def model_cfg(cfg):
    """The oracle's view of a config: its vocoder.model section."""
    return dict(cfg['vocoder']['model'])


def model_sd(m):
    return wr.to_torch({k: v.detach().cpu() for k, v in m.state_dict().items()})


def draw_taps(rng, scale):
    """One smoother's (1, 1, 1, k) weight, k = 2 scale + 1: U(0.2, 1.8) / k (the recipe of
    the wr_upsample_taps golden, tests/golden/make_goldens_wavernn.py)."""
    k = 2 * scale + 1
    return torch.from_numpy((rng.uniform(0.2, 1.8, (1, 1, 1, k)) / k).astype(np.float32))


@functools.lru_cache(maxsize=None)
def _base_sd(factors, bits, mode):
    m = load_synthetic(WaveRNN.from_config(small_config(factors, bits, mode)), kind='wavernn')
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def state_dict(factors, bits, mode, seed):
    """The synthetic fp32 state dict of small_config(...), taps redrawn from `seed`; the big
    tensors are shared between cases and read-only."""
    sd = dict(_base_sd(tuple(factors), bits, mode))
    rng = np.random.Generator(np.random.PCG64([seed, 1]))
    for i, s in enumerate(factors):
        sd[f'upsample.up_layers.{2 * i + 1}.weight'] = draw_taps(rng, s)
    return sd


def build_model(cfg, sd, device):
    m = WaveRNN.from_config(cfg)
    m.load_state_dict(sd)
    return m.to(device).eval()


def launches(B, ni_env=2):
    """ftmi_wavernn's host loop restated: [(NBV, NI, fold0, B of the launch)].  ni_env = 1 is
    FTMI_WR_NI=1 (one instance)."""
    out, f0 = [], 0
    while f0 < B:
        b = min(B - f0, PER_LAUNCH)
        ni = 2 if (b >= 2 and ni_env != 1) else 1
        bi = (b + ni - 1) // ni
        if ni == 1:
            nbv = 8 if b <= 8 else (16 if b <= 16 else 32)
        else:
            nbv = 8 if bi <= 8 else 16
        out.append((nbv, ni, f0, b))
        f0 += b
    return out


def instance_split(b, ni):
    """Folds of each instance of one launch (wavernn_kernel's prologue)."""
    bi = (b + ni - 1) // ni
    return [min(b - i * bi, bi) for i in range(ni)]


class Case:
    """The fp32 weights and inputs both sides receive."""

    def __init__(self, name, **over):
        c = dict(CASES[name], **over)
        self.name = name
        self.factors, self.bits, self.B, self.T = tuple(c['factors']), c['bits'], c['B'], c['T']
        self.fold = c.get('fold')
        self.mode = 'MOL' if self.bits is None else 'RAW'
        self.seed = 100 + list(CASES).index(name)
        self.cfg = small_config(self.factors, 9 if self.bits is None else self.bits, self.mode)
        self.mcfg = model_cfg(self.cfg)
        self.pad = self.mcfg['pad']
        self.hop = int(np.prod(self.factors))
        self.NC = 30 if self.bits is None else 2 ** self.bits
        self.sd = state_dict(self.factors, self.cfg['dsp']['bits'], self.mode, self.seed)
        rng = np.random.Generator(np.random.PCG64(self.seed))
        if self.fold is None:
            self.L = (self.T - 2 * self.pad) * self.hop
            n_items = self.B
        else:
            target, overlap = self.fold
            self.total_len = self.T * self.hop  # generate pads the mels by `pad` frames a side
            nf = (self.total_len - overlap) // (target + overlap)
            if self.total_len - (nf * (target + overlap) + overlap) != 0:
                nf += 1
            assert nf == self.B, (name, nf)
            self.L = target + 2 * overlap
            n_items = 1
        self.mels = torch.from_numpy((rng.normal(0.0, 1.0, (n_items, N_MELS, self.T)) - 4.0).astype(np.float32))
        x = rng.uniform(-1.0, 1.0, (self.B, self.L)).astype(np.float32)
        for i, v in enumerate((-1.0, 0.0, 1.0)[:self.L]):
            x[:, i] = v
        self.x = torch.from_numpy(x)
        # what the kernel reads at step t (see the module docstring)
        self.xk = self.x if self.fold is None else F.pad(self.x, (1, 0))[:, :-1].contiguous()

    def positions(self):
        """(B, L) index g of every step in the upsampled utterance (fold cases: past
        total_len - 1 the position is padded)."""
        t = np.arange(self.L)[None, :]
        if self.fold is None:
            return np.broadcast_to(t, (self.B, self.L))
        return np.arange(self.B)[:, None] * (self.fold[0] + self.fold[1]) + t

    def padded_positions(self):
        return int((self.positions() >= self.total_len).sum()) if self.fold else 0


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


# ---------------------------------------------------------------------------------------
# the oracle, with the planted defects on its inputs

def _upsample_swapped(sd, m, cfg):
    """wr.upsample with the smoothers' order swapped; each keeps (k - 1) / 2 as its padding so
    the lengths stand."""
    scales = cfg['upsample_factors']
    total = int(np.prod(scales))
    indent = cfg['pad'] * total
    aux = wr.stretch2d(wr.mel_resnet(sd, m, cfg['res_blocks']).unsqueeze(1), total, 1).squeeze(1)
    x = m.unsqueeze(1)
    n = len(scales)
    for i, s in enumerate(scales):
        w = sd[f'upsample.up_layers.{2 * (n - 1 - i) + 1}.weight']
        x = F.conv2d(wr.stretch2d(x, s, 1), w, padding=(0, (w.size(-1) - 1) // 2))
    x = x.squeeze(1)[:, :, indent:-indent]
    return x.transpose(1, 2), aux.transpose(1, 2)


@contextlib.contextmanager
def _planted(defect):
    """Replace the oracle's upsample / fold_with_overlap for the defects that act on the
    conditioning they return."""
    up0, fold0 = wr.upsample, wr.fold_with_overlap

    def upsample(sd, m, cfg):
        if defect == 'smoothers_swapped':
            return _upsample_swapped(sd, m, cfg)
        mel, aux = up0(sd, m, cfg)
        if defect == 'frame_shift':  # frame (g + 1) // hop; the last sample keeps its frame
            aux = torch.cat([aux[:, 1:], aux[:, -1:]], 1)
        elif defect in ('a1_zero', 'a2_zero', 'a3_zero', 'a4_zero'):
            i = int(defect[1]) - 1
            aux = aux.clone()
            aux[:, :, AUX * i:AUX * (i + 1)] = 0.0
        return mel, aux

    def fold(x, target, overlap):
        out = fold0(x, target, overlap)
        if defect == 'pad_nonzero' and x.size(2) == N_MELS:
            real = fold0(torch.ones_like(x), target, overlap) != 0
            out = torch.where(real, out, torch.full_like(out, -4.0))
        return out

    wr.upsample, wr.fold_with_overlap = upsample, fold
    try:
        yield
    finally:
        wr.upsample, wr.fold_with_overlap = up0, fold0


def run_oracle(c, dtype, defect=None):
    """The oracle's logits (B, L, NC) as float64 numpy, on the case's fp32 inputs cast to dtype."""
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in c.sd.items()}
    mels, x = c.mels.to(dtype), c.x.to(dtype)
    if defect == 'mel_mod32':
        mels = mels[torch.arange(c.B) % 32]
    elif defect == 'x_zero':
        x = torch.zeros_like(x)
    elif defect in ('taps0_reversed', 'taps1_reversed'):
        k = f'upsample.up_layers.{2 * int(defect[4]) + 1}.weight'
        sd[k] = sd[k].flip(-1)
    with torch.no_grad(), _planted(defect):
        if c.fold is None:
            logits = wr.forward(sd, c.mcfg, x, mels)
        else:
            trace = []
            wr.generate(sd, c.mcfg, mels, batched=True, target=c.fold[0], overlap=c.fold[1],
                        forced=x, trace=trace, steps=c.L)
            logits = torch.stack(trace, 1)
    assert logits.dtype == dtype and tuple(logits.shape) == (c.B, c.L, c.NC)
    return logits.double().numpy()


@functools.lru_cache(maxsize=None)
def oracle(name, dtype=torch.float64, defect=None):
    """Computed once per (case, dtype, defect), read-only."""
    out = run_oracle(case(name), dtype, defect)
    out.setflags(write=False)
    return out


def drift_of(c):
    return float(np.abs(run_oracle(c, torch.float32) - run_oracle(c, torch.float64)).max())


@functools.lru_cache(maxsize=None)
def drift(name):
    return float(np.abs(oracle(name, torch.float32) - oracle(name)).max())


def bound_from(d):
    return max(1e-4, 10.0 * d)


def bound(name):
    return bound_from(drift(name))


def existing_bar(l64):
    """tests/test_gpu_wavernn.py's bar at the case's largest logit: no case bound may exceed it."""
    return 2e-4 + 2e-5 * float(np.abs(l64).max())


def preactivations(name):
    """(fc1, fc2) pre-activations and the logits of a case (float64), recomputed from the
    oracle's tensors with WaveRNN.forward's body (the logits must equal oracle(name))."""
    c = case(name)
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in c.sd.items()}
    with torch.no_grad():
        m, aux = wr.upsample(sd, c.mels.double(), c.mcfg)
        a1, a2, a3, a4 = (aux[:, :, AUX * i:AUX * (i + 1)] for i in range(4))
        h = F.linear(torch.cat([c.x.double().unsqueeze(-1), m, a1], 2), sd['I.weight'], sd['I.bias'])
        z = torch.zeros(c.B, h.size(2), dtype=h.dtype)
        h = wr._gru_seq(sd, 'rnn1', h, z) + h
        h = wr._gru_seq(sd, 'rnn2', torch.cat([h, a2], 2), z) + h
        p1 = F.linear(torch.cat([h, a3], 2), sd['fc1.weight'], sd['fc1.bias'])
        p2 = F.linear(torch.cat([F.relu(p1), a4], 2), sd['fc2.weight'], sd['fc2.bias'])
        logits = F.linear(F.relu(p2), sd['fc3.weight'], sd['fc3.bias'])
    return p1.numpy(), p2.numpy(), logits.numpy()


def gumbel_draws(logits, seed, slots=None, fill=0.0):
    """The kernel's RAW draw restated on (B, L, NC) logits: argmax_k logit_k - log(-log u_k)
    with the Philox words of class k.  slots > NC: the planted defect — the fc3 rows past NC
    (the FC workgroups hold `slots` = 512 of them) enter with logit `fill` instead of -inf."""
    B, L, NC = logits.shape
    s = wr.PhiloxSampler(seed)
    out = np.zeros((B, L), dtype=np.int64)
    for t in range(L):
        l = logits[:, t]
        if slots is not None and slots > NC:
            l = np.concatenate([l, np.full((B, slots - NC), fill)], 1)
        out[:, t] = np.argmax(s.gumbel_scores(torch.from_numpy(np.ascontiguousarray(l)), t), axis=1)
    return out


# ---------------------------------------------------------------------------------------
# the GPU side

def gpu_logits(c, model):
    """The kernel's teacher-forced logits of a case -> ((B, L, NC) float32 numpy, status word).
    Fold cases: `_upsample` on the padded rows, then `_run(batched=True, xin=...)`, as
    generate_samples sets the launch up."""
    from forwardtacotron_amd import ops
    dev = model.step.device
    if c.fold is None:
        out = model.forward(c.x, c.mels)
    else:
        target, overlap = c.fold
        with torch.no_grad():
            rows = model.pad_tensor(c.mels.to(dev).transpose(1, 2), pad=model.pad, side='both')

            def run():
                m_up, frames = model._upsample(rows)
                B, L = model._fold_shape(m_up.size(1), m_up.size(0), True, target, overlap)
                assert (B, L) == (c.B, c.L), (B, L)
                return model._run(m_up, frames, batched=True, L=L, fold_stride=target + overlap,
                                  B=B, xin=c.xk)
            out = ops.run_checked(run, dev)
    status = int(ops.status_word(dev).item())
    return out.cpu().numpy(), status


def check_draws(m, cfg, mels, seed, target, overlap, batched=True):
    """generate_samples against the oracle fed the GPU's own sample sequence: every choice is
    the oracle's argmax or within 1e-3 of it, >= 99.5 % exact."""
    smp = m.generate_samples(torch.from_numpy(mels), batched, target, overlap, seed=seed).cpu().numpy()
    trace = []
    sd = model_sd(m)
    wr.generate(sd, model_cfg(cfg), torch.from_numpy(mels), batched=batched, target=target,
                overlap=overlap, forced=smp, trace=trace, steps=smp.shape[1])
    sampler = wr.PhiloxSampler(seed)
    nc = m.n_classes
    exact = total = 0
    for t, logits in enumerate(trace):
        if m.mode == 'RAW':
            z = sampler.gumbel_scores(logits, t)
            idx = np.rint((smp[:, t] + 1.0) * (nc - 1) / 2.0).astype(np.int64)
            best = z.max(axis=1)
            got = z[np.arange(z.shape[0]), idx]
            assert np.all(best - got <= 1e-3), (t, (best - got).max())
            exact += int(np.sum(np.argmax(z, axis=1) == idx))
        else:
            tu, u = sampler.mol_uniforms(t, logits.size(0), nc // 3)
            x = wr.sample_mol(logits, tu, u).numpy()
            close = np.abs(x - smp[:, t]) <= 1e-4 + 1e-4 * np.abs(x)
            exact += int(close.sum())
        total += logits.size(0)
    assert exact >= 0.995 * total, (exact, total)
    return smp


def finish_ref(smp, batched, target, overlap, mu_law, n_classes, wave_len, fade_len):
    """wr.finish with a free fade_len (0: none), float64 numpy, from the oracle's own pieces."""
    out = np.array(smp, dtype=np.float64)
    if mu_law:
        out = wr.decode_mu_law(out, n_classes, False)
    out = wr.xfade_and_unfold(out, target, overlap) if batched else out[0]
    out = out[:wave_len].copy()
    if fade_len > 0:
        out[-fade_len:] *= np.linspace(1, 0, fade_len)
    return out
