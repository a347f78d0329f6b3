"""Cases for the packed WaveRNN launches (ftmi_wavernn_packed, WaveRNN.generate_batch): several
utterances of unequal length whose folds share launches — test infrastructure only, no tests in
here.  Built on tests/wr_cases.py (configs, weights, bound rule) and oracle/wr_torch_cpu.py.

Shapes: hop 6 (factors (2, 3)).  Batched: utterances of T = 21, 27, 45 mel frames at target 5,
overlap 1 (fold length 7, stride 6): T * 6 samples fold into T rows, the last with ONE padded
position, so 21 + 27 + 45 = 93 folds in launches of 32, 32 and 29.  Utterance 1 straddles the
first launch boundary, utterance 2 the second; utterance 0 ends inside the second instance of
the first launch.  Unbatched: T = 21, 30, 33, one row each, run longest first.

The oracle sees one utterance at a time — `wr.generate(mels_i, forced=x_i, trace=...)`, float64
— which is what a packed run has to reproduce row for row.  Inputs per utterance: mels =
N(0, 1) - 4, x = U(-1, 1) with x[:, :3] = -1, 0, +1, from PCG64([seed, i]); the kernel's xin is
x shifted right by one step (tests/wr_cases.py docstring).

Planted defects (oracle only, tests/test_wavernn_pack.py): DEFECTS below.
"""
from __future__ import annotations

import contextlib
import functools

import numpy as np
import torch
import torch.nn.functional as F

import wr_cases as C
from oracle import wr_torch_cpu as wr

FACTORS, HOP = (2, 3), 6
ITEMS_T = (21, 27, 45)
FOLD = (5, 1)  # target, overlap
UNBATCHED_T = (21, 30, 33)
SEEDS = (1234567, 89, 2 ** 40 + 17)  # per utterance; the last uses the key's high word

DEFECTS = {
    'reads_next_item': "a fold past its utterance's end reads the next utterance's rows, not padding",
    'global_fold_word': 'the Philox fold word counts over the whole table, not per utterance',
    'first_items_key': "the second utterance draws with the first utterance's key",
}


def fold_count(T, target, overlap, hop=HOP):
    total = T * hop
    nf = (total - overlap) // (target + overlap)
    if total - (nf * (target + overlap) + overlap) != 0:
        nf += 1
    return nf


class Pack:
    """The fp32 weights and per-utterance inputs both sides receive."""

    def __init__(self, bits, lengths=ITEMS_T, fold=FOLD):
        self.bits, self.lengths, self.fold = bits, tuple(lengths), fold
        self.mode = 'MOL' if bits is None else 'RAW'
        self.seed = 300 + (0 if bits is None else bits)
        self.cfg = C.small_config(FACTORS, 9 if bits is None else bits, self.mode)
        self.mcfg = C.model_cfg(self.cfg)
        self.NC = 30 if bits is None else 2 ** bits
        self.sd = C.state_dict(FACTORS, self.cfg['dsp']['bits'], self.mode, self.seed)
        self.L = fold[0] + 2 * fold[1]
        self.folds = [fold_count(T, *fold) for T in self.lengths]
        self.mels, self.x, self.xk = [], [], []
        for i, (T, nf) in enumerate(zip(self.lengths, self.folds)):
            rng = np.random.Generator(np.random.PCG64([self.seed, i]))
            self.mels.append(torch.from_numpy((rng.normal(0.0, 1.0, (1, C.N_MELS, T)) - 4.0).astype(np.float32)))
            x = rng.uniform(-1.0, 1.0, (nf, self.L)).astype(np.float32)
            for k, v in enumerate((-1.0, 0.0, 1.0)[:self.L]):
                x[:, k] = v
            self.x.append(torch.from_numpy(x))
            self.xk.append(F.pad(self.x[-1], (1, 0))[:, :-1].contiguous())


@functools.lru_cache(maxsize=None)
def pack(bits):
    return Pack(bits)


def _unfolded(sd, mcfg, mels):
    """One utterance's conditioning before folding: (mel rows (1, T hop, 80), aux (1, T hop, 128))."""
    m, aux, _ = wr.conditioning(sd, mcfg, mels, False, 0, 0)
    return m, aux


@contextlib.contextmanager
def _reads_next_item(sd, p, i):
    """wr.conditioning replaced for utterance i: its folds cut from the utterances' rows laid
    end to end (as `mel` / `cond` hold them), so the position past its end is the next
    utterance's first row; past the last utterance there is padding, as there should be."""
    target, overlap = p.fold
    stride, nf = target + overlap, p.folds[i]
    parts = [_unfolded(sd, p.mcfg, m.to(sd['I.weight'].dtype)) for m in p.mels[i:]]
    need = (nf - 1) * stride + p.L
    cat = [torch.cat([q[k] for q in parts], 1) for k in (0, 1)]
    cat = [F.pad(c, (0, 0, 0, max(0, need - c.size(1)))) for c in cat]
    folded = [torch.stack([c[0, j * stride:j * stride + p.L] for j in range(nf)]) for c in cat]
    cond0 = wr.conditioning

    def conditioning(sd_, cfg, mels, batched, tg, ov):
        return folded[0], folded[1], (mels.size(-1) - 1) * HOP

    wr.conditioning = conditioning
    try:
        yield
    finally:
        wr.conditioning = cond0


def run_oracle(p, i, dtype, defect=None):
    """The oracle's teacher-forced logits of utterance i alone, (folds_i, L, NC) float64 numpy."""
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in p.sd.items()}
    ctx = _reads_next_item(sd, p, i) if defect == 'reads_next_item' else contextlib.nullcontext()
    trace = []
    with torch.no_grad(), ctx:
        wr.generate(sd, p.mcfg, p.mels[i].to(dtype), batched=True, target=p.fold[0], overlap=p.fold[1],
                    forced=p.x[i].to(dtype), trace=trace, steps=p.L)
    logits = torch.stack(trace, 1)
    assert logits.dtype == dtype and tuple(logits.shape) == (p.folds[i], p.L, p.NC)
    return logits.double().numpy()


@functools.lru_cache(maxsize=None)
def oracle(bits, i, dtype=torch.float64, defect=None):
    out = run_oracle(pack(bits), i, dtype, defect)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def drift(bits, i):
    return float(np.abs(oracle(bits, i, torch.float32) - oracle(bits, i)).max())


def bound(bits, i):
    return C.bound_from(drift(bits, i))


def item_rows(lengths_folds):
    """[(first row, folds)] of utterances laid out consecutively."""
    out, r = [], 0
    for nf in lengths_folds:
        out.append((r, nf))
        r += nf
    return out


# ---------------------------------------------------------------------------------------
# the draws, restated with a free fold word and key

def gumbel_draws(logits, seed, word0=0):
    """The kernel's RAW draw on (B, L, NC) logits with fold words word0 .. word0 + B - 1."""
    B, L, NC = logits.shape
    s = wr.PhiloxSampler(seed)
    out = np.zeros((B, L), dtype=np.int64)
    for t in range(L):
        l = np.concatenate([np.zeros((word0, NC)), logits[:, t]], 0)
        z = s.gumbel_scores(torch.from_numpy(np.ascontiguousarray(l)), t)
        out[:, t] = np.argmax(z[word0:], axis=1)
    return out


def mol_draws(logits, seed, word0=0):
    """The kernel's MOL draw on (B, L, 30) logits with fold words word0 .. word0 + B - 1."""
    B, L, NC = logits.shape
    s = wr.PhiloxSampler(seed)
    out = np.zeros((B, L), dtype=np.float64)
    for t in range(L):
        tu, u = s.mol_uniforms(t, word0 + B, NC // 3)
        l = torch.from_numpy(np.array(logits[:, t], dtype=np.float32))
        out[:, t] = wr.sample_mol(l, tu[word0:], u[word0:]).numpy()
    return out


def check_item_draws(m, cfg, mels, smp, seed, target, overlap, batched=True):
    """tests/wr_cases.py check_draws' rule on samples already drawn: the oracle is fed ONE
    utterance (mels (1, 80, T)) and its rows `smp` of a packed run, with PhiloxSampler(seed)
    and the utterance's own fold indices 0 .. B - 1.  Every choice is the oracle's argmax or
    within 1e-3 of it; returns (exact, total) for the caller's 99.5 % count."""
    trace = []
    sd = C.model_sd(m)
    wr.generate(sd, C.model_cfg(cfg), torch.as_tensor(mels), batched=batched, target=target,
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
            exact += int((np.abs(x - smp[:, t]) <= 1e-4 + 1e-4 * np.abs(x)).sum())
        total += logits.size(0)
    return exact, total


# ---------------------------------------------------------------------------------------
# the GPU side

def gpu_packed_logits(p, model, order=None, host_table=False):
    """Teacher-forced logits of the pack's utterances in shared launches, utterances in `order`
    (default 0, 1, 2) -> ((F, L, NC) float32 numpy, the plan, status word)."""
    from forwardtacotron_amd import ops
    order = list(range(len(p.lengths))) if order is None else list(order)
    dev = model.step.device
    plan = model.pack_plan([p.lengths[i] for i in order], True, *p.fold)
    mels = [p.mels[i] for i in order]
    xin = torch.cat([p.xk[i] for i in order], 0)
    with torch.no_grad():
        def run():
            m_rows, frames = model._condition_batch(mels, plan)
            return model._run_packed(m_rows, frames, plan, [0] * len(order), xin=xin,
                                     host_table=host_table)
        out = ops.run_checked(run, dev)
    return out.cpu().numpy(), plan, int(ops.status_word(dev).item())


def gpu_single_logits(p, model, i):
    """Utterance i alone through the one-utterance launch, as tests/wr_cases.py gpu_logits."""
    from forwardtacotron_amd import ops
    dev = model.step.device
    target, overlap = p.fold
    with torch.no_grad():
        rows = model.pad_tensor(p.mels[i].to(dev).transpose(1, 2), pad=model.pad, side='both')

        def run():
            m_up, frames = model._upsample(rows)
            B, L = model._fold_shape(m_up.size(1), m_up.size(0), True, target, overlap)
            assert (B, L) == (p.folds[i], p.L), (B, L)
            return model._run(m_up, frames, batched=True, L=L, fold_stride=target + overlap, B=B,
                              xin=p.xk[i])
        out = ops.run_checked(run, dev)
    return out.cpu().numpy(), int(ops.status_word(dev).item())
