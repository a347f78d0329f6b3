"""CPU baseline + checker of the Tacotron path — test infrastructure only.

A functional torch-CPU restatement of the reference's Tacotron inference
(models/tacotron.py: Encoder :21-26, PreNet :36-43 in eval mode, LSA :81-99, Decoder.forward
:124-174 in eval mode, Tacotron.forward :216-270, Tacotron.generate :272-331), written from
the formulas on the ATen CPU ops the reference reaches (linear, conv1d, gru_cell, lstm_cell,
softmax), with no nn.Module and no import of the reference.  It works on a {key: tensor}
state dict in the dict's floating-point dtype (float64 gives the higher-precision truth).
Pinned against the reference goldens by tests/test_oracle_tacotron.py; tools/taco_bench.py
times it as the CPU baseline.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle.ft_torch_cpu import cbhg, to_torch  # noqa: F401  (to_torch re-exported)

MAX_R = 20


def _prenet(sd, pre, x):
    x = F.relu(F.linear(x, sd[pre + '.fc1.weight'], sd[pre + '.fc1.bias']))
    return F.relu(F.linear(x, sd[pre + '.fc2.weight'], sd[pre + '.fc2.bias']))


def _k(sd, pre):
    k = 0
    while f'{pre}.conv1d_bank.{k}.conv.weight' in sd:
        k += 1
    return k


def encode(sd, ids):
    """(B, T) ids -> encoder_seq (B, T, 256), encoder_seq_proj."""
    x = _prenet(sd, 'encoder.pre_net', F.embedding(ids, sd['encoder.embedding.weight']))
    enc = cbhg(sd, 'encoder.cbhg', x.transpose(1, 2), _k(sd, 'encoder.cbhg'))
    return enc, F.linear(enc, sd['encoder_proj.weight'])


def postnet(sd, mel):
    """mel (B, 80, F) -> linear (B, 80, F)."""
    post = cbhg(sd, 'postnet', mel, _k(sd, 'postnet'))
    return F.linear(post, sd['post_proj.weight']).transpose(1, 2)


class DecoderState:
    def __init__(self, sd, enc):
        B, T, D = enc.shape
        H = sd['decoder.res_rnn1.weight_hh'].shape[1]
        z = lambda *s: torch.zeros(*s, dtype=enc.dtype)  # noqa: E731
        self.hA, self.ctx = z(B, D), z(B, D)
        self.h1, self.c1, self.h2, self.c2 = z(B, H), z(B, H), z(B, H), z(B, H)
        self.cum, self.att = z(B, T), z(B, T)


def decoder_step(sd, st, enc, enc_proj, prenet_in, r):
    """One Decoder.forward in eval mode -> (frames (B, 80, r), scores (B, T))."""
    d = 'decoder.'
    p = _prenet(sd, d + 'prenet', prenet_in)
    g = d + 'attn_rnn.'
    st.hA = torch.gru_cell(torch.cat([st.ctx, p], -1), st.hA, sd[g + 'weight_ih'], sd[g + 'weight_hh'],
                           sd[g + 'bias_ih'], sd[g + 'bias_hh'])
    a = d + 'attn_net.'
    q = F.linear(st.hA, sd[a + 'W.weight'], sd[a + 'W.bias']).unsqueeze(1)
    loc = torch.stack([st.cum, st.att], 1)
    conv = F.conv1d(loc, sd[a + 'conv.weight'], padding=(sd[a + 'conv.weight'].shape[2] - 1) // 2)
    ploc = F.linear(conv.transpose(1, 2), sd[a + 'L.weight'], sd[a + 'L.bias'])
    u = F.linear(torch.tanh(q + enc_proj + ploc), sd[a + 'v.weight']).squeeze(-1)
    st.att = F.softmax(u, dim=1)
    st.cum = st.cum + st.att
    st.ctx = (st.att.unsqueeze(1) @ enc).squeeze(1)
    x = F.linear(torch.cat([st.ctx, st.hA], 1), sd[d + 'rnn_input.weight'], sd[d + 'rnn_input.bias'])
    for n in ('1', '2'):
        c = d + f'res_rnn{n}.'
        h, cc = torch.lstm_cell(x, (getattr(st, 'h' + n), getattr(st, 'c' + n)), sd[c + 'weight_ih'],
                                sd[c + 'weight_hh'], sd[c + 'bias_ih'], sd[c + 'bias_hh'])
        setattr(st, 'h' + n, h)
        setattr(st, 'c' + n, cc)
        x = x + h
    mels = F.linear(x, sd[d + 'mel_proj.weight']).view(x.size(0), -1, MAX_R)[:, :, :r]
    return mels, st.att


def forward(sd, ids, m, r):
    """Tacotron.forward (eval): ids (B, T), m (B, 80, F) -> mel (B, 80, n r), linear, attn (B, n, T)."""
    enc, enc_proj = encode(sd, ids)
    st = DecoderState(sd, enc)
    go = torch.zeros(m.size(0), m.size(1), dtype=enc.dtype)
    mels, attns = [], []
    for t in range(0, m.size(2), r):
        fr, sc = decoder_step(sd, st, enc, enc_proj, m[:, :, t - 1] if t > 0 else go, r)
        mels.append(fr)
        attns.append(sc.unsqueeze(1))
    mel = torch.cat(mels, 2)
    return mel, postnet(sd, mel), torch.cat(attns, 1)


def generate(sd, ids, steps, r, stop_threshold, trace=None):
    """Tacotron.generate: ids (1, T) -> mel (80, n r), linear (80, n r), attn (n, T).
    trace (a list) receives each step's largest frame value (what the stop rule compares)."""
    enc, enc_proj = encode(sd, ids)
    st = DecoderState(sd, enc)
    n_mels = sd['decoder.prenet.fc1.weight'].shape[1]
    go = torch.zeros(1, n_mels, dtype=enc.dtype)
    mels, attns = [], []
    for t in range(0, steps, r):
        fr, sc = decoder_step(sd, st, enc, enc_proj, mels[-1][:, :, -1] if t > 0 else go, r)
        mels.append(fr)
        attns.append(sc.unsqueeze(1))
        if trace is not None:
            trace.append(float(fr.max()))
        if bool((fr < stop_threshold).all()) and t > 10:
            break
    mel = torch.cat(mels, 2)
    return mel[0], postnet(sd, mel)[0], torch.cat(attns, 1)[0]
