"""Tacotron (reference: `models/tacotron.py`) on libftmi.so: CBHG encoder -> location-sensitive
attention decoder -> CBHG postnet.  The model `gen_tacotron.py` synthesises with and
`train_tacotron.py` runs teacher-forced for the attention matrices the ForwardTacotron
durations are extracted from.

Parameters and buffers carry exactly the reference's names and shapes (``step``,
``stop_threshold``, ``decoder.r`` included), so ``load_state_dict(ckpt['model'])`` works
unchanged.  No torch compute layers: the encoder and the postnet run the package's GEMM /
CBHG kernels (default f16x3 path), the decoder loop is ONE persistent launch
(`csrc/tacotron.hip`, exact fp32): `generate` reads a single device word (the number of steps
the device-side stop rule took) after it, `forward` reads nothing.

Inference numerics only: no dropout (the reference applies the prenets' dropout in training
mode only) and no zoneout.  Like `ForwardTacotron.forward` here, `forward` called in training
mode advances ``step`` and still computes the eval-mode result.
"""
from __future__ import annotations

from pathlib import Path
from typing import Any, Dict, Tuple, Union

import numpy as np
import torch
import torch.nn as nn

from . import _lib, ops
from .common_layers import CBHG, Conv1dParams, LinearParams, Packed, _uniform_, check_device
from .forward_tacotron import Embedding
from .text.symbols import phonemes


class PreNet(nn.Module):
    """`models/tacotron.py:29-43` in eval mode: relu(fc2(relu(fc1(x))))."""

    def __init__(self, in_dims: int, fc1_dims: int = 256, fc2_dims: int = 128, dropout: float = 0.5) -> None:
        super().__init__()
        self.fc1 = LinearParams(in_dims, fc1_dims)
        self.fc2 = LinearParams(fc1_dims, fc2_dims)
        self.p = dropout

    def forward_cl(self, x: torch.Tensor) -> torch.Tensor:
        """(B, T, in_dims) -> (B, T, fc2_dims): two k = 1 convolutions with bias and ReLU."""
        for fc in (self.fc1, self.fc2):
            w, b, w3 = fc.packed_weights()
            x, _ = ops.conv1d(x, w, 1, 0, bias=b, relu=True, w_split=w3)
        return x

    forward = forward_cl


class Encoder(nn.Module):
    """`models/tacotron.py:12-26`."""

    def __init__(self, embed_dims, num_chars, cbhg_channels, K, num_highways, dropout) -> None:
        super().__init__()
        self.embedding = Embedding(num_chars, embed_dims)
        self.pre_net = PreNet(embed_dims)
        self.cbhg = CBHG(K=K, in_channels=cbhg_channels, channels=cbhg_channels,
                         proj_channels=[cbhg_channels, cbhg_channels], num_highways=num_highways)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """(B, T) ids -> (B, T, 2 cbhg_channels)."""
        h = ops.embedding(x, self.embedding.weight.detach())
        return self.cbhg.forward_cl(self.pre_net.forward_cl(h))


class LSA(nn.Module):
    """Parameters of `models/tacotron.py:65-73` (the arithmetic is in the decoder launch)."""

    def __init__(self, attn_dim: int, kernel_size: int = 31, filters: int = 32) -> None:
        super().__init__()
        self.conv = Conv1dParams(2, filters, kernel_size, bias=False)
        self.L = LinearParams(filters, attn_dim, bias=True)
        self.W = LinearParams(attn_dim, attn_dim, bias=True)
        self.v = LinearParams(attn_dim, 1, bias=False)


class CellParams(nn.Module):
    """Parameters of nn.GRUCell (gates = 3) / nn.LSTMCell (gates = 4)."""

    def __init__(self, fin: int, hidden: int, gates: int) -> None:
        super().__init__()
        self.input_size, self.hidden_size = fin, hidden
        b = 1.0 / np.sqrt(hidden)
        for name, shape in (('weight_ih', (gates * hidden, fin)), ('weight_hh', (gates * hidden, hidden)),
                            ('bias_ih', (gates * hidden,)), ('bias_hh', (gates * hidden,))):
            prm = nn.Parameter(torch.empty(*shape))
            _uniform_(prm, b)
            self.register_parameter(name, prm)


class Decoder(Packed):
    """Parameters of `models/tacotron.py:102-117`, packed for `ftmi_tacotron_decoder`."""
    max_r = 20

    def __init__(self, n_mels: int, decoder_dims: int, lstm_dims: int) -> None:
        super().__init__()
        self.register_buffer('r', torch.tensor(1, dtype=torch.int))
        self.n_mels, self.decoder_dims, self.lstm_dims = n_mels, decoder_dims, lstm_dims
        self.prenet = PreNet(n_mels)
        self.attn_net = LSA(decoder_dims)
        self.attn_rnn = CellParams(decoder_dims + decoder_dims // 2, decoder_dims, 3)
        self.rnn_input = LinearParams(2 * decoder_dims, lstm_dims)
        self.res_rnn1 = CellParams(lstm_dims, lstm_dims, 4)
        self.res_rnn2 = CellParams(lstm_dims, lstm_dims, 4)
        self.mel_proj = LinearParams(lstm_dims, n_mels * self.max_r, bias=False)

    def _pack(self):
        c = lambda t: t.detach().float().contiguous()  # noqa: E731
        p, at = self.prenet, self.attn_net
        d = self.decoder_dims
        pk = {
            'pre_w1t': c(p.fc1.weight.t()), 'pre_b1': c(p.fc1.bias),
            'pre_w2t': c(p.fc2.weight.t()), 'pre_b2': c(p.fc2.bias),
            'gru_wih': c(self.attn_rnn.weight_ih), 'gru_whh': c(self.attn_rnn.weight_hh),
            'gru_bih': c(self.attn_rnn.bias_ih), 'gru_bhh': c(self.attn_rnn.bias_hh),
            'lsa_conv': c(at.conv.weight), 'lsa_L': c(at.L.weight), 'lsa_Lb': c(at.L.bias),
            'lsa_wt': c(at.W.weight.t()), 'lsa_Wb': c(at.W.bias), 'lsa_v': c(at.v.weight.reshape(-1)),
            'rin_w': c(self.rnn_input.weight), 'rin_b': c(self.rnn_input.bias),
            'mel_w': c(self.mel_proj.weight),
        }
        for n, cell in (('l1', self.res_rnn1), ('l2', self.res_rnn2)):
            pk[n + '_wih'], pk[n + '_whh'] = c(cell.weight_ih), c(cell.weight_hh)
            pk[n + '_bih'], pk[n + '_bhh'] = c(cell.bias_ih), c(cell.bias_hh)
        # teacher-forced: the prenet's share of the attention GRU's input product, as a GEMM
        w_pre = c(self.attn_rnn.weight_ih[:, d:])
        pk['gi_pre'] = (w_pre, pk['gru_bih'], ops.presplit_for(w_pre))
        return pk

    def launch(self, enc: torch.Tensor, enc_proj: torch.Tensor, r: int, steps: int,
               stop_threshold: float, prenet_in: torch.Tensor = None, stamps: torch.Tensor = None):
        """One persistent launch over (B <= ops.TACO_MAX_BATCH, T, 256) encoder rows.
        prenet_in None: free-running (B = 1) -> (mel (1, n r, 80), attn (1, n, T), steps word);
        prenet_in (B, n, 80), the frame fed to each step: teacher-forced."""
        pk = self.packed_weights()
        B, T, _ = enc.shape
        n = (steps + r - 1) // r
        dev = enc.device
        mel = torch.zeros(B, n * r, self.n_mels, device=dev)
        attn = torch.zeros(B, n, T, device=dev)
        steps_out = torch.zeros(1, device=dev, dtype=torch.int32)
        ws = ops.tacotron_decoder_workspace(B, T, dev)
        a = _lib.TacoArgs()
        for k, v in pk.items():
            if k != 'gi_pre':
                setattr(a, k, v.data_ptr())
        keep = [enc.contiguous(), enc_proj.contiguous()]
        a.enc, a.enc_proj = keep[0].data_ptr(), keep[1].data_ptr()
        if prenet_in is not None:
            w_pre, b_ih, w3 = pk['gi_pre']
            pre = self.prenet.forward_cl(prenet_in)
            gi, _ = ops.conv1d(pre, w_pre, 1, 0, bias=b_ih, w_split=w3)
            gi = gi.contiguous()
            keep.append(gi)
            a.pre_gi = gi.data_ptr()
        a.mel_out, a.attn_out, a.steps_out = mel.data_ptr(), attn.data_ptr(), steps_out.data_ptr()
        a.workspace = ws.data_ptr()
        if stamps is not None:  # diagnostic: int64[FTMI_TACO_STAMPS] phase sums (tools/taco_stamps.py)
            a.stamps = stamps.data_ptr()
        a.stop_threshold = float(stop_threshold)
        a.B, a.T, a.r, a.steps = B, T, r, steps
        a.decoder_dims, a.lstm_dims, a.n_mels = self.decoder_dims, self.lstm_dims, self.n_mels
        a.prenet_dims = self.prenet.fc2.out_features
        ops.tacotron_decoder(a, dev)
        for t in keep + [ws]:  # stream-ordered: the caching allocator frees after the launch
            t.record_stream(torch.cuda.current_stream(dev))
        return mel, attn, steps_out


class Tacotron(nn.Module):
    """`models/tacotron.py:177-356`."""

    def __init__(self, embed_dims: int, num_chars: int, encoder_dims: int, decoder_dims: int,
                 n_mels: int, postnet_dims: int, encoder_k: int, lstm_dims: int, postnet_k: int,
                 num_highways: int, dropout: float, stop_threshold: float) -> None:
        super().__init__()
        self.n_mels = n_mels
        self.lstm_dims = lstm_dims
        self.decoder_dims = decoder_dims
        self.encoder = Encoder(embed_dims, num_chars, encoder_dims, encoder_k, num_highways, dropout)
        self.encoder_proj = LinearParams(decoder_dims, decoder_dims, bias=False)
        self.decoder = Decoder(n_mels, decoder_dims, lstm_dims)
        self.postnet = CBHG(postnet_k, n_mels, postnet_dims, [256, 80], num_highways)
        self.post_proj = LinearParams(postnet_dims * 2, n_mels, bias=False)
        self.init_model()
        self.register_buffer('step', torch.zeros(1, dtype=torch.long))
        self.register_buffer('stop_threshold', torch.tensor(stop_threshold, dtype=torch.float32))

    @property
    def r(self) -> int:
        return self.decoder.r.item()

    @r.setter
    def r(self, value: int) -> None:
        self.decoder.r = self.decoder.r.new_tensor(value, requires_grad=False)

    # ---------------------------------------------------------------------------------
    def _check_device(self, x: torch.Tensor) -> None:
        check_device(self.encoder.embedding.weight, x, 'Tacotron',
                     'call .to("cuda") (there is no CPU fallback)')

    def _encode(self, x: torch.Tensor):
        enc = self.encoder(x)
        w, _, w3 = self.encoder_proj.packed_weights()
        enc_proj, _ = ops.conv1d(enc, w, 1, 0, w_split=w3)
        return enc, enc_proj

    def _post(self, mel_cl: torch.Tensor) -> torch.Tensor:
        """(B, F, 80) frames -> linear (B, 80, F): the postnet CBHG and post_proj."""
        post = self.postnet.forward_cl(mel_cl)
        w, _, w3 = self.post_proj.packed_weights()
        linear = torch.empty(mel_cl.size(0), self.n_mels, mel_cl.size(1), device=mel_cl.device)
        ops.conv1d(post, w, 1, 0, out_t=linear, want_y=False, w_split=w3)
        return linear

    def _check_tokens(self, T: int) -> None:
        if not 1 <= T <= ops.TACO_MAX_TOKENS:
            raise _lib.FtmiError(f'the Tacotron decoder launch takes 1..{ops.TACO_MAX_TOKENS} tokens '
                                 f'(got {T}): FTMI_E_UNSUPPORTED')

    def forward(self, x: torch.Tensor, m: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """Teacher-forced pass (`models/tacotron.py:216-270`), inference numerics: x (B, T)
        ids, m (B, 80, F) -> (mel (B, 80, n r), linear (B, 80, n r), attn (B, n, T)),
        n = ceil(F / r).  No masking: attention runs over the pad tokens too."""
        self._check_device(x)
        self._check_tokens(x.size(1))
        if self.training:
            self.step += 1
        return ops.run_checked(lambda: self._forward(x, m), x.device)

    def _forward(self, x, m):
        r = self.r
        B, _, F = m.shape
        n = (F + r - 1) // r
        enc, enc_proj = self._encode(x)
        # the frame fed to step s: m[:, :, s r - 1], the zero <GO> frame for s = 0
        m_cl = m.transpose(1, 2).float()
        prenet_in = torch.zeros(B, n, self.n_mels, device=m.device)
        if n > 1:
            prenet_in[:, 1:] = m_cl[:, r - 1:(n - 1) * r:r]
        mels, attns = [], []
        for b0 in range(0, B, ops.TACO_MAX_BATCH):
            sl = slice(b0, b0 + ops.TACO_MAX_BATCH)
            mel, attn, _ = self.decoder.launch(enc[sl], enc_proj[sl], r, F, 0.0, prenet_in[sl].contiguous())
            mels.append(mel)
            attns.append(attn)
        mel_cl = torch.cat(mels, 0)
        linear = self._post(mel_cl)
        return mel_cl.transpose(1, 2).contiguous(), linear, torch.cat(attns, 0)

    def generate(self, x: torch.Tensor, steps: int = 2000) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """`models/tacotron.py:272-331`: x (1, T) ids -> numpy (mel (80, n r), linear (80, n r),
        attn (n, T)).  The decoder loop, its feedback and the stop rule (every value of a
        step's r frames < stop_threshold and t > 10) run in one launch; its step count is the
        one value read back before the postnet."""
        self.eval()
        self._check_device(x)
        if x.size(0) != 1:
            raise ValueError('generate takes one sequence, x of shape (1, T), like the reference')
        self._check_tokens(x.size(1))
        r = self.r
        thr = float(self.stop_threshold.item())

        def run():
            enc, enc_proj = self._encode(x)
            mel, attn, steps_out = self.decoder.launch(enc, enc_proj, r, steps, thr)
            n = int(steps_out.item())
            if n <= 0:  # the launch never wrote its count: a timeout, reported by run_checked
                n = 1
            mel_cl = mel[0, :n * r].unsqueeze(0)  # B = 1: rows with a uniform batch stride
            linear = self._post(mel_cl)
            return mel_cl, linear, attn[:, :n]

        mel_cl, linear, attn = ops.run_checked(run, x.device)
        out = (mel_cl[0].t().cpu().numpy(), linear[0].cpu().numpy(), attn[0].cpu().numpy())
        self.train()
        return out

    # ---------------------------------------------------------------------------------
    def init_model(self) -> None:
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)

    def get_step(self) -> int:
        return self.step.data.item()

    def reset_step(self) -> None:
        # assignment to parameters or buffers is overloaded, updates internal dict entry
        self.step = self.step.data.new_tensor(1)

    @classmethod
    def from_config(cls, config: Dict[str, Any]) -> 'Tacotron':
        model_config = config['tacotron']['model']
        model_config['num_chars'] = len(phonemes)
        model_config['n_mels'] = config['dsp']['num_mels']
        return Tacotron(**model_config)

    @classmethod
    def from_checkpoint(cls, path: Union[Path, str]) -> 'Tacotron':
        checkpoint = torch.load(path, map_location=torch.device('cpu'), weights_only=True)
        model = Tacotron.from_config(checkpoint['config'])
        model.load_state_dict(checkpoint['model'])
        return model
