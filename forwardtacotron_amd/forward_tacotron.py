"""ForwardTacotron (V2: pitch + energy) on MI355X — drop-in for `models/forward_tacotron.py`.

Same constructor keywords (:93-118), same state_dict keys and shapes (checkpoints from the
reference load unchanged), same ``generate`` / ``generate_jit`` / ``forward`` /
``from_config`` / ``from_checkpoint`` / ``get_step`` surface and return dictionaries.
All math runs in libftmi.so (HIP, gfx950, fp32); torch only allocates device buffers,
moves tokens / results and runs the user's pitch / energy callbacks.

Pipeline of ``generate`` (channels-last activations, one HIP stream):
  predictors  embed -> 3x conv k5 (ReLU, BN) -> GRU in-proj GEMM -> GRU recurrence -> head
  durations   fill-2 rule + clip + counts + scan in one kernel (bit-exact), one host sync
              for T_mel (the reference syncs at the same point, :254 and common_layers.py:16)
  encoder     embed -> CBHG(K=16) -> + pitch/energy conv projections
  decoder     LSTM input projection at PHONEME rate (x W_ih^T + b), the recurrence reads
              it through the LengthRegulator index map: LR(x) W_ih^T == LR(x W_ih^T), so the
              expanded (B, T_mel, 512) tensor and 7x of the projection FLOPs are never needed;
              lin (-> mel, written both channels-last and as (B, 80, T_mel))
  postnet     CBHG(K=8) on the channels-last mel -> post_proj (-> mel_post (B, 80, T_mel))
"""
from __future__ import annotations

import os
from pathlib import Path
from typing import Any, Callable, Dict, Union

import numpy as np
import torch
import torch.nn as nn

from . import _lib, chain, ops, phase_graph
from .common_layers import (CBHG, BatchNormConv, BiRNN, Conv1dParams, LengthRegulator,
                            LinearParams, Packed, cached_pack, check_device, pack_conv, pad_time,
                            series_proj_weights)
from .phase_graph import _graphable, _identity, graph_safe  # noqa: F401  (public here)
from .text.symbols import phonemes


# generate() replays the phoneme phase as a HIP graph (captured per (device, x shape, alpha,
# callbacks), see phase_graph) when the phase is launch-bound: B*T <= GRAPH_MAX_TOKENS.
# Measured: c2 (B = 1, T = 120) 4.18 -> 3.57 ms/step; c3 (B = 64, T = 200) 9.20 -> 9.58, the
# replay loses the prenet stream's priority and the kernels are long enough to hide the host
# issue anyway.  FTMI_GRAPH=0, or GRAPH = False, keeps it eager.
GRAPH = os.environ.get('FTMI_GRAPH', '1') != '0'
GRAPH_MAX_TOKENS = int(os.environ.get('FTMI_GRAPH_MAX_TOKENS', 2048))


class Embedding(nn.Module):
    """Parameters of nn.Embedding(num, dim)."""

    def __init__(self, num: int, dim: int) -> None:
        super().__init__()
        self.num_embeddings, self.embedding_dim = num, dim
        self.weight = nn.Parameter(torch.randn(num, dim))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return ops.embedding(x, self.weight.detach())


class SeriesPredictor(Packed):
    """`models/forward_tacotron.py:14-55`: embed -> [Conv1d k5 -> ReLU -> BN]x3 -> biGRU ->
    Linear(2h -> 1) -> / alpha."""

    def __init__(self, num_chars, emb_dim=64, conv_dims=256, rnn_dims=64, dropout=0.5):
        super().__init__()
        self.embedding = Embedding(num_chars, emb_dim)
        self.convs = nn.ModuleList([
            BatchNormConv(emb_dim, conv_dims, 5, relu=True),
            BatchNormConv(conv_dims, conv_dims, 5, relu=True),
            BatchNormConv(conv_dims, conv_dims, 5, relu=True),
        ])
        self.rnn = BiRNN(conv_dims, rnn_dims, 'gru')
        self.lin = LinearParams(2 * rnn_dims, 1)
        self.dropout = dropout

    def _pack(self):
        return self.lin.weight.detach().reshape(-1).contiguous(), self.lin.bias.detach().contiguous()

    def forward_bt(self, x: torch.Tensor, alpha: float = 1.0) -> torch.Tensor:
        """(B, T) ids -> (B, T) series (before the reference's trailing unsqueeze): the whole
        chain as one launch list (chain.series_predictor; FTMI_CHAIN=0: a launch per op)."""
        if chain.CHAIN:
            return chain.series_predictor(self, x, alpha)
        return self._forward_ops(x, alpha)

    def _forward_ops(self, x: torch.Tensor, alpha: float = 1.0) -> torch.Tensor:
        """forward_bt one launch per op; also the pass a launch list is recorded from."""
        h = ops.embedding(x, self.embedding.weight.detach())
        for conv in self.convs:
            h = conv.forward_cl(h)
        h = self.rnn.forward_cl(h)
        w, b = self.packed_weights()
        return ops.rowdot(h, w, b, alpha)

    def forward_masked(self, ids: torch.Tensor, lengths: torch.Tensor,
                       alpha: float = 1.0) -> torch.Tensor:
        """_forward_ops for items of unequal length: (B, T) ids whose positions from
        lengths[b] on lie outside the table (zero embedded rows), lengths (B,) int32 on the
        device -> (B, T) series, on each item's valid positions what forward_bt gives for
        the item alone (the pad positions hold no defined value).  Convs 2 and 3 (k = 5)
        read two rows past an item's end: those rows of their inputs are zeroed, and the
        GRU takes the lengths."""
        h = ops.embedding(ids, self.embedding.weight.detach())
        for i, conv in enumerate(self.convs):
            h = conv.forward_cl(h)
            if i + 1 < len(self.convs):
                ops.fill_tail(h, lengths, reach=self.convs[i + 1].kernel // 2)
        h = self.rnn.forward_cl(h, lengths=lengths)
        w, b = self.packed_weights()
        return ops.rowdot(h, w, b, alpha)

    def forward(self, x: torch.Tensor, alpha: float = 1.0) -> torch.Tensor:
        """(B, T) -> (B, T, 1), like the reference."""
        return self.forward_bt(x, alpha).unsqueeze(-1)


PAD_ID = -1  # a pad position of a length-aware batch: outside every table, embeds to zero


def batch_plan(lengths, max_batch=None):
    """Chunk plan of generate_batch (host only).  lengths: the items' token counts, in input
    order.  Returns (chunks, inverse): chunks is a list of lists of input positions, each of
    at most max_batch items, taken from the items sorted by length (longest first, ties in
    input order) so a chunk pads little; max_batch=None is one chunk in input order.
    inverse[i] is the place of input item i in the concatenation of the chunks, so
    [flat[inverse[i]] for i in range(n)] restores input order."""
    n = len(lengths)
    if n == 0:
        raise ValueError('xs: no sequences given')
    if max_batch is None:
        chunks = [list(range(n))]
    else:
        if int(max_batch) < 1:
            raise ValueError(f'max_batch must be at least 1 (got {max_batch})')
        order = sorted(range(n), key=lambda i: (-int(lengths[i]), i))
        chunks = [order[i:i + int(max_batch)] for i in range(0, n, int(max_batch))]
    inverse = [0] * n
    for pos, i in enumerate(i for c in chunks for i in c):
        inverse[i] = pos
    return chunks, inverse


class ForwardTacotron(nn.Module):
    """ForwardTacotron V2; see module docstring.  Reference: models/forward_tacotron.py:74-350."""

    def __init__(self,
                 embed_dims: int,
                 series_embed_dims: int,
                 num_chars: int,
                 durpred_conv_dims: int,
                 durpred_rnn_dims: int,
                 durpred_dropout: float,
                 pitch_conv_dims: int,
                 pitch_rnn_dims: int,
                 pitch_dropout: float,
                 pitch_strength: float,
                 energy_conv_dims: int,
                 energy_rnn_dims: int,
                 energy_dropout: float,
                 energy_strength: float,
                 rnn_dims: int,
                 prenet_dims: int,
                 prenet_k: int,
                 postnet_num_highways: int,
                 prenet_dropout: float,
                 postnet_dims: int,
                 postnet_k: int,
                 prenet_num_highways: int,
                 postnet_dropout: float,
                 n_mels: int,
                 padding_value=-11.5129):
        # the constructor keywords, for the TorchScript archive (jit.model_config)
        ctor = {k: v for k, v in locals().items() if k not in ('self', '__class__')}
        super().__init__()
        self._ctor_kwargs = ctor
        self.rnn_dims = rnn_dims
        self.padding_value = padding_value
        self.register_buffer('step', torch.zeros(1, dtype=torch.long))
        # registration order follows the reference so state_dict() iterates identically
        self.embedding = Embedding(num_chars, embed_dims)
        self.prenet = CBHG(K=prenet_k, in_channels=embed_dims, channels=prenet_dims,
                           proj_channels=[prenet_dims, embed_dims],
                           num_highways=prenet_num_highways, dropout=prenet_dropout)
        self.pitch_pred = SeriesPredictor(num_chars, series_embed_dims, pitch_conv_dims,
                                          pitch_rnn_dims, pitch_dropout)
        self.energy_pred = SeriesPredictor(num_chars, series_embed_dims, energy_conv_dims,
                                           energy_rnn_dims, energy_dropout)
        self.pitch_proj = Conv1dParams(1, 2 * prenet_dims, 3, bias=True)
        self.energy_proj = Conv1dParams(1, 2 * prenet_dims, 3, bias=True)
        self.pitch_strength = pitch_strength
        self.energy_strength = energy_strength
        self.lr = LengthRegulator()
        self.dur_pred = SeriesPredictor(num_chars, series_embed_dims, durpred_conv_dims,
                                        durpred_rnn_dims, durpred_dropout)
        self.lstm = BiRNN(2 * prenet_dims, rnn_dims, 'lstm')
        self.lin = LinearParams(2 * rnn_dims, n_mels)
        self.postnet = CBHG(K=postnet_k, in_channels=n_mels, channels=postnet_dims,
                            proj_channels=[postnet_dims, n_mels],
                            num_highways=postnet_num_highways, dropout=postnet_dropout)
        self.post_proj = LinearParams(2 * postnet_dims, n_mels, bias=False)
        self.n_mels = n_mels
        # the decoder-side recurrences run alone on the device: they may spread over every
        # CU (the phoneme phase's four GRUs share it and keep the compact form)
        self.lstm.spread = self.postnet.rnn.spread = True

    def __repr__(self):
        num_params = sum([np.prod(p.size()) for p in self.parameters()])
        return f'ForwardTacotron, num params: {num_params}'

    # ---------------------------------------------------------------------------------
    def _check_device(self, x=None) -> None:
        check_device(self.embedding.weight, x, 'forwardtacotron_amd.ForwardTacotron')

    def _folded_series_weights(self):
        """The pitch / energy projections carried through the LSTM's input projection:
        W_ih (enc + ps proj_p(pitch) + es proj_e(energy)) + b
          = (W_ih enc + b) + ps (W_ih W_p * pitch + W_ih b_p) + es (W_ih W_e * energy + W_ih b_e),
        so the projection of enc can start as soon as the prenet ends and the predictors'
        outputs are added to its (B, T, 4H) rows afterwards (the same series_proj_add kernel
        with 4H-wide weights).  Made once per weights version, in float64."""
        pp, ep = self.pitch_proj, self.energy_proj

        def build():
            w_ih = self.lstm.packed_weights().w_ih.double()  # [2*4H][In], both directions
            out = []
            for w, b in (pp.weight, pp.bias), (ep.weight, ep.bias):
                out.append((w_ih @ w.detach().double().reshape(-1, 3)).float().contiguous())
                out.append((w_ih @ b.detach().double()).float().contiguous())
            return tuple(out)
        return cached_pack(self.lstm, '_ftmi_fold', build, (
            pp.weight._version, pp.bias._version, ep.weight._version, ep.bias._version,
            pp.weight.data_ptr(), ep.weight.data_ptr()))

    def _add_series(self, h, pitch, energy, folded=True) -> None:
        """h += pitch_strength proj_p(pitch) + energy_strength proj_e(energy), in place.
        folded: h holds LSTM input projection rows (_folded_series_weights), not prenet rows."""
        wp, bp, we, be = (self._folded_series_weights() if folded
                          else series_proj_weights(self.pitch_proj, self.energy_proj))
        ops.series_proj_add(h, pitch, wp, bp, self.pitch_strength, energy, we, be,
                            self.energy_strength)

    def _encode(self, x: torch.Tensor, pitch: torch.Tensor, energy: torch.Tensor) -> torch.Tensor:
        """embedding -> prenet CBHG -> + pitch / energy projections: (B, T, 2*prenet_dims)."""
        h = ops.embedding(x, self.embedding.weight.detach())
        h = self.prenet.forward_cl(h)
        self._add_series(h, pitch, energy, folded=False)
        return h

    def _decode(self, xp: torch.Tensor, index: torch.Tensor, *, lengths=None, pad_value=None,
                item_frames=None):
        """The decoder tail on xp, the LSTM input projection at phoneme rate: the LSTM reads
        it through the LR index map -> lin -> postnet -> post_proj.  lengths / pad_value
        (default padding_value): the recurrence's.  item_frames: the per-item frame totals
        of a length-aware batch ((B,) int32 on the device): the rows past an item's end are
        filled where a conv would read them or the caller sees them (ops.fill_tail) and the
        postnet takes the lengths; None: exactly the launches without them."""
        B, T_mel, dev = xp.size(0), index.size(1), xp.device
        lstm_out = self.lstm.recur(xp, T=T_mel, index=index, lengths=lengths,
                                   pad_value=self.padding_value if pad_value is None else pad_value)
        del xp
        mel_cl = torch.empty(B, T_mel, self.n_mels, device=dev)
        mel = torch.empty(B, self.n_mels, T_mel, device=dev)
        w, b, w3 = self.lin.packed_weights()
        ops.conv1d(lstm_out, w, 1, 0, bias=b, out=mel_cl, out_t=mel, w_split=w3)
        del lstm_out
        if item_frames is not None:  # mel_cl: the postnet bank's input and residual
            ops.fill_tail(mel_cl, item_frames, reach=self.postnet.K // 2)
            ops.fill_tail(mel, item_frames, value=self.padding_value, time_last=True)
        post = self.postnet.forward_cl(mel_cl, lengths=item_frames)
        mel_post = torch.empty(B, self.n_mels, T_mel, device=dev)
        w, _, w3 = self.post_proj.packed_weights()
        ops.conv1d(post, w, 1, 0, out_t=mel_post, want_y=False, w_split=w3)
        if item_frames is not None:
            ops.fill_tail(mel_post, item_frames, value=self.padding_value, time_last=True)
        return mel, mel_post

    # ---------------------------------------------------------------------------------
    def forward(self, batch: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """Teacher-forced pass (`models/forward_tacotron.py:184-242`), inference numerics."""
        x = batch['x']
        self._check_device(x)
        if self.training:
            self.step += 1
        return ops.run_checked(lambda: self._forward(batch), x.device)

    def _forward(self, batch: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        x = batch['x']
        mel = batch['mel']
        mel_lens = batch['mel_len']
        dur = batch['dur']
        pitch = batch['pitch'].unsqueeze(1)
        energy = batch['energy'].unsqueeze(1)
        with torch.no_grad():
            dur_hat = self.dur_pred.forward_bt(x)
            pitch_hat = self.pitch_pred.forward_bt(x).unsqueeze(1)
            energy_hat = self.energy_pred.forward_bt(x).unsqueeze(1)
            enc = self._encode(x, pitch, energy)
            dur_c = dur.float().contiguous()
            offsets, totals, _ = ops.duration_counts(dur_c, apply_fill=False)
            if dur_c.data_ptr() != dur.data_ptr():
                dur.copy_(dur_c)  # the reference's LR clips batch['dur'] in place
            lens = mel_lens.to(torch.int64)
            T_pack = int(lens.max().item())
            if T_pack > int(totals.max().item()):
                raise RuntimeError('mel_len exceeds the length-regulated sequence length')
            index = ops.lr_index(offsets, T_pack)
            lens = lens.to(x.device)
            x_mel, x_post = self._decode(self.lstm.project(enc), index, lengths=lens)
            x_post = self._pad(x_post, mel.size(2))
            x_mel = self._pad(x_mel, mel.size(2))
        return {'mel': x_mel, 'mel_post': x_post,
                'dur': dur_hat, 'pitch': pitch_hat, 'energy': energy_hat}

    def _side_streams(self, device, B: int, T: int = 0):
        """(pitch, energy, prenet) streams.  The prenet CBHG -> LSTM input projection is the
        phoneme phase's critical chain: its stream gets the higher priority
        (FTMI_PRENET_PRIORITY, default -1 = high; 0 = same as the others), so the
        predictors fill the CUs it leaves idle instead of delaying it.
        The four recurrences of the phase (three predictor GRUs, the prenet GRU) are
        persistent kernels whose workgroups wait on each other: run concurrently they must
        fit the CUs together.  The prenet stream's two persistent kernels — the spread CBHG
        tail at few rows (ops.hs_spread_blocks: its workgroups wait on each other too), then
        the prenet GRU — run one after the other, so the larger of them counts beside the
        predictors' three.  When they do not fit (large batches), every stream is the
        caller's (the phase runs serialised) — never a co-residency timeout."""
        cache = self.__dict__.setdefault('_ftmi_streams', {})
        if device not in cache:
            prio = int(os.environ.get('FTMI_PRENET_PRIORITY', '-1'))
            cache[device] = [torch.cuda.Stream(device=device), torch.cuda.Stream(device=device),
                             torch.cuda.Stream(device=device, priority=prio)]
        fits = self.__dict__.setdefault('_ftmi_concurrent', {})
        key = (device, B, T, ops.RNN_MMA, bool(ops._FORCED), os.environ.get('FTMI_HS_SPREAD', '1'),
               _lib.load().ftmi_rnn_switches_digest())  # ops.rnn_blocks reads those switches
        if key not in fits:
            preds = (self.dur_pred.rnn, self.pitch_pred.rnn, self.energy_pred.rnn)
            need = sum(ops.rnn_blocks(r.cell, B, r.hidden) for r in preds)
            # the prenet stream's persistent kernels (the spread CBHG tail, then the prenet
            # GRU) run one after the other on it: the larger of the two beside the predictors.
            # The spread tail counts only where it would run (the fused stack applies and
            # spreads at this row count); where predictors + spread tail would not fit, the
            # tail takes the one-workgroup-per-64-rows stack kernel (nothing to co-schedule)
            # and the phase stays concurrent (~900 prenet rows)
            pre = ops.rnn_blocks(self.prenet.rnn.cell, B, self.prenet.rnn.hidden)
            spread = self.prenet.spread_blocks(B * T)
            cus = ops._num_cus()
            use_spread = spread > 0 and need + max(pre, spread) <= cus
            fits[key] = (0 < need + pre <= cus and pre > 0, use_spread)
        concurrent, use_spread = fits[key]
        self.prenet.allow_spread = use_spread
        if not concurrent:
            main = torch.cuda.current_stream(device)
            return [main, main, main]
        return cache[device]

    def _phoneme_phase(self, x, alpha, pitch_fn, energy_fn, batch=None, capture=False):
        """Duration / pitch / energy predictors and the prenet CBHG are independent: pitch,
        energy and the prenet run on three side streams while the caller's stream runs the
        duration predictor and the LengthRegulator bookkeeping (fill-2 rule, counts, T_mel).
        The prenet stream (high priority: its chain is the phase's critical path) continues
        with the LSTM input projection of the prenet output (independent of the predictors)
        and then, after the pitch / energy streams, adds their projections through W_ih:
        none of it depends on T_mel, so it runs while the duration path finishes and the
        host waits for T_mel (the one host sync, a pinned copy queued right after the
        duration kernel).  Issue order = priority order: prenet, durations, pitch,
        energy.  Returns a phase_graph.Phase with every tensor ready on the caller's stream
        (h: the LSTM input projection of the prenet output plus the pitch / energy
        projections, folded through W_ih; the prenet output itself is last read on the
        prenet stream and freed there; index: the LR index map, queued on the caller's
        stream before it joins the side streams).  capture=True (graph capture, see
        phase_graph): no host sync, t_mel holds max(totals) on the device and index None.
        pitch_fn = energy_fn = None (capture only): the predictors' raw outputs are returned
        and h does not carry their projections yet (the split graph of phase_graph)."""
        main = torch.cuda.current_stream(x.device)
        s_pitch, s_energy, s_prenet = self._side_streams(x.device, x.size(0), x.size(1))
        for s in (s_pitch, s_energy, s_prenet):
            s.wait_stream(main)
        with torch.cuda.stream(s_prenet):
            enc = self.prenet.forward_ids(x, self.embedding.weight)
            # the LSTM input projection right after the prenet; the pitch / energy terms are
            # added to its rows once the predictors are done (_folded_series_weights)
            xp = self.lstm.project(enc)
        dur_hat = self.dur_pred.forward_bt(x, alpha=alpha)
        t_host = t_ready = None
        if batch is None:
            offsets, totals, _ = ops.duration_counts(dur_hat, apply_fill=True)
            T_mel = totals.max()
            if not capture:
                # the one host sync (output size is data dependent): max(totals) goes to pinned
                # host memory now and is read after the T_mel-independent work is queued
                t_host = torch.empty((), dtype=totals.dtype, pin_memory=True)
                t_host.copy_(T_mel, non_blocking=True)
                t_ready = torch.cuda.Event()
                t_ready.record(main)
        with torch.cuda.stream(s_pitch):
            pitch_hat = self.pitch_pred.forward_bt(x).unsqueeze(1)
            if pitch_fn is not None:
                pitch_hat = pitch_fn(pitch_hat)
        with torch.cuda.stream(s_energy):
            energy_hat = self.energy_pred.forward_bt(x).unsqueeze(1)
            if energy_fn is not None:
                energy_hat = energy_fn(energy_hat)
        if pitch_fn is not None and energy_fn is not None:
            with torch.cuda.stream(s_prenet):
                for s, t in ((s_pitch, pitch_hat), (s_energy, energy_hat)):
                    s_prenet.wait_stream(s)
                    if not capture:
                        t.record_stream(s_prenet)
                self._add_series(xp, pitch_hat, energy_hat)
        if batch is not None:  # a shard of a larger batch (sharded.GlobalBatch): batch-global
            offsets, totals = batch.duration_counts(dur_hat)  # fill rule / T_mel
            T_mel = batch.t_mel(totals)
        index = None
        if not capture:
            if t_ready is not None:
                t_ready.synchronize()
                T_mel = int(t_host)
            # the LR index map only needs the durations: queued before the caller's stream
            # joins the side streams, so it is not held behind the prenet chain's tail
            index = ops.lr_index(offsets, T_mel)
        for s, t in ((s_pitch, pitch_hat), (s_energy, energy_hat), (s_prenet, xp)):
            main.wait_stream(s)
            if not capture:
                t.record_stream(main)
        return phase_graph.Phase(dur_hat, pitch_hat, energy_hat, xp, offsets, T_mel, index)

    def _generate(self, x, alpha, pitch_fn, energy_fn, batch=None, graph=False):
        """The run body of generate / generate_jit under the f16x3 range guard: phoneme phase
        (from its graph where `graph` says so) -> decoder tail -> the reference's dictionary."""
        def finish(ph):  # what a split graph leaves out: the projections, folded through W_ih
            self._add_series(ph.h, ph.pitch, ph.energy)

        def run():
            with torch.no_grad():
                phase, consumed = phase_graph.phoneme_phase(
                    self, self._phoneme_phase, finish, (ops.MMA, ops.RNN_MMA), x, alpha,
                    pitch_fn, energy_fn, batch, graph and not ops.forced_exact())
                index = phase.index
                if index is None:  # a replayed phase: T_mel was not known inside the graph
                    index = ops.lr_index(phase.offsets, phase.t_mel)
                mel, mel_post = self._decode(phase.h, index)
                consumed()  # the decoder is queued: the graph's static buffers may be rewritten
                return {'mel': mel, 'mel_post': mel_post, 'dur': phase.dur,
                        'pitch': phase.pitch, 'energy': phase.energy}
        return ops.run_checked(run, x.device, reduce=None if batch is None else batch.status)

    def generate(self,
                 x: torch.Tensor,
                 alpha=1.0,
                 pitch_function: Callable[[torch.Tensor], torch.Tensor] = _identity,
                 energy_function: Callable[[torch.Tensor], torch.Tensor] = _identity,
                 batch=None) -> Dict[str, torch.Tensor]:
        """`models/forward_tacotron.py:244-268`.  The callbacks run on the stream of their
        predictor (torch ops issued inside them are ordered after the prediction).
        `batch`: a sharded.GlobalBatch when x is one rank's shard of a larger batch.
        Runs under the f16x3 range guard (ops.run_checked): one status read at the end."""
        if self.training:  # the module-tree walk of eval() is host time on every call
            self.eval()
        self._check_device(x)

        # only callbacks known to be pure are captured (graph_safe): a replay would freeze any
        # Python-side state an arbitrary callback reads; any other callback runs eagerly
        # between the captured predictors and the launch that consumes its output
        graph = GRAPH and batch is None and x.numel() <= GRAPH_MAX_TOKENS
        return self._generate(x, alpha, pitch_function, energy_function, batch, graph)

    # ---------------------------------------------------------------------------------
    # length-aware batches: each item's result is that of generate() on the item alone

    def _masked_pass(self, ids, lens, alpha, pitch_fn, energy_fn):
        """One length-aware pass.  ids: (B, T) int64 on the device, PAD_ID
        from lens[b] on; lens: (B,) int32 on the device.  Every item starts at row 0 of its
        batch row, so the existing kernels give its left edge; at its right edge the rows a
        conv reads past the end are zeroed (ops.fill_tail), the recurrences take the lengths,
        and the duration rules are decided per item.  One launch per op, all on the caller's
        stream (no side streams: nothing to co-schedule).  Returns (dict, totals on the
        host); the one host sync is the copy of the totals."""
        dev = ids.device
        B = ids.size(0)
        dur = self.dur_pred.forward_masked(ids, lens, alpha)
        offsets, totals, _ = ops.duration_counts_rows(dur, lens)
        t_host = torch.empty(B, dtype=torch.int32, pin_memory=True)
        t_host.copy_(totals, non_blocking=True)
        t_ready = torch.cuda.Event()
        t_ready.record(torch.cuda.current_stream(dev))
        series = []
        for pred, fn in ((self.pitch_pred, pitch_fn), (self.energy_pred, energy_fn)):
            s = pred.forward_masked(ids, lens).unsqueeze(1)
            ops.fill_tail(s, lens, time_last=True)  # the callback sees zero pads ...
            s = fn(s)
            if s.dtype != torch.float32 or not s.is_contiguous():
                s = s.float().contiguous()
            ops.fill_tail(s, lens, time_last=True)  # ... and whatever it wrote there goes
            series.append(s)
        pitch, energy = series
        enc = self.prenet.forward_ids(ids, self.embedding.weight, lengths=lens)
        xp = self.lstm.project(enc)
        del enc
        self._add_series(xp, pitch, energy)
        t_ready.synchronize()
        tot = t_host.clone()
        index = ops.lr_index(offsets, int(tot.max()))
        # the decoder of forward(): frames past an item's total are skipped by the LSTM (zero
        # rows, so lin leaves its bias there, not lin(padding_value))
        mel, mel_post = self._decode(xp, index, lengths=totals, pad_value=0.0, item_frames=totals)
        return {'mel': mel, 'mel_post': mel_post, 'dur': dur, 'pitch': pitch,
                'energy': energy, 'mel_len': tot.to(torch.int64)}, tot

    def _run_masked(self, ids, lens, alpha, pitch_fn, energy_fn):
        """_masked_pass under the f16x3 range guard.  The rows past an item's halo hold
        finite values nobody reads for a valid row; they still pass through the f16x3 GEMMs
        and may set the range bit, and the pass then runs again on the fp32 paths."""
        if self.training:
            self.eval()

        def run():
            with torch.no_grad():
                return self._masked_pass(ids, lens, alpha, pitch_fn, energy_fn)
        return ops.run_checked(run, ids.device)

    def generate_masked(self,
                        x: torch.Tensor,
                        x_len,
                        alpha=1.0,
                        pitch_function: Callable[[torch.Tensor], torch.Tensor] = _identity,
                        energy_function: Callable[[torch.Tensor], torch.Tensor] = _identity
                        ) -> Dict[str, torch.Tensor]:
        """generate() of a padded batch whose items do not see each other or the padding.
        x: (B, T) int64 on the model's device; x_len: (B,) lengths in [1, T] (a tensor on
        either side or a sequence; read on the host).  Whatever x holds from x_len[b] on is
        ignored (an id 0 below x_len[b] is a real symbol).  Returns generate()'s dictionary
        for the batch plus 'mel_len' ((B,) int64 on the host: each item's frame count):
        item b's `mel` / `mel_post` frames below mel_len[b] and `dur` / `pitch` / `energy`
        positions below x_len[b] are what generate(x[b:b+1, :x_len[b]]) returns; past them
        mel / mel_post hold padding_value and dur / pitch / energy hold 0.
        The callbacks get the padded (B, 1, T) series once, pads zeroed before the call and
        again after it; equality with the item alone is promised for elementwise callbacks."""
        if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.size(0) < 1 or x.size(1) < 1:
            raise ValueError('x: a (B, T) tensor of token ids is expected, got '
                             + (f'shape {tuple(x.shape)}' if isinstance(x, torch.Tensor)
                                else type(x).__name__))
        B, T = x.shape
        lens = torch.as_tensor(x_len.cpu() if isinstance(x_len, torch.Tensor) else x_len)
        if lens.dim() != 1 or lens.numel() != B:
            raise ValueError(f'x_len: {B} lengths expected for x of shape {(B, T)}, got shape '
                             f'{tuple(lens.shape)}')
        if lens.is_floating_point() or int(lens.min()) < 1 or int(lens.max()) > T:
            raise ValueError(f'x_len: integer lengths in [1, T = {T}] expected, got '
                             f'{lens.tolist()}')
        if not x.is_cuda:
            raise RuntimeError('x: generate_masked runs on a HIP device only (got a CPU '
                               'tensor); there is no CPU path')
        self._check_device(x)
        lens = lens.to(torch.int32).to(x.device)
        pad = torch.arange(T, device=x.device).unsqueeze(0) >= lens.unsqueeze(1)
        ids = x.long().masked_fill(pad, PAD_ID)
        return self._run_masked(ids, lens, alpha, pitch_function, energy_function)[0]

    def generate_batch(self,
                       xs,
                       alpha=1.0,
                       pitch_function: Callable[[torch.Tensor], torch.Tensor] = _identity,
                       energy_function: Callable[[torch.Tensor], torch.Tensor] = _identity,
                       max_batch=None):
        """Synthesise many sentences of unequal length in shared launches.  xs: a list of 1-D
        token tensors or int lists.  Returns a list of dictionaries in input order, item i's
        the one generate(x_i[None]) returns — 'mel' / 'mel_post' (1, n_mels, T_mel_i), 'dur'
        (1, L_i), 'pitch' / 'energy' (1, 1, L_i) — each tensor with storage of its own.
        max_batch: items are sorted by length and run in chunks of at most that many
        (batch_plan; results do not depend on batch-mates, so the order is free).  The
        callbacks run once per chunk, see generate_masked."""
        if isinstance(xs, torch.Tensor) or not hasattr(xs, '__len__'):
            raise ValueError('xs: a list of 1-D token sequences is expected')
        if len(xs) == 0:
            raise ValueError('xs: no sequences given')
        seqs = []
        for i, s in enumerate(xs):
            a = np.asarray(s.detach().cpu() if isinstance(s, torch.Tensor) else s)
            if a.ndim != 1 or a.size == 0:
                raise ValueError(f'xs[{i}]: a non-empty 1-D token sequence is expected, got '
                                 f'shape {a.shape}')
            if a.dtype.kind not in 'iu':
                raise ValueError(f'xs[{i}]: integer token ids expected, got {a.dtype}')
            seqs.append(a.astype(np.int64))
        chunks, inverse = batch_plan([a.size for a in seqs], max_batch)
        self._check_device()
        dev = self.embedding.weight.device
        flat = []
        for chunk in chunks:
            lens = [seqs[i].size for i in chunk]
            ids = np.full((len(chunk), max(lens)), PAD_ID, dtype=np.int64)
            for r, i in enumerate(chunk):
                ids[r, :lens[r]] = seqs[i]
            out, tot = self._run_masked(torch.from_numpy(ids).to(dev),
                                        torch.tensor(lens, dtype=torch.int32).to(dev), alpha,
                                        pitch_function, energy_function)
            for r, L in enumerate(lens):
                F = int(tot[r])
                flat.append({'mel': out['mel'][r:r + 1, :, :F].clone(),
                             'mel_post': out['mel_post'][r:r + 1, :, :F].clone(),
                             'dur': out['dur'][r:r + 1, :L].clone(),
                             'pitch': out['pitch'][r:r + 1, :, :L].clone(),
                             'energy': out['energy'][r:r + 1, :, :L].clone()})
        return [flat[p] for p in inverse]

    def __prepare_scriptable__(self):
        """`torch.jit.script(model)` (the reference's export, README.md:149-161): the compute
        runs in libftmi.so through ctypes, which TorchScript cannot compile, so what gets
        scripted is `jit.ScriptedForwardTacotron` — the reference's scriptable surface
        (`forward(batch)`, `generate_jit(x, alpha, beta)`) over dispatcher operators
        (`torch.ops.ftmi.*`) that run this model's HIP path.  The scripted module carries the
        constructor keywords and the weights, so a torch.jit.save'd archive loads and runs
        in any process that has imported forwardtacotron_amd."""
        from .jit import ScriptedForwardTacotron
        return ScriptedForwardTacotron(self)

    def generate_jit(self, x: torch.Tensor, alpha: float = 1.0, beta: float = 1.0) -> Dict[str, torch.Tensor]:
        """`models/forward_tacotron.py:270-284` (pitch scaled by beta, no callbacks)."""
        self._check_device(x)
        return self._generate(x, alpha, lambda p: p * beta, lambda e: e)

    def get_step(self) -> int:
        return self.step.data.item()

    def _pad(self, x: torch.Tensor, max_len: int) -> torch.Tensor:
        """`models/forward_tacotron.py:332-335` (crop / pad the time axis with padding_value)."""
        return pad_time(x, max_len, self.padding_value)

    @classmethod
    def from_config(cls, config: Dict[str, Any]) -> 'ForwardTacotron':
        model_config = config['forward_tacotron']['model']
        model_config['num_chars'] = len(phonemes)
        model_config['n_mels'] = config['dsp']['num_mels']
        return ForwardTacotron(**model_config)

    @classmethod
    def from_checkpoint(cls, path: Union[Path, str]) -> 'ForwardTacotron':
        checkpoint = torch.load(path, map_location=torch.device('cpu'), weights_only=True)
        model = ForwardTacotron.from_config(checkpoint['config'])
        model.load_state_dict(checkpoint['model'])
        return model
