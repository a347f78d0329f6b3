"""Per-phase breakdown of the Tacotron decoder step (ftmi_taco_args.stamps): thread 0 of
workgroup 0 sums s_memtime deltas per phase over a B = 1, T = 120, 800-frame free-running
launch; the shares are scaled by the launch's event time to microseconds per step.

    python tools/taco_stamps.py [r] [out file]
"""
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

from forwardtacotron_amd.synthetic import default_config, load_synthetic, synthetic_tokens  # noqa: E402
from forwardtacotron_amd.tacotron import Tacotron  # noqa: E402

PHASES = ['prenet + its GRU input share', 'GRU cell, publish hA', 'acquire hA', 'query projection',
          'energies of own tokens, publish u', 'shadow: W_hh hA', 'acquire u', 'softmax, cum',
          'context', 'rnn_input rows, publish x; shadow: W_ih ctx', 'acquire x',
          'LSTM1 rows + cell, publish h1', 'acquire h1', 'x += h1, LSTM2 rows + cell; shadow: W_hh h1',
          'acquire h2', 'x += h2, mel rows, publish; shadow: W_hh h2', 'acquire frames, stop rule']

r = int(sys.argv[1]) if len(sys.argv) > 1 else 1
model = load_synthetic(Tacotron.from_config(default_config()), 0, 'tacotron').cuda().eval()
x = torch.from_numpy(synthetic_tokens(1, 120, seed=5)).cuda()
enc, enc_proj = model._encode(x)
for _ in range(2):
    st = torch.zeros(24, device='cuda', dtype=torch.int64)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    mel, attn, n = model.decoder.launch(enc, enc_proj, r, 800, -1e9, stamps=st)
    e1.record()
    torch.cuda.synchronize()
steps = int(n.item())
us = e0.elapsed_time(e1) * 1e3 / steps
v = st.cpu().double().numpy()[:len(PHASES)]
lines = [f'tacotron decoder, B=1 T=120 r={r}: {steps} steps, {us:.1f} us/step (launch event time)']
for name, c in zip(PHASES, v):
    lines.append(f'  {name:52s} {us * c / v.sum():6.2f} us  {100 * c / v.sum():5.1f} %')
text = '\n'.join(lines)
print(text)
if len(sys.argv) > 2:
    Path(sys.argv[2]).write_text(text + '\n')
