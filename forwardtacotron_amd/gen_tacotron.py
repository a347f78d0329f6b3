"""Tacotron synthesis CLI (reference: `gen_tacotron.py`) on the HIP path.

    python -m forwardtacotron_amd.gen_tacotron [--checkpoint taco.pt | --config config.yaml | --synthetic] \\
        [--input_phonemes "həloʊ wɜːld" | --input_tokens 12,40,7 | --sentences file] \\
        [--steps 1000] {griffinlim | melgan | wavernn [--voc_checkpoint voc.pt | --voc_synthetic]
                                                      [--target 11000] [--overlap 550]}

The reference's grammar (`gen_tacotron.py:41-56`): --input_text, --checkpoint, --config,
--steps, then the vocoder as a sub-command.  As in `gen_forward.py` here, raw text is refused
(the cleaner needs espeak) and phonemised / token input, --synthetic weights and --out are
added.  The mel the vocoder receives is the postnet output of `Tacotron.generate`
(`gen_tacotron.py:111`), whose decoder loop is one persistent launch.  Outputs:
`{out}/{i}_taco_{k}k_{vocoder}.wav` (`.mel` for melgan), written through this package's DSP /
WaveRNN.
"""
from __future__ import annotations

import argparse
from pathlib import Path
from typing import List, Optional, Sequence

import torch

from .gen_forward import load_wavernn, read_inputs, synthetic_wavernn, write_output

VOCODERS = ('griffinlim', 'wavernn', 'melgan')


def load_taco(checkpoint_path: str):
    """`gen_tacotron.py:17-24` (weights_only load: nothing in the file is executed)."""
    from .tacotron import Tacotron
    print(f'Loading tts checkpoint {checkpoint_path}')
    checkpoint = torch.load(checkpoint_path, map_location=torch.device('cpu'), weights_only=True)
    config = checkpoint['config']
    tts_model = Tacotron.from_config(config)
    tts_model.load_state_dict(checkpoint['model'])
    print(f'Loaded taco with step {tts_model.get_step()}')
    return tts_model, config


def synthetic_taco():
    from .synthetic import default_config, load_synthetic
    from .tacotron import Tacotron
    config = default_config()
    return load_synthetic(Tacotron.from_config(config), 0, 'tacotron'), config


def wav_name(i: int, tts_k: int, vocoder: str) -> str:
    """`gen_tacotron.py:109`."""
    return f'{i}_taco_{tts_k}k_{vocoder}'


def checkpoint_from_config(config_path: str) -> Path:
    """`gen_tacotron.py:60-64`: without --checkpoint, checkpoints/{tts_model_id}.tacotron/
    latest_model.pt under the directory the CLI runs from (read with yaml.safe_load)."""
    import yaml
    with open(config_path, 'r', encoding='utf-8') as f:
        config = yaml.safe_load(f)
    return Path.cwd() / 'checkpoints' / f"{config['tts_model_id']}.tacotron" / 'latest_model.pt'


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description='TTS Generator (Tacotron, MI355X HIP path)')
    parser.add_argument('--input_text', '-i', default=None, type=str,
                        help='[string] raw text (refused: needs the espeak text frontend)')
    parser.add_argument('--input_phonemes', default=None, type=str,
                        help='phonemised sentence (what the reference cleaner produces)')
    parser.add_argument('--input_tokens', default=None, type=str, help='comma-separated token ids')
    parser.add_argument('--sentences', default='sentences.txt',
                        help='file of PHONEMISED sentences, one per line (raw text is refused)')
    parser.add_argument('--checkpoint', type=str, default=None,
                        help='[string/path] path to .pt model file.')
    parser.add_argument('--config', metavar='FILE', default='config.yaml',
                        help='The config containing all hyperparams. Only used if no checkpoint is set.')
    parser.add_argument('--steps', type=int, default=1000, help='Max number of steps.')
    parser.add_argument('--synthetic', action='store_true', help='synthetic weights, no checkpoint')
    parser.add_argument('--out', default='model_outputs')
    subparsers = parser.add_subparsers(dest='vocoder')
    wr_parser = subparsers.add_parser('wavernn')
    wr_parser.add_argument('--overlap', '-o', default=550, type=int,
                           help='[int] number of crossover samples')
    wr_parser.add_argument('--target', '-t', default=11_000, type=int,
                           help='[int] number of samples in each batch index')
    wr_parser.add_argument('--voc_checkpoint', type=str,
                           help='[string/path] Load in different WaveRNN weights')
    wr_parser.add_argument('--voc_synthetic', action='store_true', help='synthetic WaveRNN weights')
    subparsers.add_parser('griffinlim')
    subparsers.add_parser('melgan')
    return parser


def main(argv: Optional[Sequence[str]] = None) -> List[Path]:
    args = build_parser().parse_args(argv)
    if args.vocoder not in VOCODERS:  # gen_tacotron.py:57-58
        raise SystemExit("Please provide a valid vocoder! Choices: ['griffinlim', 'wavernn', 'melgan']")
    texts = read_inputs(args)  # refuses raw text before anything is loaded
    if args.synthetic:
        tts_model, config = synthetic_taco()
    else:
        tts_model, config = load_taco(str(args.checkpoint or checkpoint_from_config(args.config)))
    from .dsp import DSP
    dsp = DSP.from_config(config)
    voc = None
    if args.vocoder == 'wavernn':
        if args.voc_synthetic:
            voc_model, voc_config = synthetic_wavernn()
        elif args.voc_checkpoint:
            voc_model, voc_config = load_wavernn(args.voc_checkpoint)
        else:
            raise SystemExit('wavernn: --voc_checkpoint (or --voc_synthetic) is required')
        voc = (voc_model, DSP.from_config(voc_config))
    out_path = Path(args.out)
    out_path.mkdir(parents=True, exist_ok=True)
    if not torch.cuda.is_available():
        raise SystemExit('the HIP path needs a GPU (there is no CPU fallback)')
    device = torch.device('cuda')
    tts_model.to(device)
    if voc is not None:
        voc[0].to(device)
    tts_k = tts_model.get_step() // 1000
    written = []
    for i, ids in enumerate(texts, 1):
        print(f'\n| Generating {i}/{len(texts)}')
        x = torch.as_tensor(ids, dtype=torch.long, device=device).unsqueeze(0)
        _, m, _ = tts_model.generate(x=x, steps=args.steps)
        m = torch.tensor(m).unsqueeze(0)  # gen_tacotron.py:113,116: the postnet output
        written.append(write_output(m, wav_name(i, tts_k, args.vocoder), args.vocoder, out_path, dsp,
                                    voc, getattr(args, 'target', 11000), getattr(args, 'overlap', 550)))
    print('\n\nDone.\n')
    return written


if __name__ == '__main__':
    main()
