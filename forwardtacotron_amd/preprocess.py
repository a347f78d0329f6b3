"""`preprocess.py` (reference) on libftmi.so: wav files -> the mel and vocoder-label files every
later stage reads.

    python -m forwardtacotron_amd.preprocess --path WAVDIR --out DIR --config FILE [--batch N]

Every ``*.wav`` under WAVDIR goes through ``DSP.prepare_batch`` (start / end silence trim, peak
rule, log-mel, labels: ``Preprocessor._convert_file`` of the reference, `preprocess.py:51-91`),
sorted by length and N files at a time.  Written, with the reference's names and dtypes
(``np.save(..., allow_pickle=False)``):

    DIR/mel/<id>.npy      float32 (n_mels, frames)
    DIR/quant/<id>.npy    int64 (samples,)
    DIR/dataset.json      [[id, frames], ...] sorted by id (the reference pickles this list
                          after a shuffle and a train / validation split, which need the
                          metadata file)

Not done here: the text side (cleaner, tokenizer, metadata: espeak is absent) and the raw
pitch track (pyworld's dio is absent); wavs must already be at the config's sample rate
(DSP.load_wav has no resampler).  CONFIG is the reference's YAML, or the same mapping as JSON.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path
from typing import Any, Dict, List, Optional, Tuple

import numpy as np
import torch

from .dsp import DSP


def read_config(path: str) -> Dict[str, Any]:
    text = Path(path).read_text(encoding='utf-8')
    if str(path).endswith('.json'):
        return json.loads(text)
    import yaml
    return yaml.safe_load(text)


def prepare_files(dsp: DSP, files: List[Path], out: Path, batch: int = 16,
                  device: str = 'cuda') -> List[Tuple[str, int]]:
    """Prepare `files` in batches of `batch` (sorted by length, so a batch's rows are padded
    little) and write DIR/mel, DIR/quant; returns [(id, mel frames)] sorted by id."""
    (out / 'mel').mkdir(parents=True, exist_ok=True)
    (out / 'quant').mkdir(parents=True, exist_ok=True)
    wavs = sorted(((dsp.load_wav(f), f.stem) for f in files), key=lambda t: (len(t[0]), t[1]))
    dataset = []
    for i in range(0, len(wavs), batch):
        chunk = wavs[i:i + batch]
        L = max(len(w) for w, _ in chunk)
        rows = np.zeros((len(chunk), L), dtype=np.float32)
        for b, (w, _) in enumerate(chunk):
            rows[b, :len(w)] = w
        lengths = torch.tensor([len(w) for w, _ in chunk], dtype=torch.int32)
        p = dsp.prepare_batch(torch.from_numpy(rows).to(device), lengths.to(device))
        n, fr = p.lengths.cpu().tolist(), p.frames.cpu().tolist()
        mel, quant = p.mel.cpu().numpy(), p.quant.cpu().numpy()
        for b, (_, wav_id) in enumerate(chunk):
            if n[b] < 1:
                raise ValueError(f'{wav_id}: nothing is left of the audio after the trim')
            np.save(out / 'mel' / f'{wav_id}.npy', np.ascontiguousarray(mel[b, :, :fr[b]]),
                    allow_pickle=False)
            np.save(out / 'quant' / f'{wav_id}.npy', np.ascontiguousarray(quant[b, :n[b]]),
                    allow_pickle=False)
            dataset.append((wav_id, fr[b]))
    dataset.sort()
    (out / 'dataset.json').write_text(json.dumps(dataset))
    return dataset


def main(argv: Optional[List[str]] = None) -> int:
    ap = argparse.ArgumentParser(description='Preprocessing for WaveRNN and Tacotron '
                                             '(MI355X HIP path: mel and labels)')
    ap.add_argument('--path', '-p', required=True, help='directory with the .wav files')
    ap.add_argument('--out', required=True, help='output directory (mel/, quant/, dataset.json)')
    ap.add_argument('--config', metavar='FILE', default='config.yaml',
                    help='the config containing all hyperparams')
    ap.add_argument('--batch', type=int, default=16, help='files per device batch')
    a = ap.parse_args(argv)
    if a.batch < 1:
        ap.error('--batch must be at least 1')
    files = sorted(Path(a.path).expanduser().resolve().rglob('*.wav'))
    if not files:
        print(f'Found no wav files in {a.path}, exiting.', file=sys.stderr)
        return 1
    stems = [f.stem for f in files]
    if len(set(stems)) != len(stems):
        print('two wav files share an id (file stem)', file=sys.stderr)
        return 1
    dsp = DSP.from_config(read_config(a.config))
    dataset = prepare_files(dsp, files, Path(a.out), a.batch)
    print(f'{len(dataset)} files -> {a.out} (mel/, quant/, dataset.json)')
    return 0


if __name__ == '__main__':
    sys.exit(main())
