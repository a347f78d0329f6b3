"""gen_forward --batch N: the sentences of a --sentences file synthesised together
(ForwardTacotron.generate_batch) give the files the one-at-a-time loop gives — the same
names in the original numbering, the same shapes, contents within the mel_post bounds of
tests/test_gpu_model.py.

The five lines tokenise to 27, 10, 46, 4 and 49 ids; under the torch-CPU oracle their frame
counts are 175, 75, 307, 33 and 313 and the smallest distance of dur + 0.5 from an integer is
0.0035 (350 x the duration tolerance), so the frame counts are decided."""
import numpy as np
import pytest

from test_gpu_model import MAX_TOL, MEAN_TOL

pytestmark = pytest.mark.gpu

LINES = ['həloʊ wɜːld, ðɪs ɪz ɐ tɛst.',
         'ʃɔːɹt wʌn.',
         'ðə kwɪk bɹaʊn fɑːks dʒʌmps oʊvɚ ðə leɪzi dɔːɡ!',
         'noʊ.',
         'wɪtʃ sɛntəns ɪz ðə lɔŋɡəst ʌv ɔːl faɪv, aɪ wʌndɚ?']
FRAMES = [175, 75, 307, 33, 313]


def test_batch_writes_what_the_loop_writes(tmp_path):
    from forwardtacotron_amd.gen_forward import main
    sentences = tmp_path / 'sentences.txt'
    sentences.write_text('\n'.join(LINES) + '\n', encoding='utf-8')
    written = {}
    for batch in (1, 3):
        out = tmp_path / f'batch{batch}'
        written[batch] = main(['--synthetic', '--sentences', str(sentences), '--out', str(out),
                               '--batch', str(batch), 'hifigan'])
    names = [f'{i}_forward_0k_alpha1.0_amp1.0_hifigan.npy' for i in range(1, len(LINES) + 1)]
    assert [p.name for p in written[1]] == names
    assert [p.name for p in written[3]] == names
    for a, b, frames in zip(written[1], written[3], FRAMES):
        ma, mb = np.load(a, allow_pickle=False), np.load(b, allow_pickle=False)
        assert ma.shape == mb.shape == (1, 80, frames), (a.name, ma.shape, mb.shape)
        d = np.abs(ma - mb)
        assert d.mean() < MEAN_TOL and d.max() < MAX_TOL, (a.name, d.mean(), d.max())
