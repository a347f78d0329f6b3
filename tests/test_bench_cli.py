"""bench.py's command line: a plain run prints the line of the timed steps alone, --full
gates every further measurement, --dump-outputs writes the last timed step's arrays."""
import json
import sys

import numpy as np
import pytest
import torch

import bench


def test_dump_outputs_types(tmp_path):
    arrays = {'mel': torch.arange(12, dtype=torch.float32).reshape(1, 3, 4),
              'dur': torch.tensor([[3, 0, 2 ** 40 + 1]]),
              'wav': np.linspace(0, 1, 7, dtype=np.float64),
              'half': torch.ones(5, dtype=torch.float16)}
    bench.dump_outputs(str(tmp_path / 'd'), arrays)
    got = {p.stem: np.load(p, allow_pickle=False) for p in (tmp_path / 'd').iterdir()}
    assert sorted(got) == sorted(arrays)
    assert got['mel'].dtype == np.float32 and got['mel'].shape == (1, 3, 4)
    assert got['dur'].dtype == np.float64 and got['dur'][0, 2] == 2 ** 40 + 1  # integers exact
    assert got['wav'].dtype == np.float64 and np.array_equal(got['wav'], arrays['wav'])
    assert got['half'].dtype == np.float32
    assert np.array_equal(got['mel'], arrays['mel'].numpy())


def test_dump_outputs_samples_within_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, 'DUMP_BUDGET', 4000)
    big = np.arange(5000, dtype=np.float32)
    small = np.arange(10, dtype=np.float32)
    for d in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / d), {'big': big, 'small': small})
    a, b = np.load(tmp_path / 'a' / 'big.npy'), np.load(tmp_path / 'b' / 'big.npy')
    assert np.array_equal(a, b)  # the same elements in every run
    assert np.array_equal(np.load(tmp_path / 'a' / 'small.npy'), small)  # within its share: whole
    assert a.nbytes + small.nbytes <= 4000 and a.size == 500
    assert np.all(np.diff(a) >= 0) and set(a) <= set(big)


@pytest.mark.parametrize('extra', [['--kernels'], ['--vocoder', 'griffinlim'], ['--steps', '0']])
def test_arguments_refused_before_any_gpu_work(extra, monkeypatch, capsys):
    monkeypatch.setattr(sys, 'argv', ['bench.py', *extra])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 2
    assert '--full' in capsys.readouterr().err or extra[0] == '--steps'


@pytest.mark.gpu
def test_plain_run_line_and_dump(tmp_path, monkeypatch, capsys):
    """c2 (batch 1, 120 phonemes), 3 timed steps: the line holds the headline fields and none
    of the --full measurements, and the dump is what generate() returned."""
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '1', '--config', 'c2', '--steps', '3',
                                      '--warmup', '1', '--dump-outputs', str(tmp_path / 'out')])
    bench.main()
    lines = [s for s in capsys.readouterr().out.splitlines() if s.startswith('{')]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line['steps'] == 3 and line['warmup'] == 1 and line['n_gpus'] == 1
    assert line['unit'] == 'mel-frames/s' and line['higher_is_better'] is True and line['dtype'] == 'fp32'
    assert line['ms_per_step'] > 0
    t_mel = line['config']['T_mel']
    # value and ms_per_step describe the same 3 steps (both rounded in the line)
    assert line['value'] == pytest.approx(t_mel / (line['ms_per_step'] / 1e3), rel=1e-3)
    for k in ('roofline', 'host_to_host', 'prenet_bank', 'cpu_baseline', 'parity', 'with_vocoder'):
        assert k not in line
    got = {p.stem: np.load(p, allow_pickle=False) for p in (tmp_path / 'out').iterdir()}
    assert {'mel', 'mel_post', 'dur'} <= set(got)
    assert got['mel_post'].shape == (1, 80, t_mel) and got['mel_post'].dtype == np.float32
    assert all(np.isfinite(a).all() for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= bench.DUMP_BUDGET
