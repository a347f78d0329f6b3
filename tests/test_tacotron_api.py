"""Tacotron's public surface without a GPU: checkpoint compatibility (state_dict keys and
shapes of the reference), the `r` property, from_config, the gen_tacotron CLI grammar and the
C ABI of the decoder launch (header, binding struct, host-side argument checks)."""
import ctypes
import json
import re
from pathlib import Path

import pytest
import torch

from conftest import GOLDEN
from forwardtacotron_amd import _lib, gen_tacotron
from forwardtacotron_amd.synthetic import default_config, load_synthetic
from forwardtacotron_amd.tacotron import Tacotron

HEADER = Path(__file__).resolve().parent.parent / 'include' / 'ftmi.h'


@pytest.fixture(scope='module')
def model():
    return Tacotron.from_config(default_config())


def test_state_dict_matches_reference(model):
    keys = json.loads((GOLDEN / 'tacotron_state_dict_keys.json').read_text())
    sd = model.state_dict()
    assert [[k, list(v.shape), str(v.dtype).replace('torch.', '')] for k, v in sd.items()] == keys
    have = {k: tuple(v.shape) for k, v in sd.items()}
    assert have['decoder.mel_proj.weight'] == (1600, 512)
    assert have['decoder.attn_net.conv.weight'] == (32, 2, 31)
    assert sd['decoder.r'].dtype == torch.int32 and sd['step'].dtype == torch.int64
    assert {'step', 'stop_threshold', 'decoder.r'} <= set(have)


def test_r_round_trips_through_state_dict(model):
    model.r = 5
    assert model.r == 5 and int(model.state_dict()['decoder.r']) == 5
    other = Tacotron.from_config(default_config())
    assert other.r == 1
    other.load_state_dict(model.state_dict())
    assert other.r == 5 and other.decoder.r.dtype == torch.int32
    model.r = 1


def test_from_config_fills_the_config_like_the_reference():
    cfg = default_config()
    assert 'num_chars' not in cfg['tacotron']['model']
    m = Tacotron.from_config(cfg)
    from forwardtacotron_amd.text.symbols import phonemes
    assert cfg['tacotron']['model']['num_chars'] == len(phonemes)
    assert cfg['tacotron']['model']['n_mels'] == cfg['dsp']['num_mels'] == 80
    assert float(m.stop_threshold) == -11.0 and m.get_step() == 0
    m.reset_step()
    assert m.get_step() == 1


def test_synthetic_recipe_sets_r_and_threshold():
    m = load_synthetic(Tacotron.from_config(default_config()), 0, 'tacotron')
    assert m.r == 1 and float(m.stop_threshold) == -11.0
    a = m.decoder.attn_net.v.weight.detach()
    b = load_synthetic(Tacotron.from_config(default_config()), 0, 'tacotron').decoder.attn_net.v.weight
    assert torch.equal(a, b)  # deterministic from the key names


def test_cpu_model_is_refused(model):
    with pytest.raises(RuntimeError, match='HIP device only'):
        model.generate(torch.ones(1, 4, dtype=torch.long), steps=4)


def test_cli_grammar_and_names():
    p = gen_tacotron.build_parser()
    a = p.parse_args(['--synthetic', '--input_tokens', '12,40,7', '--steps', '60', 'griffinlim'])
    assert a.vocoder == 'griffinlim' and a.steps == 60 and a.synthetic and a.input_tokens == '12,40,7'
    a = p.parse_args(['-i', 'Hello', '--checkpoint', 'x.pt', 'wavernn', '-o', '100', '-t', '2000',
                      '--voc_checkpoint', 'v.pt'])
    assert (a.input_text, a.checkpoint, a.vocoder, a.overlap, a.target) == ('Hello', 'x.pt', 'wavernn', 100, 2000)
    assert p.parse_args(['melgan']).steps == 1000 and p.parse_args(['melgan']).config == 'config.yaml'
    with pytest.raises(SystemExit):
        p.parse_args(['hifigan'])
    assert gen_tacotron.wav_name(3, 40, 'griffinlim') == '3_taco_40k_griffinlim'


def test_cli_refuses_raw_text_and_missing_vocoder():
    from forwardtacotron_amd.gen_forward import RAW_TEXT_HINT
    with pytest.raises(SystemExit) as e:
        gen_tacotron.main(['--synthetic', '--input_text', 'Hello world', 'griffinlim'])
    assert RAW_TEXT_HINT in str(e.value)
    with pytest.raises(SystemExit, match='valid vocoder'):
        gen_tacotron.main(['--synthetic', '--input_tokens', '1,2'])


def test_binding_struct_mirrors_header():
    text = re.sub(r'/\*.*?\*/', '', HEADER.read_text(), flags=re.S)
    body = re.search(r'typedef struct ftmi_taco_args \{(.*?)\} ftmi_taco_args;', text, re.S).group(1)
    names = [n.split()[-1].lstrip('*') for decl in body.split(';') if decl.strip()
             for n in decl.split(',')]
    assert names == [f[0] for f in _lib.TacoArgs._fields_]
    assert _lib.ABI_VERSION == 22
    from forwardtacotron_amd import ops
    lim = dict(re.findall(r'(FTMI_TACO_MAX_[A-Z]+) = (\d+)', text))
    assert (ops.TACO_MAX_TOKENS, ops.TACO_MAX_BATCH) == (int(lim['FTMI_TACO_MAX_TOKENS']), int(lim['FTMI_TACO_MAX_BATCH']))
    assert ops.TACO_MAX_TOKENS >= 400


def test_decoder_argument_errors():
    lib = _lib.load()
    assert lib.ftmi_tacotron_decoder(None, None) == 1001
    a = _lib.TacoArgs()
    assert lib.ftmi_tacotron_decoder(ctypes.byref(a), None) == 1001  # null pointers
    assert lib.ftmi_tacotron_decoder_workspace_bytes(1, 400) > 0
    assert lib.ftmi_tacotron_decoder_workspace_bytes(2, 512) > 0
    assert lib.ftmi_tacotron_decoder_workspace_bytes(1, 513) == 0   # beyond the stated T range
    assert lib.ftmi_tacotron_decoder_workspace_bytes(3, 100) == 0   # beyond the per-launch batch
    fake = ctypes.c_void_p(256)
    for n, _ in _lib.TacoArgs._fields_[:34]:
        setattr(a, n, fake)
    a.B, a.T, a.r, a.steps = 1, 600, 1, 10
    a.decoder_dims, a.lstm_dims, a.n_mels, a.prenet_dims = 256, 512, 80, 128
    assert lib.ftmi_tacotron_decoder(ctypes.byref(a), None) == 1003  # T beyond the range
    a.T, a.lstm_dims = 100, 256
    assert lib.ftmi_tacotron_decoder(ctypes.byref(a), None) == 1003  # another architecture
    a.lstm_dims, a.r = 512, 21
    assert lib.ftmi_tacotron_decoder(ctypes.byref(a), None) == 1003  # r beyond Decoder.max_r
