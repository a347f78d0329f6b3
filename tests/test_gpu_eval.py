"""Validation losses and checkpoint evaluation on the HIP path (forwardtacotron_amd/evaluate.py,
csrc/eval.hip) against the reference evaluated in float64 (tests/golden/goldens_eval.npz, made
by tests/golden/make_goldens_eval.py) and the float64 restatement (tests/eval_cases.py).

Bounds.  Every loss is an fp64 sum rounded to fp32 once, so a reduced loss lies within 2^-23 of
the float64 golden, relative: half of that is the rounding, the rest is slack for the order of
the fp64 additions and the last bit of exp and log.  The reference's own fp32 result is off by
the error recorded per case, so it is matched within that plus 2^-23.  A per-sample mixture
value adds a floor of 2^-40 for the fp64 rounding of terms as large as 2^7.

The end-to-end tests check the wiring of evaluate_*: which tensors, which lengths, m1 + m2, the
transpose and unsqueeze of RAW mode, the division by len(val_set), the return types.  They
apply the restatement to the outputs of the very forward calls evaluate_* makes (a recording
wrapper keeps them), so model parity, covered elsewhere, plays no part."""
import json

import numpy as np
import pytest
import torch

import eval_cases as ec
from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu

L1, CE, MOL = ec.l1_cases(), ec.ce_cases(), ec.mol_cases()
EPS = 2.0 ** -23
FLOOR = 2.0 ** -40


@pytest.fixture(scope='module')
def gold():
    g = load_golden('goldens_eval')
    for kind, cases in (('l1', L1), ('ce', CE), ('mol', MOL)):
        for n, c in cases.items():
            assert ec.sha(c) == str(g[f'sha/{kind}/{n}']), (kind, n)
    return g


@pytest.fixture(scope='module')
def ev():
    from forwardtacotron_amd import evaluate
    return evaluate


def scalar(t):
    assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 0
    return float(t)


def check(gold, key, got):
    want, ref32, own = float(gold[f'f64/{key}']), float(gold[f'f32/{key}']), float(gold[f'err/{key}'])
    if np.isnan(want):
        assert np.isnan(got), key
        return
    print(key, 'vs float64', abs(got - want) / abs(want) / EPS, 'x 2^-23; vs reference fp32',
          abs(got - ref32) / abs(want) / EPS, 'reference own', own / EPS)
    assert abs(got - want) <= EPS * abs(want)
    assert abs(got - ref32) <= (own + EPS) * abs(want)


# ---- L1 -------------------------------------------------------------------------------------

def l1_device(c, layout):
    """x in the named layout ('frame': unit frame stride, contiguous; 'channel': unit channel
    stride, the transposed view a channels-last model output is), target as a view into a
    padded buffer with row stride L + 5, lens as the collate's int64."""
    x = torch.from_numpy(c['x']).cuda()
    if layout == 'channel':
        x = x.transpose(1, 2).contiguous().transpose(1, 2)
        assert x.stride(1) == 1 or x.size(1) == 1
    B, C, L = c['target'].shape
    buf = torch.full((B, C, L + 5), float('nan'), device='cuda')
    buf[:, :, :L] = torch.from_numpy(c['target']).cuda()
    lens = torch.from_numpy(c['lens']).cuda() if 'lens' in c else None
    return x, buf[:, :, :L], lens


def run_l1(ev, c, layout):
    x, t, lens = l1_device(c, layout)
    return scalar(ev.l1(x, t) if lens is None else ev.masked_l1(x, t, lens))


@pytest.mark.parametrize('layout', ['frame', 'channel'])
@pytest.mark.parametrize('name', list(L1))
def test_l1(gold, ev, name, layout):
    check(gold, f'l1/{name}', run_l1(ev, L1[name], layout))


@pytest.mark.parametrize('name', [n for n, c in L1.items() if 'lens' in c])
def test_l1_nan_padding_is_never_read(ev, name):
    """NaN at every frame t >= lens[b]: the result is the bits of the ordinary case, so finite
    wherever that is (the reference would return NaN: x * 0)."""
    plain, padded = run_l1(ev, L1[name], 'frame'), run_l1(ev, ec.nan_padding(L1[name]), 'frame')
    if name == 'lens_all_zero':
        assert np.isnan(plain) and np.isnan(padded)  # 0/0, like the reference
    else:
        assert np.isfinite(padded) and padded == plain


def test_l1_integer_target_and_views(ev):
    """The trainer's dur loss: pred (B, T) and the collate's int64 dur, both unsqueezed."""
    g = np.random.Generator(np.random.PCG64(60))
    dur = g.integers(0, 30, (3, 12))
    pred = g.uniform(0, 30, (3, 12)).astype(np.float32)
    lens = np.array([12, 7, 1])
    got = scalar(ev.masked_l1(torch.from_numpy(pred).cuda().unsqueeze(1),
                              torch.from_numpy(dur).cuda().unsqueeze(1), torch.from_numpy(lens).cuda()))
    want = ec.masked_l1(pred[:, None], dur[:, None].astype(np.float32), lens)
    assert abs(got - want) <= EPS * want
    big = torch.from_numpy(dur).cuda().unsqueeze(1).clone()
    big[1, 0, 3] = -(2 ** 24)
    with pytest.raises(ValueError, match='2\\^24'):
        ev.masked_l1(torch.from_numpy(pred).cuda().unsqueeze(1), big, torch.from_numpy(lens).cuda())


def test_ops_refuse_wrong_dtypes_and_strides():
    from forwardtacotron_amd import ops
    x = torch.zeros(2, 6, 8, device='cuda')
    with pytest.raises(ValueError, match='fp32'):
        ops.l1_loss(x.double(), x.double())
    with pytest.raises(ValueError, match='unit frame stride'):
        ops.l1_loss(x[:, ::2, ::2], x[:, ::2, ::2])
    with pytest.raises(ValueError, match='int32'):
        ops.l1_loss(x, x, torch.tensor([8, 8], device='cuda'))
    with pytest.raises(ValueError, match='int32'):
        ops.cross_entropy(x[0], torch.zeros(6, device='cuda', dtype=torch.int64))
    with pytest.raises(ValueError, match='unit column stride'):
        ops.cross_entropy(x[0, :, ::2], torch.zeros(6, device='cuda', dtype=torch.int32))
    with pytest.raises(ValueError, match='3 K'):
        ops.mol_loss(x[0], torch.zeros(6, device='cuda'), 65536, -32.0)


# ---- cross-entropy --------------------------------------------------------------------------

def run_ce(ev, c, pad=0):
    """Through the public function: (rows, C) logits (a view with row stride C + pad) with
    (rows,) int64 labels, or for the 'batch' cases (B, C, L) with (B, L), as F.cross_entropy takes
    them."""
    rows, C = c['logits'].shape
    buf = torch.full((rows, C + pad), float('nan'), device='cuda')
    buf[:, :C] = torch.from_numpy(c['logits']).cuda()
    x, t = buf[:, :C], torch.from_numpy(c['target']).cuda()
    if 'batch' in c:
        B = c['batch']
        x, t = x.reshape(B, rows // B, C).transpose(1, 2), t.view(B, rows // B)
    return ev.cross_entropy(x, t)


@pytest.mark.parametrize('name', list(CE))
def test_cross_entropy(gold, ev, name):
    check(gold, f'ce/{name}', scalar(run_ce(ev, CE[name], pad=3 if name in ('c30_r63', 'c513_r1400') else 0)))


def test_cross_entropy_rejects_labels_out_of_range(ev):
    from forwardtacotron_amd import ops
    bad = ec.ce_rejected()
    with pytest.raises(ValueError, match='2 label'):
        run_ce(ev, bad)
    # the kernel's part: the two labels are counted and add nothing to the sum
    loss, n_bad = ops.cross_entropy(torch.from_numpy(bad['logits']).cuda(),
                                    torch.from_numpy(bad['target']).cuda().int())
    keep = (bad['target'] >= 0) & (bad['target'] < bad['logits'].shape[1])
    want = ec.cross_entropy(bad['logits'][keep], bad['target'][keep]) * keep.sum() / len(keep)
    assert int(n_bad) == 2 and abs(float(loss) - want) <= EPS * want


# ---- discretized mixture of logistics -------------------------------------------------------

def run_mol(ev, c, pad=0):
    B, L, C = c['y_hat'].shape
    buf = torch.full((B, L, C + pad), float('nan'), device='cuda')
    buf[..., :C] = torch.from_numpy(c['y_hat']).cuda()
    kw = {'num_classes': c['num_classes'], 'reduce': c['reduce']}
    if 'log_scale_min' in c:
        kw['log_scale_min'] = c['log_scale_min']
    return ev.discretized_mix_logistic_loss(buf[..., :C], torch.from_numpy(c['y']).cuda(), **kw)


@pytest.mark.parametrize('name', list(MOL))
def test_mol(gold, ev, name):
    c = MOL[name]
    got = run_mol(ev, c)
    if c['reduce']:
        check(gold, f'mol/{name}', scalar(got))
        return
    assert got.shape == c['y'].shape and got.dtype == torch.float32 and got.is_cuda
    got = got.cpu().numpy().astype(np.float64)
    want, ref32 = gold[f'f64/mol/{name}'], gold[f'f32/mol/{name}'].astype(np.float64)
    own = float(gold[f'err/mol/{name}'])
    print(name, 'per sample vs float64', float(np.max(np.abs(got - want) / (EPS * np.abs(want) + FLOOR))),
          'x bound; reference own', own / EPS, 'x 2^-23')
    assert (np.abs(got - want) <= EPS * np.abs(want) + FLOOR).all()
    assert (np.abs(got - ref32) <= (own + EPS) * np.abs(want) + FLOOR).all()


def test_mol_row_alone_and_in_a_larger_launch(ev):
    """A per-sample value depends on its row alone: rows 100..139 of the edge case, launched by
    themselves and from a buffer with another row stride, have the bits they have in the whole."""
    c = dict(MOL['edge_k10'], reduce=False)
    whole = run_mol(ev, c)
    part = {'y_hat': c['y_hat'][1:2, 100:140], 'y': c['y'][1:2, 100:140], 'num_classes': 65536,
            'reduce': False}
    assert torch.equal(run_mol(ev, part, pad=2), whole[1:2, 100:140])
    # and the reduced loss is the mean of the per-sample values, up to its one rounding
    red = scalar(run_mol(ev, MOL['edge_k10']))
    mean = float(whole.double().mean())
    assert abs(red - mean) <= EPS * abs(mean)


def test_same_bits_on_every_call(ev):
    for run in (lambda: run_l1(ev, L1['big_wide'], 'frame'), lambda: run_l1(ev, L1['big_wide'], 'channel'),
                lambda: float(run_ce(ev, CE['c513_r1400'])), lambda: float(run_mol(ev, MOL['edge_k10']))):
        first = run()
        assert all(np.float32(run()).tobytes() == np.float32(first).tobytes() for _ in range(3))


# ---- end to end -----------------------------------------------------------------------------

class Recording(torch.nn.Module):
    """Delegates to a model and keeps what each forward call returned, on the host."""

    def __init__(self, inner):
        super().__init__()
        self.inner = inner
        self.calls = []

    @property
    def mode(self):
        return self.inner.mode

    def forward(self, *args):
        out = self.inner(*args)
        host = lambda t: t.detach().cpu().numpy().copy()  # noqa: E731
        self.calls.append({k: host(v) for k, v in out.items()} if isinstance(out, dict)
                          else [host(v) for v in (out if isinstance(out, tuple) else (out,))])
        return out


def tts_batches():
    """Two collated batches, B = 2 and B = 3, T <= 12, mel_len <= 40, dur as int64."""
    from forwardtacotron_amd.gta import collate_tts
    rng = np.random.Generator(np.random.PCG64(70))
    batches = []
    for k, x_lens in enumerate(((12, 7), (5, 11, 9))):
        items = []
        for i, xl in enumerate(x_lens):
            dur = rng.integers(1, 4, xl)
            ml = int(dur.sum())
            items.append({'x': rng.integers(1, 135, xl), 'mel': rng.normal(-4, 2, (80, ml)).astype(np.float32),
                          'item_id': f'v{k}{i}', 'x_len': xl, 'mel_len': ml, 'dur': dur.astype(np.float32),
                          'pitch': rng.normal(0, 1, xl).astype(np.float32),
                          'energy': rng.normal(0, 1, xl).astype(np.float32)})
            assert xl <= 12 and ml <= 40
        b = collate_tts(items, r=1)
        b['dur'] = b['dur'].long()
        batches.append(b)
    return batches


def check_forward(ev, model):
    batches = tts_batches()
    rec = Recording(model)
    got = ev.evaluate_forward(rec, batches)
    assert len(rec.calls) == 2 and not model.training
    want = {k: [] for k in ('mel', 'dur', 'pitch', 'energy')}
    for b, p in zip(batches, rec.calls):
        mel, ml, xl = b['mel'].numpy(), b['mel_len'].numpy(), b['x_len'].numpy()
        want['mel'].append(ec.masked_l1(p['mel'], mel, ml) + ec.masked_l1(p['mel_post'], mel, ml))
        want['dur'].append(ec.masked_l1(p['dur'][:, None], b['dur'].numpy()[:, None].astype(np.float32), xl))
        want['pitch'].append(ec.masked_l1(p['pitch'], b['pitch'].numpy()[:, None], xl))
        want['energy'].append(ec.masked_l1(p['energy'], b['energy'].numpy()[:, None], xl))
    assert sorted(got) == ['dur_loss', 'energy_loss', 'mel_loss', 'pitch_loss']
    assert type(got['mel_loss']) is float and type(got['dur_loss']) is float
    for k in ('mel', 'dur'):  # fp32 losses added and divided on the host in Python floats: exact
        w = sum(want[k]) / 2
        print(k, abs(got[f'{k}_loss'] - w) / w / EPS, 'x 2^-23')
        assert abs(got[f'{k}_loss'] - w) <= EPS * w
    for k in ('pitch', 'energy'):  # added as fp32 device tensors, like the reference: two more
        w = sum(want[k]) / 2       # roundings of 2^-24 each (the sum, the division)
        g = scalar(got[f'{k}_loss'])
        print(k, abs(g - w) / w / EPS, 'x 2^-23')
        assert got[f'{k}_loss'].device == next(model.parameters()).device
        assert abs(g - w) <= 2 * EPS * w


def test_evaluate_forward_tacotron(ev, gpu_model):
    check_forward(ev, gpu_model)


def test_evaluate_fastpitch(ev):
    from forwardtacotron_amd.fast_pitch import FastPitch
    from forwardtacotron_amd.synthetic import default_config, synthetic_state_dict
    m = FastPitch.from_config(default_config())
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic_state_dict(m, 0, 'fast_pitch').items()})
    check_forward(ev, m.to('cuda').eval())


def test_evaluate_tacotron(ev):
    from forwardtacotron_amd.synthetic import default_config, synthetic_array
    from forwardtacotron_amd.tacotron import Tacotron
    keys = json.loads((GOLDEN / 'tacotron_state_dict_keys.json').read_text())
    m = Tacotron.from_config(default_config())
    m.load_state_dict({k: torch.from_numpy(synthetic_array(k, shape, dt, 0, 'tacotron')) for k, shape, dt in keys})
    m = m.to('cuda').eval()
    m.r = 1
    batches = [{k: b[k] for k in ('x', 'mel', 'mel_len', 'x_len')} for b in tts_batches()]
    rec = Recording(m)
    loss, score = ev.evaluate_tacotron(rec, batches)
    assert type(loss) is float and type(score) is float and len(rec.calls) == 2
    want_loss, want_score = [], []
    for b, (m1, m2, att) in zip(batches, rec.calls):
        mel = b['mel'].numpy()
        assert m1.shape == m2.shape == mel.shape
        want_loss.append(ec.l1(m1, mel) + ec.l1(m2, mel))
        rows = att.shape[1]
        sharp = [att[j, :min(rows, int(n))].astype(np.float64).max(1).sum() / rows
                 for j, n in enumerate(b['mel_len'].numpy())]
        want_score.append(float(np.mean(sharp)))
    w = sum(want_loss) / 2
    print('val_loss', abs(loss - w) / w / EPS, 'x 2^-23')
    assert abs(loss - w) <= EPS * w
    # each item's score is rounded to fp32 once and the mean over B <= 3 items is torch's fp32
    # mean (two additions, one division): four roundings of 2^-24
    w = sum(want_score) / 2
    assert abs(score - w) <= 2 * EPS * w


@pytest.mark.parametrize('mode', ['RAW', 'MOL'])
def test_evaluate_wavernn(ev, mode):
    from forwardtacotron_amd.synthetic import default_config, load_synthetic
    from forwardtacotron_amd.wavernn import WaveRNN
    cfg = default_config()
    cfg['vocoder']['model']['mode'] = mode
    m = WaveRNN.from_config(cfg)
    load_synthetic(m, kind='wavernn')
    m = m.to('cuda').eval()
    rng = np.random.Generator(np.random.PCG64(80))
    batches = []
    for B, frames in ((2, 1), (1, 2)):
        L = frames * m.hop_length
        mel = rng.normal(-4, 2, (B, 80, frames + 2 * m.pad)).astype(np.float32)
        x = rng.uniform(-1, 1, (B, L)).astype(np.float32)
        y = rng.integers(0, m.n_classes, (B, L)) if mode == 'RAW' else \
            np.clip(rng.normal(0, 0.6, (B, L)), -1, 1).astype(np.float32)
        batches.append({'x': torch.from_numpy(x), 'y': torch.from_numpy(y), 'mel': torch.from_numpy(mel)})
    rec = Recording(m)
    got = ev.evaluate_wavernn(rec, batches)
    assert type(got) is float and len(rec.calls) == 2
    want = []
    for b, (y_hat,) in zip(batches, rec.calls):
        y = b['y'].numpy()
        assert y_hat.shape == y.shape + (m.n_classes,)
        if mode == 'RAW':
            want.append(ec.cross_entropy(y_hat.reshape(-1, m.n_classes), y.reshape(-1)))
        else:
            want.append(float(ec.mol(y_hat, y[..., None])[0].mean()))
    w = sum(want) / 2
    print(mode, abs(got - w) / abs(w) / EPS, 'x 2^-23')
    assert abs(got - w) <= EPS * abs(w)


def test_mel_l1(ev):
    from forwardtacotron_amd.dsp import DSP
    from forwardtacotron_amd.synthetic import default_config
    dsp = DSP.from_config(default_config())
    rng = np.random.Generator(np.random.PCG64(90))
    wav = torch.from_numpy(rng.uniform(-0.5, 0.5, 3000).astype(np.float32)).cuda()
    assert ev.mel_l1(dsp, wav, wav) == 0.0
    got = ev.mel_l1(dsp, wav, wav * 0.5)
    a = dsp.wav_to_mel(wav, normalize=False).cpu().numpy()
    b = dsp.wav_to_mel(wav * 0.5, normalize=False).cpu().numpy()
    assert a.shape == (80, 1 + 3000 // dsp.hop_length) and (a >= 0).all()  # not log-normalised
    want = ec.l1(a, b)
    assert type(got) is float and want > 0 and abs(got - want) <= EPS * want
    with pytest.raises(ValueError, match='one length'):
        ev.mel_l1(dsp, wav, wav[:-1])
