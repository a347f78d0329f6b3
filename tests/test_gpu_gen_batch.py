"""ForwardTacotron.generate_batch / generate_masked: every item of a batch of unequal lengths
equals generate() of that item alone.

The reference of each item is the torch-CPU restatement (oracle.ft_torch_cpu.generate) run on
the item alone, (1, L_i); the bounds are those of tests/test_gpu_model.py (its `check`).

Inputs: lengths [40, 39, 37, 33, 9, 2, 40] — item ends at T, T - 1, T - 3 and T - 7 (inside
every halo reach of the path), a 9-token and a 2-token item — ids from
np.random.Generator(PCG64(20261021)).integers(1, 135, L) drawn in that order, item 3's
position 5 set to id 0 (a real symbol inside a sentence, not a pad).

Tie margins under the oracle (the smallest distance of dur + 0.5 from an integer, which must
be at least 1e-3 = 100 x the duration tolerance for the frame counts to be decided):
alpha = 1.0, with and without the callbacks (they do not reach the durations):
0.0335, 0.0074, 0.0128, 0.0134, 0.0611, 0.0221, 0.0105, T_mel 280, 285, 250, 233, 69, 18, 274;
alpha = 1000: every duration is filled to 2.0 (margin 0.5), T_mel = 2 L_i.
"""
import numpy as np
import pytest
import torch

from conftest import load_golden
from test_gpu_model import MAX_TOL, check

pytestmark = pytest.mark.gpu

LENGTHS = [40, 39, 37, 33, 9, 2, 40]
T_MEL = [280, 285, 250, 233, 69, 18, 274]
# test_gpu_model.py's gen_callbacks pair
CALLBACKS = dict(pitch_function=lambda p: p * 2.0 + 0.1, energy_function=lambda e: e - 0.05)


def tokens():
    rng = np.random.Generator(np.random.PCG64(20261021))
    xs = [rng.integers(1, 135, L) for L in LENGTHS]
    xs[3][5] = 0
    return xs


@pytest.fixture(scope='module')
def xs():
    return tokens()


@pytest.fixture(scope='module')
def oracle(synth_sd, xs):
    """kind -> the oracle's result of every item alone, computed once and shared."""
    from oracle import ft_torch_cpu as TC
    sd = TC.to_torch(synth_sd)
    cache = {}

    def get(kind):
        if kind not in cache:
            kw = {'plain': dict(alpha=1.0), 'fill': dict(alpha=1000.0),
                  'callbacks': dict(alpha=1.0, **CALLBACKS)}[kind]
            outs = []
            for x in xs:
                o = TC.generate(sd, torch.from_numpy(x)[None], **kw)
                outs.append({k: v.numpy() for k, v in o.items()})
            for o in outs:  # the inputs' condition: decided frame counts
                f = o['dur'].ravel() + np.float32(0.5)
                assert np.abs(f - np.round(f)).min() >= 1e-3
            cache[kind] = outs
        return cache[kind]
    return get


def dev(xs):
    return [torch.from_numpy(x).cuda() for x in xs]


def check_items(outs, refs):
    assert len(outs) == len(refs)
    for i, (o, g) in enumerate(zip(outs, refs)):
        for k in ('mel', 'mel_post', 'dur', 'pitch', 'energy'):
            assert tuple(o[k].shape) == g[k].shape, (i, k, tuple(o[k].shape), g[k].shape)
        check(o, g)


def test_each_item_equals_the_item_alone(gpu_model, xs, oracle):
    refs = oracle('plain')
    assert [r['mel'].shape[2] for r in refs] == T_MEL
    outs = gpu_model.generate_batch(dev(xs))
    check_items(outs, refs)
    alone = gpu_model.generate(torch.from_numpy(xs[4]).cuda()[None])
    for k in ('mel', 'mel_post', 'dur', 'pitch', 'energy'):  # generate(x_i[None])'s shapes
        assert outs[4][k].shape == alone[k].shape and outs[4][k].dtype == alone[k].dtype


def test_padded_generate_is_not_the_item_alone(gpu_model, xs, oracle):
    """Discrimination: generate() on the zero-padded batch of the same tokens couples the
    items (pads get durations, the reverse recurrences start in the padding, the batch runs
    to one T_mel), so generate_batch cannot pass by forwarding to it."""
    refs = oracle('plain')
    T = max(LENGTHS)
    x = np.zeros((len(xs), T), np.int64)
    for b, s in enumerate(xs):
        x[b, :len(s)] = s
    out = gpu_model.generate(torch.from_numpy(x).cuda())
    dur = out['dur'].cpu().numpy()
    post = out['mel_post'].cpu().numpy()
    worst_dur = worst_post = 0.0
    for b, g in enumerate(refs):
        L, F = LENGTHS[b], g['mel'].shape[2]
        worst_dur = max(worst_dur, float(np.abs(dur[b, :L] - g['dur'][0]).max()))
        n = min(F, post.shape[2])
        worst_post = max(worst_post, float(np.abs(post[b, :, :n] - g['mel_post'][0, :, :n]).max()))
    print(f'padded generate vs item alone: dur {worst_dur:.3f} frames, mel_post {worst_post:.3f}')
    assert worst_dur > 0.5 or worst_post > 10 * MAX_TOL


def test_order_and_chunking_do_not_matter(gpu_model, xs, oracle):
    refs = oracle('plain')
    outs = gpu_model.generate_batch(dev(xs)[::-1])
    check_items(outs, refs[::-1])
    outs = gpu_model.generate_batch([x.tolist() for x in xs], max_batch=3)  # int lists
    check_items(outs, refs)


def test_fill_rule_is_decided_per_item(gpu_model, xs, oracle):
    """alpha = 1000: every predicted duration truncates to 0, so every item alone fills its
    durations with 2.0 — T_mel == 2 L_i per item, not the batch's 2 T."""
    outs = gpu_model.generate_batch(dev(xs), alpha=1000.0)
    for o, L in zip(outs, LENGTHS):
        assert o['mel'].shape[2] == 2 * L and o['mel_post'].shape[2] == 2 * L
        assert torch.equal(o['dur'], torch.full((1, L), 2.0, device='cuda'))
    check_items(outs, oracle('fill'))


def test_elementwise_callbacks(gpu_model, xs, oracle):
    check_items(gpu_model.generate_batch(dev(xs), **CALLBACKS), oracle('callbacks'))
    check_items(gpu_model.generate_batch(dev(xs), max_batch=4, **CALLBACKS), oracle('callbacks'))


def test_generate_masked(gpu_model, xs, oracle):
    """The tensor-level entry: whatever the pad positions hold is ignored (here a real id,
    7), mel_len is the oracle's frame counts, mel / mel_post hold padding_value past
    mel_len, dur / pitch / energy hold 0 past x_len."""
    refs = oracle('plain')
    B, T = len(xs), max(LENGTHS)
    x = np.full((B, T), 7, np.int64)
    for b, s in enumerate(xs):
        x[b, :len(s)] = s
    out = gpu_model.generate_masked(torch.from_numpy(x).cuda(), torch.tensor(LENGTHS))
    assert out['mel_len'].tolist() == T_MEL
    pad = np.float32(gpu_model.padding_value)
    assert out['mel'].shape == out['mel_post'].shape == (B, 80, max(T_MEL))
    assert out['dur'].shape == (B, T) and out['pitch'].shape == out['energy'].shape == (B, 1, T)
    host = {k: out[k].cpu().numpy() for k in ('mel', 'mel_post', 'dur', 'pitch', 'energy')}
    for b, g in enumerate(refs):
        L, F = LENGTHS[b], T_MEL[b]
        assert (host['mel'][b, :, F:] == pad).all() and (host['mel_post'][b, :, F:] == pad).all()
        assert (host['dur'][b, L:] == 0).all()
        assert (host['pitch'][b, :, L:] == 0).all() and (host['energy'][b, :, L:] == 0).all()
        check({'mel': out['mel'][b:b + 1, :, :F], 'mel_post': out['mel_post'][b:b + 1, :, :F],
               'dur': out['dur'][b:b + 1, :L], 'pitch': out['pitch'][b:b + 1, :, :L],
               'energy': out['energy'][b:b + 1, :, :L]}, g)
    # lengths on the device are read on the host too
    again = gpu_model.generate_masked(torch.from_numpy(x).cuda(), torch.tensor(LENGTHS).cuda())
    for k in host:
        assert torch.equal(again[k], out[k]), k


def test_same_call_same_bits_and_own_storage(gpu_model, xs):
    first = gpu_model.generate_batch(dev(xs), max_batch=4)
    kept = [{k: v.clone() for k, v in o.items()} for o in first]
    second = gpu_model.generate_batch(dev(xs), max_batch=4)
    gpu_model.generate_batch(dev(xs)[:3], alpha=1000.0)  # a later call of another shape
    torch.cuda.synchronize()
    for a, b, c in zip(first, kept, second):
        for k in a:
            assert torch.equal(a[k], b[k]), k  # not overwritten by the later calls
            assert torch.equal(a[k], c[k]), k  # the same bits
    ptrs = [t.untyped_storage().data_ptr() for o in first for t in o.values()]
    assert len(set(ptrs)) == len(ptrs)


def test_generate_is_undisturbed(gpu_model, xs):
    """Packs, caches and the phase graph are untouched: generate() on the gen_b3 golden input
    gives the same bits before and after a generate_batch call."""
    x = torch.from_numpy(load_golden('gen_b3')['x']).cuda()
    before = {k: v.clone() for k, v in gpu_model.generate(x).items()}
    gpu_model.generate_batch(dev(xs), max_batch=3)
    after = gpu_model.generate(x)
    for k in before:
        assert torch.equal(before[k], after[k]), k
