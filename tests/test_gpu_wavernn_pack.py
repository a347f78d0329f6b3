"""Packed WaveRNN launches on the GPU (ftmi_wavernn_packed, ftmi_wr_unfold_packed,
WaveRNN.generate_batch, `gen_forward wavernn --voc_batch`): utterances of 21, 27 and 45 mel frames
whose 93 folds share three launches (tests/wr_pack_cases.py; the shapes' claims and the defects
these tests catch are checked on the CPU by tests/test_wavernn_pack.py).

  * teacher-forced logits of every utterance against the float64 oracle run on that utterance
    alone: |logits - oracle| <= max(1e-4, 10 drift), drift per utterance; status word clean;
  * bit equality with the utterance run alone through ftmi_wavernn (logits and drawn samples),
    under a permuted order, and with the table handed over as host memory.  The per-fold
    arithmetic does not depend on the fold's slot, its instance or the launch's NBV (each fold
    has its own accumulators; the k-parts meet in a fixed order), so every row must agree;
  * the draw rule of tests/wr_cases.py check_draws per utterance, with its own key and its own
    fold indices, at 256 and 16 classes and in MOL mode;
  * unbatched rows of unequal length; the one-launch tail; the CLI flag.

Every test prints its figures (`WRPACK ...` lines) before it asserts.
"""
import functools
import wave

import numpy as np
import pytest
import torch

import wr_cases as C
import wr_pack_cases as PC
from forwardtacotron_amd import _lib, ops

pytestmark = pytest.mark.gpu

DEV = 'cuda'
TARGET, OVERLAP = PC.FOLD


@functools.lru_cache(maxsize=None)
def _model(bits):
    p = PC.pack(bits)
    return C.build_model(p.cfg, p.sd, DEV)


@functools.lru_cache(maxsize=None)
def _packed(bits, order=None, host_table=False):
    got, plan, status = PC.gpu_packed_logits(PC.pack(bits), _model(bits), order, host_table)
    got.setflags(write=False)
    return got, plan, status


@pytest.mark.parametrize('bits', [9, None])
def test_packed_teacher_forced_logits(bits):
    p, m = PC.pack(bits), _model(bits)
    assert [m._fold_shape(T * PC.HOP, 1, True, TARGET, OVERLAP) for T in PC.ITEMS_T] == [(21, 7), (27, 7), (45, 7)]
    got, plan, status = _packed(bits)
    assert plan.launches == [(16, 2, 0, 32), (16, 2, 32, 32), (16, 2, 64, 29)]
    assert got.shape == (93, p.L, p.NC) and got.dtype == np.float32
    finite = bool(np.isfinite(got).all())
    rows = []
    for i in range(3):
        l64, b = PC.oracle(bits, i), PC.bound(bits, i)
        err = float(np.abs(got[plan.rows(i)] - l64).max()) if finite else float('inf')
        rows.append((err, b))
        print(f'WRPACK logits bits={bits} item={i} folds={p.folds[i]} drift={PC.drift(bits, i):.3e} '
              f'bound={b:.3e} err={err:.3e} status={status}')
    assert status == 0 and finite
    for i, (err, b) in enumerate(rows):
        assert err <= b, (bits, i, err, b)


@pytest.mark.parametrize('bits', [9, None])
def test_packed_rows_equal_the_utterance_alone(bits):
    p, m = PC.pack(bits), _model(bits)
    got, plan, status = _packed(bits)
    assert status == 0
    for i in (1, 2):
        alone, st = PC.gpu_single_logits(p, m, i)
        same = np.array_equal(alone, got[plan.rows(i)])
        print(f'WRPACK alone bits={bits} item={i} launches={C.launches(p.folds[i])} equal={same} '
              f'max_diff={float(np.abs(alone - got[plan.rows(i)]).max()):.3e}')
        assert st == 0 and same, (bits, i)
    perm, plan2, st2 = _packed(bits, (2, 0, 1))
    assert st2 == 0 and plan2.order == [0, 1, 2] and plan2.lengths == [45, 21, 27]
    for k, i in enumerate((2, 0, 1)):  # utterance i sits at position k of the permuted call
        assert np.array_equal(perm[plan2.rows(k)], got[plan.rows(i)]), (bits, i)


def test_host_table_is_checked_and_staged_by_the_library():
    got, _, _ = _packed(9)
    host, _, status = _packed(9, None, True)
    assert status == 0 and np.array_equal(host, got)


@pytest.mark.parametrize('bits', [9, None])
def test_packed_samples_equal_the_utterance_alone(bits):
    p, m = PC.pack(bits), _model(bits)
    smp, plan = m.generate_samples_batch(p.mels, True, TARGET, OVERLAP, seeds=PC.SEEDS)
    assert int(ops.status_word(torch.device(DEV)).item()) == 0
    smp = smp.cpu().numpy()
    assert smp.shape == (93, p.L)
    for i in (1, 2):
        alone = m.generate_samples(p.mels[i], True, TARGET, OVERLAP, seed=PC.SEEDS[i]).cpu().numpy()
        assert np.array_equal(alone, smp[plan.rows(i)]), (bits, i)
    other = m.generate_samples(p.mels[1], True, TARGET, OVERLAP, seed=PC.SEEDS[0]).cpu().numpy()
    assert not np.array_equal(other, smp[plan.rows(1)])  # the key matters


@pytest.mark.parametrize('bits', [8, 4, None])
def test_draws_for_every_utterance(bits):
    p, m = PC.pack(bits), _model(bits)
    smp, plan = m.generate_samples_batch(p.mels, True, TARGET, OVERLAP, seeds=PC.SEEDS)
    assert int(ops.status_word(torch.device(DEV)).item()) == 0
    smp = smp.cpu().numpy()
    exact = total = 0
    for i in range(3):
        e, t = PC.check_item_draws(m, p.cfg, p.mels[i].numpy(), smp[plan.rows(i)], PC.SEEDS[i], TARGET, OVERLAP)
        print(f'WRPACK draws bits={bits} item={i} exact={e}/{t}')
        exact, total = exact + e, total + t
    assert total == 93 * p.L
    assert exact >= 0.995 * total, (exact, total)
    if bits is not None:  # every sample is a class value
        idx = np.rint((smp + 1.0) * (m.n_classes - 1) / 2.0)
        assert np.array_equal(smp, (2.0 * idx.astype(np.float32) / np.float32(m.n_classes - 1) - 1.0).astype(np.float32))
        assert len(np.unique(idx)) >= 2


@pytest.mark.parametrize('bits', [9, None])
def test_unbatched_rows_of_unequal_length(bits):
    p = PC.Pack(bits, lengths=PC.UNBATCHED_T)
    m = _model(bits)
    smp, plan = m.generate_samples_batch(p.mels, False, TARGET, OVERLAP, seeds=PC.SEEDS)
    assert int(ops.status_word(torch.device(DEV)).item()) == 0
    smp = smp.cpu().numpy()
    assert plan.order == [2, 1, 0] and plan.launches == [(8, 2, 0, 3)] and plan.launch_steps == [198]
    assert smp.shape == (3, 198)
    exact = total = 0
    for i, T in enumerate(PC.UNBATCHED_T):
        row = smp[plan.rows(i)][:, :T * PC.HOP]
        e, t = PC.check_item_draws(m, p.cfg, p.mels[i].numpy(), row, PC.SEEDS[i], TARGET, OVERLAP, batched=False)
        print(f'WRPACK unbatched bits={bits} item={i} T={T} exact={e}/{t}')
        exact, total = exact + e, total + t
    assert total == sum(PC.UNBATCHED_T) * PC.HOP and exact >= 0.995 * total, (exact, total)
    waves = m.generate_batch(p.mels, False, TARGET, OVERLAP, True, seeds=PC.SEEDS)
    assert [w.shape for w in waves] == [((T - 1) * PC.HOP,) for T in PC.UNBATCHED_T]
    yd = torch.from_numpy(smp).to(DEV)
    for i, T in enumerate(PC.UNBATCHED_T):
        ref = ops.wr_unfold(yd[plan.rows(i)], TARGET, OVERLAP, False, bits is not None, m.n_classes,
                            (T - 1) * PC.HOP, 20 * PC.HOP).cpu().numpy()
        assert waves[i].dtype == np.float64 and np.array_equal(waves[i], ref), i


# ---------------------------------------------------------------------------------------
# the tail

def _samples(rng, B, L, mu_law, nc):
    if mu_law:
        i = rng.integers(0, nc, (B, L)).astype(np.float32)
        return (2.0 * i / np.float32(nc - 1) - np.float32(1.0)).astype(np.float32)
    return rng.normal(0.0, 1.0, (B, L)).astype(np.float32)


@pytest.mark.parametrize('mu_law,nc', [(False, 512), (True, 256), (True, 16)])
def test_unfold_packed_equals_unfold_per_utterance(mu_law, nc):
    target, overlap, fade = 4, 3, 5
    stride, L = target + overlap, target + 2 * overlap
    folds = (3, 1, 5, 2)
    waves = (3 * stride + overlap, stride, 5 * stride - 1, 2 * stride + 1)  # full, cropped, odd
    rng = np.random.Generator(np.random.PCG64([int(mu_law), nc]))
    y = _samples(rng, sum(folds), L, mu_law, nc)
    yd = torch.from_numpy(y).to(DEV)
    items, r, off = [], 0, 0
    for nf, w in zip(folds, waves):
        items.append((r, nf, w, off))
        r, off = r + nf, off + w
    items = np.asarray(items, dtype=np.int32)
    out = ops.wr_unfold_packed(yd, items, target, overlap, True, mu_law, nc, fade).cpu().numpy()
    assert out.dtype == np.float64 and out.shape == (sum(waves),)
    for r0, nf, w, o in items.tolist():
        ref = ops.wr_unfold(yd[r0:r0 + nf], target, overlap, True, mu_law, nc, w, fade).cpu().numpy()
        assert np.array_equal(out[o:o + w], ref), (r0, nf, w)
    # the same table as host memory: checked and staged by the library
    host = torch.full((sum(waves),), np.nan, device=DEV, dtype=torch.float64)
    _lib.call('ftmi_wr_unfold_packed', yd.data_ptr(), yd.size(0), L, items.ctypes.data, len(items), target,
              overlap, 1, int(mu_law), nc, fade, host.data_ptr(), host.numel(), ops._stream())
    torch.cuda.synchronize()
    assert np.array_equal(host.cpu().numpy(), out)
    # unbatched: one row per utterance, cropped rows
    it1 = np.asarray([(0, 1, L, 0), (4, 1, L - 3, L), (2, 1, fade, 2 * L - 3)], dtype=np.int32)
    out1 = ops.wr_unfold_packed(yd, it1, target, overlap, False, mu_law, nc, fade).cpu().numpy()
    for r0, nf, w, o in it1.tolist():
        ref = ops.wr_unfold(yd[r0:r0 + 1], target, overlap, False, mu_law, nc, w, fade).cpu().numpy()
        assert np.array_equal(out1[o:o + w], ref), (r0, w)
    with pytest.raises(ValueError):  # rows past the matrix: refused by the binding
        ops.wr_unfold_packed(yd, np.asarray([(9, 3, 10, 0)], dtype=np.int32), target, overlap, True,
                             mu_law, nc, fade)


def test_generate_batch_returns_each_utterances_wave():
    """Alone, the 21-, 27- and 45-fold utterances draw the same samples (previous tests), so
    generate_batch's waves equal generate's bit for bit, in the caller's order."""
    p, m = PC.pack(8), _model(8)
    order = (2, 0, 1)
    waves = m.generate_batch([p.mels[i][0] for i in order], True, TARGET, OVERLAP, True,
                             seeds=[PC.SEEDS[i] for i in order])
    assert m.training
    for k, i in enumerate(order):
        T = PC.ITEMS_T[i]
        ref = m.generate(p.mels[i], True, TARGET, OVERLAP, True, seed=PC.SEEDS[i])
        assert waves[k].dtype == np.float64 and waves[k].shape == ((T - 1) * PC.HOP,)
        assert np.array_equal(waves[k], ref), i
        assert np.abs(waves[k]).max() <= 1.0 and np.abs(waves[k]).max() > 0
    # default seeds: one draw per utterance from torch's CPU generator, in order, as generate does
    torch.manual_seed(5)
    a = m.generate_batch([p.mels[0], p.mels[1]], True, TARGET, OVERLAP, True)
    torch.manual_seed(5)
    b = [m.generate(p.mels[i], True, TARGET, OVERLAP, True) for i in (0, 1)]
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    with pytest.raises(ValueError, match='at least 21'):
        m.generate_batch([p.mels[0], p.mels[1][:, :, :20]], True, TARGET, OVERLAP, True)


def test_cli_voc_batch_writes_the_same_files(tmp_path):
    from forwardtacotron_amd.gen_forward import main
    lines = ['həloʊ wɜːld, haʊ ɑːɹ juː tədeɪ', 'ðɪs ɪz ɐ tɛst ʌv ðə vəʊkəʊdə ɪn wʌn lɔːntʃ fɔːɹ ɔːl',
             'ɡʊd mɔːnɪŋ tə juː ɔːl']
    src = tmp_path / 'sentences.txt'
    src.write_text('\n'.join(lines) + '\n', encoding='utf-8')
    common = ['--synthetic', '--sentences', str(src)]
    mels = main(common + ['--out', str(tmp_path / 'mel'), 'hifigan'])
    frames = [np.load(f, allow_pickle=False).shape[2] for f in mels]
    assert len(set(frames)) > 1  # unequal lengths
    voc = ['wavernn', '--voc_synthetic', '--target', '4000', '--overlap', '200']
    one = main(common + ['--out', str(tmp_path / 'one')] + voc + ['--voc_batch', '1'])
    three = main(common + ['--out', str(tmp_path / 'three')] + voc + ['--voc_batch', '3'])
    two = main(common + ['--out', str(tmp_path / 'two')] + voc + ['--voc_batch', '2'])  # 2 + 1
    assert [f.name for f in one] == [f.name for f in three] == [f.name for f in two]
    assert [f.name for f in one] == [f'{i}_forward_0k_alpha1.0_amp1.0_wavernn.wav' for i in (1, 2, 3)]
    for files in (one, three, two):
        for f, T in zip(files, frames):
            with wave.open(str(f), 'rb') as w:
                assert w.getframerate() == 22050 and w.getnframes() == 256 * (T - 1), (f, T)
