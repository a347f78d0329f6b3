"""Phoneme pitch / energy goldens from the reference (train_tacotron.py: extract_pitch_energy,
normalize_values).

Build container only (reads the reference checkout, absent on the GPU box):

    FT_REFERENCE=<reference checkout> python tests/golden/make_goldens_features.py

train_tacotron.py cannot be imported without librosa, so the two function definitions are
taken from the file at run time (ast, never copied into this repository) and executed with the
names they use: numpy, a `paths` namespace that points into a temporary tree, a pickle loader
and silent progress helpers.  The cases of tests/feature_cases.py are written there as one data
set ({id}.npy under alg / mel / raw_pitch, train_dataset.pkl + val_dataset.pkl) and the
reference's extract_pitch_energy runs over it once.

goldens_features.npz holds per case the reference's saved files padded with zeros to T
(`energy/<name>`, `pitch/<name>`: normalised), the sha256 of the inputs (`sha/<name>`) and the
reference's own error against the float64 restatement (`err_e/<name>`: largest relative energy
error; `err_p/<name>`: largest absolute error of a normalised pitch); for the data set the
reference's `mean_std` (fp32) and the restatement's `mean_std64`; `sha/batch`.

Asserted here, on the reference alone:
  - reference and restatement are zero at the same tokens, for energy and pitch;
  - the reference's energy is within 2^-20 relative of the restatement (a broken golden, not
    a tolerance for the device: the tests use the recorded error);
  - every planted defect of the restatement changes at least one case.
"""
import ast
import os
import pickle
import sys
import tempfile
from pathlib import Path
from types import SimpleNamespace
from typing import List, Tuple

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))

import feature_cases as fc  # noqa: E402


def reference_functions(ref: Path, paths):
    """extract_pitch_energy, normalize_values as defined in <ref>/train_tacotron.py."""
    text = (ref / 'train_tacotron.py').read_text()
    wanted = ('normalize_values', 'extract_pitch_energy')
    defs = [n for n in ast.parse(text).body if isinstance(n, ast.FunctionDef) and n.name in wanted]
    assert sorted(d.name for d in defs) == sorted(wanted)

    def unpickle_binary(p):
        with open(p, 'rb') as f:
            return pickle.load(f)

    ns = {'np': np, 'Path': Path, 'Tuple': Tuple, 'List': List, 'paths': paths,
          'unpickle_binary': unpickle_binary, 'progbar': lambda *a: '', 'stream': lambda *a: None,
          'print': lambda *a, **k: None}
    exec(compile(ast.Module(body=defs, type_ignores=[]), str(ref / 'train_tacotron.py'), 'exec'), ns)
    return ns['extract_pitch_energy'], ns['normalize_values']


def write_dataset(root: Path, cases):
    """The reference's folder layout; the first half of the cases is the training set."""
    paths = SimpleNamespace(data=root, alg=root / 'alg', mel=root / 'mel', raw_pitch=root / 'raw_pitch',
                            phon_pitch=root / 'phon_pitch', phon_energy=root / 'phon_energy')
    for k in ('alg', 'mel', 'raw_pitch', 'phon_pitch', 'phon_energy'):
        getattr(paths, k).mkdir()
    for n, c in cases.items():
        np.save(paths.alg / f'{n}.npy', c['dur'][:c['x_len']], allow_pickle=False)
        np.save(paths.mel / f'{n}.npy', c['mel'][:, :c['mel_len']], allow_pickle=False)
        np.save(paths.raw_pitch / f'{n}.npy', c['pitch'][:c['pitch_len']], allow_pickle=False)
    data = [(n, c['mel_len']) for n, c in cases.items()]
    for name, part in (('train_dataset.pkl', data[:len(data) // 2]), ('val_dataset.pkl', data[len(data) // 2:])):
        with open(root / name, 'wb') as f:
            pickle.dump(part, f)
    return paths


def main():
    ref = Path(os.environ['FT_REFERENCE'])
    cases = fc.feature_cases()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        paths = write_dataset(Path(tmp), cases)
        extract_pitch_energy, _ = reference_functions(ref, paths)
        mean, std = extract_pitch_energy(paths.phon_pitch, paths.phon_energy, fc.PITCH_MAX)
        got = {n: (np.load(paths.phon_pitch / f'{n}.npy'), np.load(paths.phon_energy / f'{n}.npy'))
               for n in cases}
    assert np.asarray(mean).dtype == np.float32 and np.asarray(std).dtype == np.float32
    mine = {n: fc.run(c) for n, c in cases.items()}
    normed, mean64, std64 = fc.normalize([mine[n][0] for n in cases])
    changed = {d: [] for d in fc.DEFECTS}
    for (n, c), t in zip(cases.items(), normed):
        p, e = got[n]
        p64, e64 = mine[n]
        C, T = c['x_len'], len(c['dur'])
        assert p.dtype == e.dtype == np.float32 and p.shape == e.shape == (C,), n
        assert not p64[C:].any() and not e64[C:].any(), n
        assert np.array_equal(e == 0, e64[:C] == 0) and np.array_equal(p == 0, p64[:C] == 0), n
        live = e64[:C] != 0
        err_e = float(np.max(np.abs(e[live] - e64[:C][live]) / e64[:C][live], initial=0.0))
        err_p = float(np.max(np.abs(p - t[:C]), initial=0.0))
        assert err_e <= 2.0 ** -20, (n, err_e)
        out[f'energy/{n}'] = np.concatenate([e, np.zeros(T - C, np.float32)])
        out[f'pitch/{n}'] = np.concatenate([p, np.zeros(T - C, np.float32)])
        out[f'err_e/{n}'], out[f'err_p/{n}'] = np.float64(err_e), np.float64(err_p)
        out[f'sha/{n}'] = np.array(fc.sha(c))
        for d in fc.DEFECTS:
            bp, be = fc.run(c, d)
            if not (np.array_equal(bp, p64) and np.array_equal(be, e64, equal_nan=True)):
                changed[d].append(n)
        print(f'{n:22s} T {T:3d} mel_len {c["mel_len"]:4d} err_e {err_e / 2.0 ** -24:.2f} x 2^-24  err_p {err_p:.2e}')
    assert all(changed.values()), changed
    print('defects change:', changed)
    print(f'mean {mean!r} std {std!r}; restated {mean64!r} {std64!r}')
    assert abs(mean - mean64) <= 1e-5 * mean64 and abs(std - std64) <= 1e-5 * std64
    out['mean_std'] = np.array([mean, std], np.float32)
    out['mean_std64'] = np.array([mean64, std64], np.float64)
    b = fc.batch_case(cases)
    out['sha/batch'] = np.array(fc.sha(b))
    np.savez_compressed(HERE / 'goldens_features.npz', **out)


if __name__ == '__main__':
    main()
