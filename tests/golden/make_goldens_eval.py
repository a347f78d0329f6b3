"""Validation-loss goldens from the reference (trainer/common.py MaskedL1, F.l1_loss,
F.cross_entropy, utils/distribution.py discretized_mix_logistic_loss).

Build container only (reads the reference checkout, absent on the GPU box):

    FT_REFERENCE=<reference checkout> python tests/golden/make_goldens_eval.py

The reference's modules are imported from the given path; nothing of them is copied.  Every case
of tests/eval_cases.py runs twice: on its fp32 inputs, the reference as it runs (`f32/<name>`),
and on the same values widened to float64 (`f64/<name>`), which is the yardstick.  One operand
stays fp32 in the widened run: the mixture loss's `y`.  The reference tests `y < -0.999` and
`y > 0.999` on the fp32 tensor, where torch compares in fp32 against the fp32 constants; a float64
`y` equal to float32(0.999) would be compared against the double 0.999 and change sides.  With a
float64 `y_hat`, `y - means` and everything after it is float64 arithmetic all the same.

goldens_eval.npz holds per case `sha/<name>`, `f32/<name>`, `f64/<name>` and `err/<name>` =
|f32 - f64| / |f64| (NaN where the result is NaN; for the reduce=False cases the vectors and
the largest relative error).  Inputs are regenerated from seeds by the tests, never stored.

Asserted here, on the reference alone: the float64 restatement of tests/eval_cases.py equals the
widened run within 1e-12 relative, and the rejected cross-entropy case is rejected by torch too.
"""
import os
import sys
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))

import eval_cases as ec  # noqa: E402


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if np.isnan(b).any():
        assert np.array_equal(np.isnan(a), np.isnan(b))
        return float('nan')
    return float(np.max(np.abs(a - b) / np.abs(b)))


def main():
    sys.path.insert(0, os.environ['FT_REFERENCE'])
    from trainer.common import MaskedL1
    from utils.distribution import discretized_mix_logistic_loss
    masked = MaskedL1()
    out = {}

    def record(name, case, f32, f64, mine):
        f32, f64 = np.asarray(f32, np.float32), np.asarray(f64, np.float64)
        err, own = rel(f32, f64), rel(mine, f64)
        assert np.isnan(own) or own <= 1e-12, (name, own)
        out[f'sha/{name}'] = np.array(ec.sha(case))
        out[f'f32/{name}'], out[f'f64/{name}'], out[f'err/{name}'] = f32, f64, np.float64(err)
        print(f'{name:16s} own error {err / 2.0 ** -23:10.3f} x 2^-23   restatement {own:.2e}')

    with torch.no_grad():
        for n, c in ec.l1_cases().items():
            x, t = torch.from_numpy(c['x']), torch.from_numpy(c['target'])
            if 'lens' in c:
                lens = torch.from_numpy(c['lens'])
                f32, f64 = masked(x, t, lens), masked(x.double(), t.double(), lens)
            else:
                f32, f64 = F.l1_loss(x, t), F.l1_loss(x.double(), t.double())
            assert f32.dtype == torch.float32 and f64.dtype == torch.float64
            record(f'l1/{n}', c, f32.numpy(), f64.numpy(), ec.run_l1(c))
        for n, c in ec.ce_cases().items():
            x, t = torch.from_numpy(c['logits']), torch.from_numpy(c['target'])
            if 'batch' in c:
                B = c['batch']
                x, t = x.view(B, -1, x.size(1)).transpose(1, 2), t.view(B, -1)
            f32, f64 = F.cross_entropy(x, t), F.cross_entropy(x.double(), t)
            record(f'ce/{n}', c, f32.numpy(), f64.numpy(), ec.cross_entropy(c['logits'], c['target']))
        bad = ec.ce_rejected()
        try:
            F.cross_entropy(torch.from_numpy(bad['logits']), torch.from_numpy(bad['target']))
            raise AssertionError('torch accepted the rejected case')
        except (IndexError, RuntimeError):
            pass
        out['sha/ce/rejected'] = np.array(ec.sha(bad))
        for n, c in ec.mol_cases().items():
            h, y = torch.from_numpy(c['y_hat']), torch.from_numpy(c['y'])
            kw = {'num_classes': c['num_classes'], 'reduce': c['reduce']}
            if 'log_scale_min' in c:
                kw['log_scale_min'] = c['log_scale_min']
            f32 = discretized_mix_logistic_loss(h, y, **kw)
            f64 = discretized_mix_logistic_loss(h.double(), y, **kw)  # y stays fp32: see above
            assert f32.dtype == torch.float32 and f64.dtype == torch.float64
            record(f'mol/{n}', c, f32.numpy(), f64.numpy(), ec.run_mol(c))
    np.savez_compressed(HERE / 'goldens_eval.npz', **out)


if __name__ == '__main__':
    main()
