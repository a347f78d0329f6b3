"""Alignment goldens from the reference (utils/duration_extraction.py, utils/metrics.py).

Build container only (imports the reference and scipy, absent on the GPU box):

    FT_REFERENCE=<reference checkout> python tests/golden/make_goldens_align.py

Inputs come from tests/align_cases.py (fixed seeds).  goldens_align.npz holds, per duration
case, the reference's durations for both methods (`dij/<name>`, `cnt/<name>`), scipy's
dist_matrix[-1] as float64 (`cost/<name>`) and the sha256 of the input bytes (`sha/<name>`);
for the batch input its sha256; for the scores the reference's fp32 results per r
(`loc32/<r>`, `sharp32/<r>`) and the fp64 values (`loc64/<r>`, `sharp64/<r>`: the exact count
over L - 1, and the reference run on att.double()).

Asserted here, on the reference alone:
  - every duration case not marked `tied` has a unique shortest path, and there the
    restatement of tests/align_cases.py gives the reference's durations and scipy's distance
    bit for bit; the tied case agrees with scipy under the diagonal-first rule;
  - the restatement's peak-count durations equal the reference's in every case;
  - the reference's fp32 loc equals the correctly rounded exact quotient.
"""
import os
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
if os.environ.get('FT_REFERENCE'):  # else the reference is expected on PYTHONPATH
    sys.path.insert(0, os.environ['FT_REFERENCE'])

from scipy.sparse.csgraph import dijkstra  # noqa: E402
from utils.duration_extraction import (extract_durations_per_count,  # noqa: E402  (reference)
                                       extract_durations_with_dijkstra, to_adj_matrix)
from utils.metrics import attention_score  # noqa: E402  (reference)

import align_cases as ac  # noqa: E402


def main():
    out = {}
    cases = ac.duration_cases()
    for name, c in cases.items():
        att, R, C = c['att'], c['mel_len'], c['x_len']
        seq = np.zeros(C, np.int64)
        if R * C == 1:  # a one-node graph has no predecessor of its last node: the reference's
            dij = np.ones(1, np.int32)  # walk raises there; the one frame goes to the one token
        else:
            dij = extract_durations_with_dijkstra(seq, att[:, :C], R)
        cnt = extract_durations_per_count(seq, att[:, :C], R)
        dist = dijkstra(csgraph=to_adj_matrix(1. - att[:R, :C]), directed=True, indices=0)
        cost = np.float64(dist[-1])
        mine, mycost, unique = ac.durations_dp(att, R, C)
        assert unique != c['tied'], (name, unique)
        assert np.array_equal(mine[:C], dij) and not mine[C:].any(), (name, mine, dij)
        assert mycost == cost, (name, mycost, cost)
        assert np.array_equal(ac.durations_count(att, R, C)[:C], cnt), name
        assert dij.sum() == R and cnt.sum() == R, name
        pad = np.zeros(att.shape[1] - C, np.int32)
        out[f'dij/{name}'] = np.concatenate([dij.astype(np.int32), pad])
        out[f'cnt/{name}'] = np.concatenate([cnt.astype(np.int32), pad])
        out[f'cost/{name}'] = cost
        out[f'sha/{name}'] = np.array(ac.sha(att))
        print(f'{name:18s} {att.shape} cost {cost:.6f} unique {unique}')
    out['sha/batch'] = np.array(ac.sha(ac.batch_case(cases)['att']))

    att = ac.score_case()
    out['sha/scores'] = np.array(ac.sha(att))
    for r in ac.SCORE_R:
        ml = ac.SCORE_MEL_LENS[r]
        loc32, sharp32 = attention_score(torch.from_numpy(att), torch.tensor(ml), r=r)
        _, sharp64 = attention_score(torch.from_numpy(att).double(), torch.tensor(ml), r=r)
        loc64, mysharp = ac.scores(att, ml, r)
        assert loc32.dtype == torch.float32 and sharp64.dtype == torch.float64
        assert np.array_equal(loc64.astype(np.float32), loc32.numpy()), (r, loc64, loc32)
        assert np.abs(mysharp - sharp64.numpy()).max() <= 2.0 ** -50, (r, mysharp, sharp64)
        assert 0.3 < loc64.min() < 1.0, loc64  # some jumps, not all
        out[f'loc32/{r}'], out[f'sharp32/{r}'] = loc32.numpy(), sharp32.numpy()
        out[f'loc64/{r}'], out[f'sharp64/{r}'] = loc64, sharp64.numpy()
        print(f'scores r={r}: loc {loc64} sharp {sharp64.numpy()}')
    np.savez_compressed(HERE / 'goldens_align.npz', **out)


if __name__ == '__main__':
    main()
