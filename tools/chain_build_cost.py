"""Host cost of recording a launch list (forwardtacotron_amd/chain.py): batch-1 generate() over
sentences whose length never repeats, so every call records three predictor plans and one
prenet plan, against the same run with FTMI_CHAIN=0 (a launch per op) and against a run whose
lengths repeat (the plans are reused).  Wall time per call, synchronised.
usage: python tools/chain_build_cost.py (GPU)"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from forwardtacotron_amd import chain  # noqa: E402
from forwardtacotron_amd import forward_tacotron as FT  # noqa: E402
from forwardtacotron_amd.synthetic import default_config, synthetic_state_dict, synthetic_tokens  # noqa: E402


def run(model, lengths):
    xs = [torch.from_numpy(synthetic_tokens(1, T, seed=T, min_len=T)).cuda() for T in lengths]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for x in xs:
        model.generate(x)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / len(xs) * 1e3


def main():
    FT.GRAPH = False  # eager phases: the graph path has its own second-sighting rule
    model = FT.ForwardTacotron.from_config(default_config())
    sd = synthetic_state_dict(model, seed=0, model='forward_tacotron')
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    model = model.cuda().eval()
    run(model, [40, 41])  # packs, allocator
    res = {}
    chain.CHAIN = False
    res['per_op_new_lengths'] = run(model, range(60, 100))
    chain.CHAIN = True
    n0 = chain.BUILDS
    res['chain_new_lengths'] = run(model, range(100, 140))
    res['plans_built'] = chain.BUILDS - n0
    run(model, [150] * 2)
    res['chain_repeated_length'] = run(model, [150] * 40)
    chain.CHAIN = False
    res['per_op_repeated_length'] = run(model, [150] * 40)
    print({k: round(v, 3) for k, v in res.items()})


if __name__ == '__main__':
    main()
