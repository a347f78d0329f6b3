"""Launch lists (ftmi_run_chain / forwardtacotron_amd.chain): a SeriesPredictor's chain issued
by one native call must return the BITS of the per-op path (`torch.equal`, no tolerance): the
list is recorded from that path, so any difference means the plan diverged from its decisions.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

S = 135  # symbols
# GEMV recurrence at B <= 4, the first MFMA batch at 5, a second 16-sequence chunk with one
# live row; T below the 5 taps; T = 0, 1, 2 mod 3 (the projection prefetch ring)
SHAPES = [(1, 1), (1, 2), (2, 4), (3, 33), (4, 61), (5, 64), (17, 130)]
PATHS = ['f16x3', 'bf16x6', 'fp32']


def _predictor(rnn_dims, seed=0, conv_gain=1.0):
    from forwardtacotron_amd.forward_tacotron import SeriesPredictor
    torch.manual_seed(seed)
    m = SeriesPredictor(S, 64, 256, rnn_dims)
    with torch.no_grad():
        for c in m.convs:  # BN statistics off their defaults, scales of both signs
            n = c.bnorm.weight.numel()
            c.bnorm.weight.copy_(torch.empty(n).uniform_(0.5, 1.5) * (torch.randint(0, 2, (n,)) * 2 - 1))
            c.bnorm.bias.normal_(0, 0.1)
            c.bnorm.running_mean.normal_(0, 0.1)
            c.bnorm.running_var.uniform_(0.5, 1.5)
        m.convs[0].conv.weight.mul_(conv_gain)
    return m.cuda().eval()


def _ids(B, T, seed=0):
    """Random ids, pad ids (0) in the tail of every sequence but the first."""
    rng = np.random.Generator(np.random.PCG64(seed * 1000 + B * 131 + T))
    ids = rng.integers(1, S, (B, T))
    for b in range(1, B):
        ids[b, T - (b * 7) % (T // 2 + 1):] = 0
    return torch.from_numpy(ids.astype(np.int64)).cuda()


@pytest.fixture(scope='module')
def preds():
    return {h: _predictor(h, seed=h) for h in (64, 128)}


def _per_op(monkeypatch, mod, x, alpha):
    from forwardtacotron_amd import chain
    monkeypatch.setattr(chain, 'CHAIN', False)
    y = mod.forward_bt(x, alpha)
    monkeypatch.setattr(chain, 'CHAIN', True)
    return y


def _plan(mod, x):
    """The plan a predictor runs for x under the current settings."""
    from forwardtacotron_amd import chain
    plan = chain.cached_plan(mod, x)
    assert plan is not None
    return plan


def _path(monkeypatch, path):
    """Context of one matrix path; the default needs nothing."""
    import contextlib

    from forwardtacotron_amd import ops
    if path == 'bf16x6':
        monkeypatch.setattr(ops, 'MMA', 1)
        monkeypatch.setattr(ops, 'RNN_MMA', 1)
    return ops.exact_paths() if path == 'fp32' else contextlib.nullcontext()


@pytest.mark.parametrize('path', PATHS)
@pytest.mark.parametrize('rnn_dims', [64, 128])
@pytest.mark.parametrize('B,T', SHAPES)
def test_predictor_chain_equals_per_op(B, T, rnn_dims, path, preds, monkeypatch):
    from forwardtacotron_amd import chain, ops
    mod, x = preds[rnn_dims], _ids(B, T)
    st = ops.status_word('cuda')
    st.zero_()
    with _path(monkeypatch, path):
        ref = _per_op(monkeypatch, mod, x, 1.3)
        n0 = chain.BUILDS
        first = mod.forward_bt(x, 1.3)      # records (or finds) the plan
        second = mod.forward_bt(x, 1.3)     # the launch list
        third = mod.forward_bt(x, 0.7)      # alpha is patched, not planned
        assert chain.BUILDS - n0 <= 1
        ref7 = _per_op(monkeypatch, mod, x, 0.7)
    torch.cuda.synchronize()
    assert int(st.item()) == 0
    assert torch.isfinite(ref).all() and float(ref.abs().max()) > 0
    assert torch.equal(first, ref) and torch.equal(second, ref)
    assert torch.equal(third, ref7) and not torch.equal(ref7, ref)


def test_workspace_contents_do_not_matter(preds, monkeypatch):
    """The workspace pre-filled with NaNs, then with another pattern: same bits; the words
    after the planned size are never written."""
    mod, x = preds[128], _ids(5, 64)
    ref = _per_op(monkeypatch, mod, x, 1.3)
    mod.forward_bt(x, 1.3)
    plan = _plan(mod, x)
    guard = 256
    buf = torch.empty(plan.ws_bytes + guard, device='cuda', dtype=torch.uint8)
    for fill in (0xFF, 0x5A):  # 0xFFFFFFFF is a NaN
        buf.fill_(fill)
        y = plan.run(x, 1.3, ws=buf[:plan.ws_bytes])
        torch.cuda.synchronize()
        assert torch.equal(y, ref), hex(fill)
        assert bool((buf[plan.ws_bytes:] == fill).all()), hex(fill)


def test_three_streams(monkeypatch):
    """Three predictors on three streams, each with its own workspace, against their serial
    results."""
    mods = [_predictor(h, seed=10 + i) for i, h in enumerate((64, 128, 64))]
    x = _ids(5, 64, seed=3)
    refs = [_per_op(monkeypatch, m, x, 1.0) for m in mods]
    for m in mods:
        m.forward_bt(x)  # record
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in mods]
    outs = []
    for m, s in zip(mods, streams):
        with torch.cuda.stream(s):
            outs.append(m.forward_bt(x))
    torch.cuda.synchronize()
    for y, r in zip(outs, refs):
        assert torch.equal(y, r)


def test_graph_capture(preds, monkeypatch):
    mod, x = preds[64], _ids(3, 33)
    ref = _per_op(monkeypatch, mod, x, 1.0)
    mod.forward_bt(x)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        y = mod.forward_bt(x)
    y.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, ref)


def _raw(plan, x, ws, out, n=None):
    from forwardtacotron_amd import _lib, chain, ops
    b = plan.bases
    b[chain.SLOT_IDS].base, b[chain.SLOT_OUT].base = x.data_ptr(), out.data_ptr()
    if ws is not None:
        b[chain.SLOT_WS].base = ws
    failed = ctypes.c_int32(-7)
    rc = _lib.load().ftmi_run_chain(plan.ops, plan.n if n is None else n, plan.bases, plan.n_bases,
                                    ctypes.byref(failed), ops._stream())
    return rc, failed.value


def test_validation_launches_nothing(monkeypatch):
    """An offset past its slot, a misaligned workspace, a workspace one byte short, n = 0 and
    an unknown tag: the error code, the op named, nothing launched (the output keeps its
    sentinel) and the status word untouched."""
    from forwardtacotron_amd import chain, ops
    mod, x = _predictor(64, seed=5), _ids(5, 64)
    ref = _per_op(monkeypatch, mod, x, 1.0)
    mod.forward_bt(x)
    plan = _plan(mod, x)
    ws = torch.empty(plan.ws_bytes + 16, device='cuda', dtype=torch.uint8)
    out = torch.full(plan.out_shape, -123.0, device='cuda')
    st = ops.status_word('cuda')
    st.fill_(8)  # no kernel sets this bit: any write to the word shows
    conv = next(k for k in range(plan.n) if plan.ops[k].tag == 2)

    ref_x = plan.ops[conv].p[0]
    keep = ref_x.offset
    ref_x.offset = plan.ws_bytes
    assert _raw(plan, x, ws.data_ptr(), out) == (1001, conv)
    ref_x.offset = keep
    assert _raw(plan, x, ws.data_ptr() + 4, out) == (1004, 0)
    plan.bases[chain.SLOT_WS].bytes -= 1
    rc, k = _raw(plan, x, ws.data_ptr(), out)
    plan.bases[chain.SLOT_WS].bytes += 1
    assert rc == 1001 and 0 <= k < plan.n
    assert _raw(plan, x, ws.data_ptr(), out, n=0) == (1001, -1)
    plan.ops[plan.n - 1].tag = 99
    assert _raw(plan, x, ws.data_ptr(), out) == (1001, plan.n - 1)
    plan.ops[plan.n - 1].tag = 4
    torch.cuda.synchronize()
    assert bool((out == -123.0).all()) and int(st.item()) == 8
    st.zero_()
    assert _raw(plan, x, ws.data_ptr(), out) == (0, -1)  # the list itself is sound
    torch.cuda.synchronize()
    assert torch.equal(out, ref) and int(st.item()) == 0


def test_failing_op_stops_the_list(monkeypatch):
    """An op whose entry point refuses its arguments stops the list and raises the binding's
    FtmiError, naming the op."""
    from forwardtacotron_amd import _lib
    mod, x = _predictor(64, seed=6), _ids(3, 33)
    mod.forward_bt(x)
    plan = _plan(mod, x)
    convs = [k for k in range(plan.n) if plan.ops[k].tag == 2]
    k = convs[1]
    mma = plan.ops[k].i[12]
    plan.ops[k].i[12] = 7  # unknown matrix path: ftmi_conv1d returns FTMI_E_ARG
    try:
        with pytest.raises(_lib.FtmiError, match=rf'status 1001.*\(op {k}: conv1d'):
            mod.forward_bt(x)
    finally:
        plan.ops[k].i[12] = mma
        torch.cuda.synchronize()
    assert torch.isfinite(mod.forward_bt(x)).all()


def test_range_guard(monkeypatch):
    """Activations beyond the f16 range (conv1's weights x 1e6): the list sets the status bits
    of the per-op path, and run_checked reruns on the exact paths to the same result."""
    from forwardtacotron_amd import chain, ops
    mod, x = _predictor(64, seed=7, conv_gain=1e6), _ids(5, 64)
    st = ops.status_word('cuda')

    def word(fn):
        st.zero_()
        fn()
        torch.cuda.synchronize()
        return int(st.item())

    monkeypatch.setattr(chain, 'CHAIN', False)
    w_ref = word(lambda: mod.forward_bt(x))
    ref = ops.run_checked(lambda: mod.forward_bt(x), x.device)
    monkeypatch.setattr(chain, 'CHAIN', True)
    mod.forward_bt(x)
    assert w_ref & ops.STATUS_F16_RANGE and word(lambda: mod.forward_bt(x)) == w_ref
    ops.run_checked(lambda: mod.forward_bt(x), x.device)  # records the exact-path plan
    y = ops.run_checked(lambda: mod.forward_bt(x), x.device)
    assert int(st.item()) == w_ref and torch.isfinite(ref).all() and torch.equal(y, ref)


def test_plan_cache(monkeypatch):
    """A second call at a shape builds nothing; load_state_dict, an in-place weight update and
    a new (B, T) build one plan each — and the new weights are the ones used."""
    from forwardtacotron_amd import chain
    mod, x = _predictor(64, seed=8), _ids(3, 33)
    n = chain.BUILDS
    mod.forward_bt(x)
    assert chain.BUILDS == n + 1
    mod.forward_bt(x)
    mod.forward_bt(x, 0.5)
    assert chain.BUILDS == n + 1
    mod.forward_bt(_ids(2, 4))
    assert chain.BUILDS == n + 2
    mod.forward_bt(x)
    assert chain.BUILDS == n + 2
    mod.load_state_dict(_predictor(64, seed=9).state_dict())
    mod.forward_bt(x)
    assert chain.BUILDS == n + 3
    with torch.no_grad():
        mod.lin.weight.mul_(2.0)
    mod.forward_bt(x)
    y = mod.forward_bt(x)
    assert chain.BUILDS == n + 4
    assert torch.equal(y, _per_op(monkeypatch, mod, x, 1.0))


def test_routing_switch_builds_another_plan(monkeypatch):
    """A routing switch of the library toggled between two calls (FTMI_GEMM_SKINNY: the 80
    rows' convs leave the skinny kernel, so the recorded splits no longer hold) reaches the
    plan cache through the library's digest: a second plan is recorded, the first one is not
    replayed, and each call returns the bits of the per-op path under the same setting."""
    from forwardtacotron_amd import chain
    mod, x = _predictor(64, seed=12), _ids(2, 40)
    monkeypatch.delenv('FTMI_GEMM_SKINNY', raising=False)
    n = chain.BUILDS
    first = mod.forward_bt(x, 1.3)
    plan = _plan(mod, x)
    assert chain.BUILDS == n + 1
    ref = _per_op(monkeypatch, mod, x, 1.3)
    monkeypatch.setenv('FTMI_GEMM_SKINNY', '0')
    assert chain.cached_plan(mod, x) is None
    second = mod.forward_bt(x, 1.3)
    assert chain.BUILDS == n + 2 and _plan(mod, x) is not plan
    replay = mod.forward_bt(x, 1.3)
    ref0 = _per_op(monkeypatch, mod, x, 1.3)
    monkeypatch.delenv('FTMI_GEMM_SKINNY')
    assert _plan(mod, x) is plan and chain.BUILDS == n + 2
    torch.cuda.synchronize()
    assert torch.isfinite(ref).all() and float(ref.abs().max()) > 0
    assert torch.equal(first, ref)
    assert torch.equal(second, ref0) and torch.equal(replay, ref0)


def test_probe_entry(preds):
    """Under a KernelProbe the chain is one entry with its ops' summed work."""
    from forwardtacotron_amd.probe import KernelProbe
    mod, x = preds[64], _ids(5, 64)
    mod.forward_bt(x)
    with KernelProbe() as p:
        mod.forward_bt(x)
    torch.cuda.synchronize()
    s = p.summary()
    assert list(s) == ['series_predictor[B=5,T=64,H=64]']
    e = s['series_predictor[B=5,T=64,H=64]']
    assert e['entry'] == 'ftmi_run_chain' and e['launches'] == 1
    assert e['flops'] > 2.0 * 5 * 64 * 256 * 5 * 256 * 2 and e['bytes'] > 0


def _batch(x, seed=0):
    rng = np.random.Generator(np.random.PCG64(seed))
    B, T = x.shape
    dur = rng.integers(1, 5, (B, T)).astype(np.float32)
    lens = dur.sum(1).astype(np.int64)
    return {'x': x, 'mel': torch.from_numpy(rng.normal(0, 1, (B, 80, int(lens.max()))).astype(np.float32)).cuda(),
            'mel_len': torch.from_numpy(lens), 'dur': torch.from_numpy(dur).cuda(),
            'pitch': torch.from_numpy(rng.normal(0, 1, (B, T)).astype(np.float32)).cuda(),
            'energy': torch.from_numpy(rng.normal(0, 1, (B, T)).astype(np.float32)).cuda()}


def test_model_level(gpu_model, monkeypatch):
    """generate, generate_jit and the packed forward at B = 3, T = 20, switch on against off
    (generate three times each: eager, the capturing call, a replay)."""
    from forwardtacotron_amd import chain
    x = _ids(3, 20, seed=4)

    def run():
        torch.cuda.synchronize()
        for k in ('_ftmi_graphs', '_ftmi_graph_seen'):  # each leg captures its own phase
            gpu_model.__dict__.pop(k, None)
        outs = [gpu_model.generate(x, alpha=1.1) for _ in range(3)]
        outs.append(gpu_model.generate_jit(x, alpha=0.9, beta=1.2))
        outs.append(gpu_model.generate_jit(x, alpha=0.9, beta=1.2))
        outs.append(gpu_model(_batch(x)))
        outs.append(gpu_model(_batch(x)))
        torch.cuda.synchronize()
        return outs

    monkeypatch.setattr(chain, 'CHAIN', False)
    ref = run()
    monkeypatch.setattr(chain, 'CHAIN', True)
    got = run()
    for a, b in zip(got, ref):
        assert set(a) == set(b)
        for k in a:
            assert torch.equal(a[k], b[k]), k


def test_ids_view_with_8_byte_alignment(preds, monkeypatch):
    """A plan recorded from a 16-byte aligned ids tensor must serve a later call whose ids are a
    row slice at an odd multiple of 8 bytes (odd T): the entry points read ids as scalars, so
    the per-op path accepts it and the list must too."""
    mod = preds[64]
    B, T = 3, 33
    x = _ids(B, T)
    assert x.data_ptr() % 16 == 0
    mod.forward_bt(x)
    whole = torch.cat([_ids(1, T, seed=9), _ids(B, T, seed=5)])
    view = whole[1:]
    assert view.is_contiguous() and view.data_ptr() % 16 == 8
    assert _plan(mod, view) is _plan(mod, x)
    y = mod.forward_bt(view)
    assert torch.equal(y, _per_op(monkeypatch, mod, view, 1.0))


def test_plan_cache_is_bounded():
    from forwardtacotron_amd import chain
    mod = _predictor(64, seed=11)
    for T in range(2, 2 + chain.MAX_PLANS + 3):
        mod.forward_bt(_ids(1, T))
    assert len(mod.__dict__['_ftmi_chain'][1]) == chain.MAX_PLANS
