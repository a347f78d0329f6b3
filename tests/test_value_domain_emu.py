"""CPU side of the value-domain tests (tests/test_gpu_value_domain.py): the numpy emulations of
the f16x3 GEMM and attention (tests/f16x3_emu.py) stay well inside the bounds the GPU tests
assert, on the same weight patterns and attention cases — so the bounds have headroom over the
arithmetic itself — and the defects those tests exist to catch, planted in the emulation only,
break the bounds: the neighbouring column's colscale, the bank groups' scales in unreversed
order, the small P V accumulator left out of the rescale, a neighbouring query's alpha."""
import numpy as np
import pytest

import f16x3_emu as E

RTOL = ATOL = 2e-5  # test_gpu_kernels.py


def _w0(rng, N, K):
    return rng.normal(0, 1 / np.sqrt(K), (N, K)).astype(np.float32)


def _patterns(rng, N, K):
    rows = E.rows_pattern(_w0(rng, N, K))
    outl = E.outlier_pattern(_w0(rng, N, K))
    bnd = E.rows_pattern(_w0(rng, N, K))
    E.boundary_rows(bnd, 17)
    return {'rows': rows, 'outlier': outl, 'boundary': bnd}


@pytest.mark.parametrize('xscale', [2.0 ** -8, 1.0, 2.0 ** 10])
def test_gemm_emulation_within_quarter_of_bound_a(xscale):
    """M = 96, K = 256, N = 64: the f16x3 arithmetic is within a quarter of bound A on every A
    weight pattern, for activations of 2^-8, 1 and 2^10."""
    rng = np.random.Generator(np.random.PCG64(11))
    x = (rng.normal(0, 1, (96, 256)) * xscale).astype(np.float32)
    for name, w in _patterns(rng, 64, 256).items():
        E.colscale_preconditions(E.split_weights_emu(w)[2])
        ref = x.astype(np.float64) @ w.astype(np.float64).T
        r = E.worst_ratio_a(E.gemm_emu(x, w), ref, ATOL, RTOL)
        assert r <= 0.25, (name, r)


def test_boundary_rows_scale_exponents():
    rng = np.random.Generator(np.random.PCG64(12))
    w = _w0(rng, 32, 96)
    want = E.boundary_rows(w, 9)
    assert E.scale_exponents(w)[9:14].tolist() == want
    assert np.abs(w[9]).max() == 16.0 and np.abs(w[10]).max() < 16.0 and np.abs(w[11]).max() == 32.0
    assert not w[12].any() and 0 < np.abs(w[13]).max() <= 2.0 ** -20
    x = rng.normal(0, 1, (8, 96)).astype(np.float32)
    got = E.gemm_emu(x, w)
    assert not got[:, 12].any()  # the all-zero row: exactly zero, and the bound asks for it


@pytest.mark.parametrize('pattern', ['rows', 'outlier'])
def test_neighbour_colscale_breaks_bound_a(pattern):
    """A local-for-global column index or an off-by-one: column n scaled by colscale[n + 1]."""
    rng = np.random.Generator(np.random.PCG64(13))
    x = rng.normal(0, 1, (96, 256)).astype(np.float32)
    w = _patterns(rng, 64, 256)[pattern]
    ref = x.astype(np.float64) @ w.astype(np.float64).T
    cs = E.split_weights_emu(w)[2]
    r = E.worst_ratio_a(E.gemm_emu(x, w, colscale=np.roll(cs, -1)), ref, ATOL, RTOL)
    assert r > 100, r
    # the clamp col < N ? col : N - 1 applied to a live column
    r = E.worst_ratio_a(E.gemm_emu(x, w, colscale=np.full_like(cs, cs[-1])), ref, ATOL, RTOL)
    assert r > 100, r


def test_unreversed_group_scales_break_bound_a():
    """The halves weight image stores the groups' scales in reversed group order and reads
    them back reversed: reading them unreversed gives group g the scales of group G - 1 - g."""
    rng = np.random.Generator(np.random.PCG64(14))
    G, C, K = 4, 32, 64
    x = rng.normal(0, 1, (50, K)).astype(np.float32)
    ws = [E.rows_pattern(_w0(rng, C, K), group=g) for g in range(G)]
    cs = [E.split_weights_emu(w)[2] for w in ws]
    for g in range(G - 1):
        assert np.any(cs[g] != cs[g + 1])
    ref = np.concatenate([x.astype(np.float64) @ w.astype(np.float64).T for w in ws], 1)
    good = np.concatenate([E.gemm_emu(x, w) for w in ws], 1)
    assert E.worst_ratio_a(good, ref, 5e-5, 5e-5) <= 0.25
    bad = np.concatenate([E.gemm_emu(x, w, colscale=cs[G - 1 - g]) for g, w in enumerate(ws)], 1)
    assert E.worst_ratio_a(bad, ref, 5e-5, 5e-5) > 100


@pytest.fixture(scope='module')
def attn_runs():
    """Every B case once: (case, bound, E32, floor, emulated error, errors of the two planted
    defects)."""
    out = []
    for c in E.ATTN_CASES:
        qkv, mask, r64, r32 = E.attention_case(*c)
        moves = E.attention_preconditions(c[0], c[1], qkv, mask, 2)
        bound, e32 = E.attention_bound(r64, r32, qkv)
        ok = np.isfinite(r64)

        def err(**kw):
            o = E.attention_emu(qkv, 2, mask, **kw)
            assert np.array_equal(np.isnan(o), ~ok)  # NaN exactly on the fully masked item
            return float(np.abs(o - r64)[ok].max())
        out.append(dict(case=c, moves=moves, bound=bound, e32=e32,
                        floor=bound - E.ATTN_F * e32, err=err(),
                        no_osm=err(skip_osm_rescale=True), nb_alpha=err(neighbour_alpha=True)))
    return out


def test_attention_cases_cover_the_issue():
    """Every profile at a T that is a multiple of the tile and one that is not, T = 64, every
    mask kind, both head dims, both gain patterns."""
    for p in E.PROFILES:
        ts = [c[2] for c in E.ATTN_CASES if c[0] == p]
        assert any(t % 64 == 0 for t in ts) and any(t % 64 for t in ts), p
    assert {c[2] for c in E.ATTN_CASES} >= {64, 128, 192, 200, 257}
    assert {c[4] for c in E.ATTN_CASES} == set(E.MASKS)
    assert {c[3] for c in E.ATTN_CASES} == {64, 128}
    assert {c[1] for c in E.ATTN_CASES} == {'one', 'mixed'}


def test_attention_emulation_within_half_of_bound_b(attn_runs):
    worst = 0.0
    for r in attn_runs:
        assert r['err'] <= E.ATTN_F / 2 * r['e32'] + r['floor'], r
        worst = max(worst, r['err'] / r['e32'])
        if r['case'][0] in ('ramp', 'saw', 'peak') and r['case'][2] >= 192:
            assert r['moves'] >= 100, r  # randn inputs: 0
    assert 2 * worst <= E.ATTN_F <= 4, worst


def test_attention_planted_defects_break_bound_b(attn_runs):
    """On every ramp / saw case (the ones that move the max repeatedly): the small accumulator
    left out of the rescale, and a neighbouring query's alpha, both miss bound B."""
    n = 0
    for r in attn_runs:
        if r['case'][0] in ('ramp', 'saw'):
            assert r['no_osm'] > r['bound'], r
            assert r['nb_alpha'] > r['bound'], r
            n += 1
    assert n >= 4


def test_panel_layernorm_emulation_within_quarter_of_bound_a():
    """panel_proj's LayerNorm cases (rows pattern, exponents 0 .. 3, bias and residual, then
    LayerNorm over the 256 columns): the emulated GEMM followed by an exact LayerNorm is within
    a quarter of bound A at panel_proj's 1e-5."""
    rng = np.random.Generator(np.random.PCG64(15))
    M, K, N = 37, 256, 256
    x = rng.normal(0, 1, (M, K)).astype(np.float32)
    w = E.rows_pattern(_w0(rng, N, K), lo=0, hi=3)
    assert len(np.unique(E.split_weights_emu(w)[2])) >= 4
    b = rng.normal(0, 0.1, N)
    r = rng.normal(0, 1, (M, N))
    g, bt = rng.normal(1, 0.2, N), rng.normal(0, 0.2, N)

    def ln(z):
        mu = z.mean(1, keepdims=True)
        return (z - mu) / np.sqrt(((z - mu) ** 2).mean(1, keepdims=True) + 1e-5) * g + bt
    ref = ln(x.astype(np.float64) @ w.astype(np.float64).T + b + r)
    got = ln((E.gemm_emu(x, w) + b.astype(np.float32) + r.astype(np.float32)).astype(np.float64))
    assert E.worst_ratio_a(got, ref, 1e-5, 1e-5) <= 0.25


def test_rescaled_checkpoints_keep_the_function():
    """The checkpoint rescalings of the whole-model GPU tests: FastPitch's is exact (powers of
    two through linear maps, ReLU and q k^T); ForwardTacotron's function-preserving part moves
    the output only through eps next to the scaled running_var; both leave weights whose rows
    ask for many distinct column scales."""
    import torch
    from forwardtacotron_amd.fast_pitch import FastPitch
    from forwardtacotron_amd.forward_tacotron import ForwardTacotron
    from forwardtacotron_amd.synthetic import default_config, synthetic_state_dict, synthetic_tokens
    from oracle import fp_torch_cpu as FTC
    from oracle import ft_torch_cpu as TC
    x = torch.from_numpy(synthetic_tokens(2, 12, seed=0, min_len=8))
    sd = synthetic_state_dict(FastPitch.from_config(default_config()), 0, 'fast_pitch')
    sd2 = E.rescale_fast_pitch({k: v.copy() for k, v in sd.items()})
    k = 'prenet.layers.0.conv1.weight'
    assert len(np.unique(E.scale_exponents(sd2[k]))) >= 8 > len(np.unique(E.scale_exponents(sd[k])))
    a = FTC.generate(FTC.to_torch(sd, torch.float64), x)
    b = FTC.generate(FTC.to_torch(sd2, torch.float64), x)
    assert torch.equal(a['mel'], b['mel']) and torch.equal(a['dur'], b['dur'])
    sd = synthetic_state_dict(ForwardTacotron.from_config(default_config()), seed=0)
    sd2 = E.rescale_forward_tacotron({k: v.copy() for k, v in sd.items()})
    for k in ('prenet.conv1d_bank.3.conv.weight', 'postnet.highways.2.W1.weight'):
        assert len(np.unique(E.scale_exponents(sd2[k]))) >= 8 > len(np.unique(E.scale_exponents(sd[k])))
    for k in ('lstm.weight_ih_l0', 'lstm.weight_ih_l0_reverse', 'lin.weight', 'lin.bias'):
        sd2[k] = sd[k]  # the rows scaled outright change the network: put back for this check
    a = TC.generate(TC.to_torch(sd, torch.float64), x)
    b = TC.generate(TC.to_torch(sd2, torch.float64), x)
    assert torch.equal((a['dur'] + 0.5).long(), (b['dur'] + 0.5).long())
    assert float((a['mel_post'] - b['mel_post']).abs().max()) <= 1e-3 * float(a['mel_post'].abs().max())
