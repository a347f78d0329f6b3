"""tests/seq_cases.py checked on the host: every restatement against an independent statement
of the same operation (the numpy oracle, torch on the CPU), every table against the branch it
names, and every planted defect against the comparison the device test uses
(tests/test_gpu_seq_kernels.py): bit equality, or tests/test_gpu_kernels.close's bound."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import seq_cases as S
from oracle import ft_oracle as O
from test_gpu_kernels import ATOL, RTOL


# --- restatements against independent statements ----------------------------------------------

@pytest.mark.parametrize('rows,dim,shape,seed', S.EMBED)
def test_embedding_ref_is_nn_embedding_inside_the_table(rows, dim, shape, seed):
    table = S.embed_table(rows, dim, seed)
    sets = S.embed_id_sets(rows, shape, seed)
    assert any(k != 'clean' for k in sets)
    seen = set()
    assert np.abs(table).min() > 0  # a zero row is told from every table row
    for name, ids in sets.items():
        out, outside = S.embedding_ref(ids, table)
        ok = (ids >= 0) & (ids < rows)
        assert outside == (not ok.all()) == (not name.startswith('clean'))
        want = F.embedding(torch.from_numpy(np.where(ok, ids, 0)), torch.from_numpy(table)).numpy()
        assert S.same_bits(out[ok], want[ok]) and not out[~ok].any()
        seen |=set(ids.reshape(-1).tolist())
    assert seen >= {0, rows - 1, *S.outside_ids(rows)}


@pytest.mark.parametrize('n,seed', S.TRUNC)
def test_trunc_sum_ref_is_the_exact_integer_sum(n, seed):
    v = S.trunc_tensor(n, seed)
    want = sum(math.trunc(float(x)) for x in v)
    assert S.trunc_sum_ref(v) == want == int(np.sum(v.astype(np.int64)))
    assert want > 2 ** 31  # the sum leaves int32
    assert {3.0e9}.issubset(set(v.tolist())) and (n < 8 or {-3.0e9, -1.5}.issubset(set(v.tolist())))


@pytest.mark.parametrize('apply_fill', [False, True])
@pytest.mark.parametrize('B,T,seed', S.DUR)
def test_duration_counts_ref_is_the_oracle(B, T, seed, apply_fill):
    dur = S.dur_tensor(B, T, seed)
    got, off, tot, flag = S.duration_counts_ref(dur, apply_fill)
    d = O.fill_rule(dur) if apply_fill else dur
    assert flag == int(apply_fill and d is not dur)
    x = np.arange(B * T, dtype=np.float32).reshape(B, T, 1)
    y, clipped = O.length_regulator(x, d)
    assert S.same_bits(got, clipped)
    counts = O.duration_counts(d)
    assert np.array_equal(off[:, 0], np.zeros(B)) and np.array_equal(np.diff(off, axis=1), counts)
    assert np.array_equal(tot, counts.sum(axis=1)) and off.dtype == tot.dtype == np.int32
    assert y.shape[1] == tot.max()
    if T >= 8:  # the known answers, in every row
        for b in range(B):
            p = (7 * b) % (T - 3)
            assert counts[b, p:p + 4].tolist() == [1, 2, 3, 0] or flag


@pytest.mark.parametrize('p,neg', S.FILL)
def test_fill_ref_is_the_oracle(p, neg):
    dur = S.fill_tensor(p, neg)
    got, off, tot, flag = S.duration_counts_ref(dur, True)
    want = O.fill_rule(dur)
    assert flag == int(neg) and S.same_bits(got, np.where(want < 0, np.float32(0), want))
    assert S.trunc_sum_ref(dur) == (0 if neg else 1)


@pytest.mark.parametrize('ext', S.EXT_SUMS)
@pytest.mark.parametrize('name', list(S.global_tensors()))
def test_global_ref_follows_ext_sum(name, ext):
    dur = S.global_tensors()[name]
    got, off, tot, flag = S.duration_counts_ref(dur, True, ext_sum=ext)
    assert flag == int(ext <= 0)
    want = np.full_like(dur, 2.0) if ext <= 0 else np.where(dur < 0, np.float32(0), dur)
    assert S.same_bits(got, want)
    assert np.array_equal(np.diff(off, axis=1), O.duration_counts(want))


def test_global_tensors_disagree_with_ext_sum():
    own = {k: S.trunc_sum_ref(v) for k, v in S.global_tensors().items()}
    assert own['dur_3x65'] > 0 and own['own_sum_le_0'] <= 0
    assert np.int64(2 ** 32).astype(np.int32) == 0  # what a 32-bit read of 2^32 sees


@pytest.mark.parametrize('name', list(S.LR))
def test_lr_refs_are_repeat_interleave_and_the_oracle(name):
    counts = S.LR[name]
    B, T = counts.shape
    off = S.exclusive_offsets(counts)
    d, off2, tot, _ = S.duration_counts_ref(counts.astype(np.float32), False)
    assert np.array_equal(off, off2)  # host offsets are what duration_counts gives
    rows = [torch.repeat_interleave(torch.arange(T), torch.from_numpy(counts[b])) for b in range(B)]
    full = torch.nn.utils.rnn.pad_sequence(rows, batch_first=True, padding_value=-1).numpy()
    x = np.random.Generator(np.random.PCG64(5)).normal(0, 1, (B, T, 4)).astype(np.float32)
    y, _ = O.length_regulator(x, counts.astype(np.float32))
    tmels = S.lr_tmels(counts)
    assert tmels[-1] == 0 and 1 in tmels and tmels[0] == tot.max() + 5
    for T_mel in tmels:
        idx = S.lr_index_ref(off, T_mel)
        want = np.full((B, T_mel), -1, np.int64)
        n = min(T_mel, full.shape[1])
        want[:, :n] = full[:, :n]
        assert idx.dtype == np.int32 and np.array_equal(idx, want)
        if T_mel == tot.max():
            assert S.same_bits(S.length_regulate_ref(x, idx), y)


@pytest.mark.parametrize('case', S.EXPAND_LRPE, ids=lambda c: c[0])
def test_lr_posenc_ref_is_torch(case):
    name, B, T, T_mel, C, stride, seed = case
    x, index, pe = S.expand_inputs(B, T, T_mel, C, seed)
    xt, it = torch.from_numpy(x), torch.from_numpy(index).long()
    g = torch.gather(xt, 1, it.clamp(min=0)[..., None].expand(B, T_mel, C)) * (it >= 0)[..., None]
    want = g + torch.tensor(S.PE_SCALE) * torch.from_numpy(pe[:T_mel])
    assert S.same_bits(S.lr_posenc_ref(x, index, pe, S.PE_SCALE), want.numpy())
    assert S.same_bits(S.length_regulate_ref(x, index), g.numpy() + np.float32(0))


@pytest.mark.parametrize('case', S.EXPAND_EMBPE, ids=lambda c: c[0])
def test_embedding_posenc_ref_is_torch(case):
    name, B, T, rows, dim, seed = case
    ids, table, pe = S.embpe_inputs(B, T, rows, dim, seed)
    ok = (ids >= 0) & (ids < rows)
    e = F.embedding(torch.from_numpy(np.where(ok, ids, 0)), torch.from_numpy(table)) * torch.from_numpy(ok)[..., None]
    want = e + torch.tensor(S.PE_SCALE) * torch.from_numpy(pe[:T])
    got, outside = S.embedding_posenc_ref(ids, table, pe, S.PE_SCALE)
    assert outside and S.same_bits(got, want.numpy())
    assert set(S.outside_ids(rows)) <= set(ids.reshape(-1).tolist())


@pytest.mark.parametrize('name', list(S.SPA))
def test_series_proj_add_ref_is_conv1d(name):
    B, T, C, stride, x_off, wp_off, vec, seed = S.SPA[name]
    x, p, e, wp, bp, we, be = S.spa_inputs(B, T, C, seed)
    ps, es = S.STRENGTHS

    def proj(s, w, b):
        y = F.conv1d(torch.from_numpy(s).double()[:, None], torch.from_numpy(w).double()[:, None],
                     torch.from_numpy(b).double(), padding=1)
        return y.transpose(1, 2).numpy()
    want = x.astype(np.float64) + ps * proj(p, wp, bp) + es * proj(e, we, be)
    got = S.series_proj_add_ref(x, p, wp, bp, ps, e, we, be, es)
    assert got.dtype == np.float64 and np.abs(got - want).max() < 1e-12
    if B > 1:
        assert abs(p[0, -1]) == 8 and abs(p[1, 0]) == 8 and abs(e[0, -1]) == 8 and abs(e[1, 0]) == 8


@pytest.mark.parametrize('C', S.ROWDOT_C)
def test_rowdot_ref_is_linear(C):
    for M in S.ROWDOT_M:
        x, w = S.rowdot_inputs(C, M)
        for bias in (S.ROWDOT_BIAS, None):
            for alpha in S.ROWDOT_ALPHA:
                b = None if bias is None else torch.tensor([float(bias)], dtype=torch.float64)
                want = F.linear(torch.from_numpy(x).double(), torch.from_numpy(w).double()[None], b)[:, 0] / alpha
                got = S.rowdot_ref(x, w, bias, alpha)
                assert got.shape == (M,) and np.abs(got - want.numpy()).max() < 1e-12


# --- every table reaches the branch it names --------------------------------------------------

def test_embed_table_shapes():
    d4 = [dim // 4 for _, dim, _, _ in S.EMBED]
    assert 1 in d4 and any(d & (d - 1) for d in d4)  # one float4; a dim4 that is no power of two
    assert any((int(np.prod(shape)) * (dim // 4)) % 256 for _, dim, shape, _ in S.EMBED)
    assert all(dim % 4 == 0 for _, dim, _, _ in S.EMBED)


def test_dur_and_fill_table_shapes():
    Ts = [T for _, T, _ in S.DUR]
    assert {1, 63, 64, 65}.issubset(Ts) and max(Ts) > 128  # one, two and three scan chunks
    assert max(B for B, _, _ in S.DUR) > 16  # a wave's second row
    n = S.FILL_SHAPE[0] * S.FILL_SHAPE[1]
    assert n > 2 * 1024 and S.FILL_SHAPE[0] > 16
    flags = [S.duration_counts_ref(S.fill_tensor(p, neg), True)[3] for p, neg in S.FILL]
    assert len(S.FILL) == 8 and sum(flags) == 4
    # thread 0, the last lane of wave 15, the second pass, the last element (third pass)
    assert [p for p, neg in S.FILL if neg] == [0, 1023, 1024, n - 1]
    for p, neg in S.FILL:
        v = S.fill_tensor(p, neg).reshape(-1)
        rest = np.delete(v, [p, (p + n // 2) % n] if neg else [p])
        assert np.abs(rest).max() < 0.99 and v[p] == 1.25
    assert sorted(c[0] for c in S.TRUNC) == [1, 1023, 1025, 2600]


def test_lr_table_shapes():
    c = S.LR['zero_runs'][0]
    assert c[0] == 0 and c[1] == 0 and c[-1] == 0 and c[-2] == 0 and c[3] == 0
    assert S.LR['t1'].shape == (1, 1)
    tot = S.LR['empty_row'].sum(axis=1)
    assert tot[0] == 0 and tot[1] > 0
    assert S.LR['t300'].shape[1] == 300 and S.LR['t300'].max() == 4 and S.LR['t300'].min() == 0
    assert S.lr_tmels(S.LR['t300'])[1] > 512  # the largest total takes three index blocks
    for counts in S.LR.values():
        m = counts.sum(axis=1).max()
        assert set(S.lr_tmels(counts)) == {m + 5, m, max(m - 3, 0), 1, 0}


def test_expand_table_shapes():
    Cs = {c[4] for c in S.EXPAND_LR}
    assert {4, 256, 260, 1024} == Cs and all(c[4] % 4 == 0 and c[5] % 4 == 0 for c in S.EXPAND_LR)
    assert any(c[4] // 4 > 64 for c in S.EXPAND_LR)  # the lane loop
    for C in (4, 256, 260):
        assert {c[5] for c in S.EXPAND_LR if c[4] == C} == {C, C + 4}
    assert {c[5] for c in S.EXPAND_LRPE if c[4] == 6} == {6, 10}
    assert all((c[1] * c[3]) % 4 for c in S.EXPAND_LR if c[0] != 'grid')
    grid = S.EXPAND_LR[-1]
    assert grid[1] * grid[3] * grid[4] > S.GRID_CAP and S.EXPAND_LRPE[-1] == grid
    for name, B, T, T_mel, C, stride, seed in S.EXPAND_LRPE:
        x, index, pe = S.expand_inputs(B, T, T_mel, C, seed)
        assert (index == -1).any() and index.max() < T and index.min() == -1
        assert (index[:, -1] >= 0).any()  # a row that fills (or is cropped at) T_mel
    assert {c[4] for c in S.EXPAND_EMBPE} == {6, 256, 1024}
    g = S.EXPAND_EMBPE[-1]
    assert g[1] * g[2] * g[4] > S.GRID_CAP


def test_spa_table_reaches_both_kernels():
    for name, (B, T, C, stride, x_off, wp_off, vec, seed) in S.SPA.items():
        assert S.spa_vector_path(C, stride, x_off, wp_off) == vec, name
        assert stride >= C
    v = {k: c for k, c in S.SPA.items() if c[6]}
    s = {k: c for k, c in S.SPA.items() if not c[6]}
    assert len(v) == 3 and len(s) == 5
    blocks = {k: -(-(c[2] // 4) // 256) for k, c in v.items()}
    assert blocks == {'v_t1': 1, 'v_2blocks': 2, 'v_partial': 2}
    assert S.SPA['v_partial'][2] % S.SP_BLOCK_COLS and S.SPA['v_partial'][3] > S.SPA['v_partial'][2]
    B, T = S.SPA['v_2blocks'][:2]
    crossed = {r // T for r0 in range(0, B * T, S.SP_ROWS)
               for r in (r0, min(r0 + S.SP_ROWS, B * T) - 1)
               if r0 // T != (min(r0 + S.SP_ROWS, B * T) - 1) // T}
    assert crossed == {0, 1, 2}  # a chunk spans items 0 | 1, another items 1 | 2
    # the scalar reasons, one each: C % 4, C % 4 beyond 256 threads, the stride, x's address, wp's
    assert s['s_c6'][2] % 4 and s['s_c514'][2] % 4 and s['s_c514'][2] > 256
    assert s['s_stride'][2] % 4 == 0 and s['s_stride'][3] % 4
    assert s['s_addr'][4] == 1 and s['s_wp_addr'][5] == 1
    assert S.SPA['v_t1'][:3] == (1, 1, 4)


def test_rowdot_table():
    assert min(S.ROWDOT_C) < 64 and any(c % 64 for c in S.ROWDOT_C if c > 64) and 64 in S.ROWDOT_C
    assert all(B * T == M for M, (B, T) in S.ROWDOT_M.items())
    assert any(M % 4 for M in S.ROWDOT_M) and 4 in S.ROWDOT_M  # partial and full workgroups of 4 rows


# --- guarded buffers --------------------------------------------------------------------------

def test_guarded_layout():
    v = np.arange(24, dtype=np.float32).reshape(2, 3, 4)
    buf, span = S.guarded(v, stride=6, offset=1)
    assert buf.size == 2 * S.GUARD + 1 + 6 * 6 and span.start == S.GUARD + 1
    assert S.same_bits(S.operand(buf, span, (2, 3, 4), 6), v)
    assert (buf == S.SENTINEL).sum() == buf.size - v.size
    t = torch.from_numpy(buf)
    assert torch.equal(S.operand(t, span, (2, 3, 4), 6), torch.from_numpy(v))
    assert S.operand(t, span, (2, 3, 4), 6).data_ptr() == t.data_ptr() + 4 * span.start
    other = buf.copy()
    other[span.start + 4] = 0  # a write into the stride gap
    assert not S.same_bits(buf, other)
    assert not S.same_bits(np.float32([0.0]), np.float32([-0.0]))
    ibuf, _ = S.guarded(np.zeros((2, 3), np.int32))
    assert ibuf[0] == S.INT_SENTINEL and ibuf.dtype == np.int32


# --- planted defects ----------------------------------------------------------------------------

def _dur(args, **kw):
    return lambda d: S.duration_counts_ref(*args, defect=d, **kw)


def _embed(i, which):
    rows, dim, shape, seed = S.EMBED[i]
    return lambda d: S.embedding_ref(S.embed_id_sets(rows, shape, seed)[which], S.embed_table(rows, dim, seed), d)


def _lr_index(name, T_mel):
    return lambda d: S.lr_index_ref(S.exclusive_offsets(S.LR[name]), T_mel, d)


def _expand(table, name, fn):
    _, B, T, T_mel, C, stride, seed = next(c for c in table if c[0] == name)
    x, index, pe = S.expand_inputs(B, T, T_mel, C, seed)
    if fn is S.length_regulate_ref:
        return lambda d: fn(x, index, d)
    return lambda d: fn(x, index, pe, S.PE_SCALE, d)


def _embpe(name):
    _, B, T, rows, dim, seed = next(c for c in S.EXPAND_EMBPE if c[0] == name)
    ids, table, pe = S.embpe_inputs(B, T, rows, dim, seed)
    return lambda d: S.embedding_posenc_ref(ids, table, pe, S.PE_SCALE, d)


def _spa(name):
    B, T, C, stride, x_off, wp_off, vec, seed = S.SPA[name]
    x, p, e, wp, bp, we, be = S.spa_inputs(B, T, C, seed)
    return lambda d: S.series_proj_add_ref(x, p, wp, bp, S.STRENGTHS[0], e, we, be, S.STRENGTHS[1], d)


def _rowdot(C, M, bias, alpha):
    x, w = S.rowdot_inputs(C, M)
    return lambda d: S.rowdot_ref(x, w, bias, alpha, d)


# (defect, the case that catches it, comparison, restatement of that case)
PLANTED = [
    ('fill_lt0', 'FILL p=0 with -1.5', 'bits', _dur((S.fill_tensor(0, True), True))),
    ('floor', 'TRUNC n=1023', 'bits', lambda d: S.trunc_sum_ref(S.trunc_tensor(1023, 52), d)),
    ('floor', 'FILL p=1023 without -1.5', 'bits', _dur((S.fill_tensor(1023, False), True))),
    ('round', 'TRUNC n=1023', 'bits', lambda d: S.trunc_sum_ref(S.trunc_tensor(1023, 52), d)),
    ('first1024', 'TRUNC n=1025', 'bits', lambda d: S.trunc_sum_ref(S.trunc_tensor(1025, 53), d)),
    ('first1024', 'FILL p=1024 without -1.5', 'bits', _dur((S.fill_tensor(1024, False), True))),
    ('first1024', 'FILL p=2599 without -1.5', 'bits', _dur((S.fill_tensor(2599, False), True))),
    ('first1024', 'FILL p=0 with -1.5', 'bits', _dur((S.fill_tensor(0, True), True))),
    ('ext32', 'GLOBAL dur_3x65 ext_sum=2^32', 'bits',
     _dur((S.global_tensors()['dur_3x65'], True), ext_sum=2 ** 32)),
    ('own_sum', 'GLOBAL dur_3x65 ext_sum=-3', 'bits',
     _dur((S.global_tensors()['dur_3x65'], True), ext_sum=-3)),
    ('own_sum', 'GLOBAL own_sum_le_0 ext_sum=1', 'bits',
     _dur((S.global_tensors()['own_sum_le_0'], True), ext_sum=1)),
    ('inclusive_scan', 'DUR (1, 63)', 'bits', _dur((S.dur_tensor(1, 63, 22), False))),
    ('carry64', 'DUR (3, 65)', 'bits', _dur((S.dur_tensor(3, 65, 24), False))),
    ('carry64', 'DUR (20, 130)', 'bits', _dur((S.dur_tensor(20, 130, 26), True))),
    ('first_equal', 'LR zero_runs T_mel=5', 'bits', _lr_index('zero_runs', 5)),
    ('first_equal', 'LR empty_row T_mel=3', 'bits', _lr_index('empty_row', 3)),
    ('minus1_row0', 'EXPAND length_regulate C4_s4', 'bits', _expand(S.EXPAND_LR, 'C4_s4', S.length_regulate_ref)),
    ('minus1_row0', 'EXPAND lr_posenc C6_s6', 'bits', _expand(S.EXPAND_LRPE, 'C6_s6', S.lr_posenc_ref)),
    ('minus1_row0', 'EMBED (135, 64) planted', 'bits', _embed(1, 'planted')),
    ('minus1_row0', 'EMBED (135, 4) id=-1', 'bits', _embed(0, 'id=-1')),
    ('clamp', 'EMBED (135, 64) planted', 'bits', _embed(1, 'planted')),
    ('clamp', 'EXPAND embedding_posenc d6', 'bits', _embpe('d6')),
    ('wrap32', 'EMBED (7, 260) planted', 'bits', _embed(2, 'planted')),
    ('wrap32', f'EMBED (135, 4) id={2 ** 32 + 1}', 'bits', _embed(0, f'id={2 ** 32 + 1}')),
    ('wrap32', 'EXPAND embedding_posenc d256', 'bits', _embpe('d256')),
    ('cross_item', 'SPA s_c6', 'close', _spa('s_c6')),
    ('cross_item', 'SPA v_2blocks', 'close', _spa('v_2blocks')),
    ('block0_weights', 'SPA v_partial', 'close', _spa('v_partial')),
    ('block0_weights', 'SPA v_2blocks', 'close', _spa('v_2blocks')),
    ('bias_after_div', 'ROWDOT C=63 M=3 alpha=1.3', 'close', _rowdot(63, 3, S.ROWDOT_BIAS, 1.3)),
    ('bias_after_div', 'ROWDOT C=200 M=38 alpha=1000', 'close', _rowdot(200, 38, S.ROWDOT_BIAS, 1000.0)),
    ('flat_row', 'EXPAND lr_posenc C6_s6', 'bits', _expand(S.EXPAND_LRPE, 'C6_s6', S.lr_posenc_ref)),
    ('flat_row', 'EXPAND embedding_posenc d6', 'bits', _embpe('d6')),
]


def _parts(out):
    return [np.asarray(o) for o in out] if isinstance(out, tuple) else [np.asarray(out)]


def test_every_defect_is_planted():
    assert {p[0] for p in PLANTED} == set(S.DEFECTS)


@pytest.mark.parametrize('defect,case,how,fn', PLANTED, ids=[f'{p[0]}@{p[1]}' for p in PLANTED])
def test_comparison_rejects_planted_defect(defect, case, how, fn):
    good, bad = _parts(fn(None)), _parts(fn(defect))
    again = _parts(fn(None))
    if how == 'bits':
        assert all(S.same_bits(a, b) for a, b in zip(good, again))
        rejected = not all(S.same_bits(a, b) for a, b in zip(good, bad))
        print(f'    {defect} ({S.DEFECTS[defect]}): rejected by {case}, bit comparison')
    else:
        ratio = S.bound_ratio(bad[0], good[0], RTOL, ATOL)
        assert S.bound_ratio(good[0].astype(np.float32), good[0], RTOL, ATOL) < 0.1  # fp32 itself passes
        rejected = ratio > 1.0
        print(f'    {defect} ({S.DEFECTS[defect]}): rejected by {case}, |err| / bound = {ratio:.3g}')
    assert rejected


def test_bound_ratio_is_close():
    """bound_ratio <= 1 exactly where tests/test_gpu_kernels.close passes."""
    from test_gpu_kernels import close
    ref = np.array([0.0, 1.0, -300.0, 5.0])
    scale = max(1.0, float(np.sqrt(np.mean(ref ** 2))))
    inside = ref + 0.99 * (ATOL * scale + RTOL * np.abs(ref))
    outside = ref + 1.01 * (ATOL * scale + RTOL * np.abs(ref)) * np.array([0, 0, 1, 0])
    close(inside, ref)
    assert S.bound_ratio(inside, ref, RTOL, ATOL) <= 1.0 < S.bound_ratio(outside, ref, RTOL, ATOL)
    with pytest.raises(AssertionError):
        close(outside, ref)
