"""The sequence-side kernels (csrc/seq.hip above the length-aware batches, and the two
positional-encoding kernels of csrc/transformer.hip) against the restatements of
tests/seq_cases.py, on its case tables: the smallest shapes that reach every branch.

Integer and byte-moving kernels (embedding, the duration kernels, lr_index, length_regulate,
both posenc kernels) are compared bit for bit; operands and, where the caller chooses it, the
output sit inside sentinel-guarded buffers that are compared whole.  series_proj_add and rowdot
are held to the float64 restatement under tests/test_gpu_kernels.close at that file's RTOL /
ATOL, in place on a guarded buffer whose stride gap, guards and lead-in stay bit-unchanged."""
import numpy as np
import pytest
import torch

import seq_cases as S
from forwardtacotron_amd import _lib, ops
from test_gpu_kernels import ATOL, RTOL, close

pytestmark = pytest.mark.gpu

E_SHAPE, E_ALIGN = 1002, 1004  # include/ftmi.h FTMI_E_SHAPE, FTMI_E_ALIGN


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


class Put:
    """`values` on the device inside a guarded buffer (seq_cases.guarded): .view is the operand,
    .buf the whole buffer, .host the buffer as it was uploaded."""

    def __init__(self, values, stride=None, offset=0):
        values = np.asarray(values)
        self.shape, self.C = values.shape, values.shape[-1]
        self.stride = self.C if stride is None else stride
        self.host, self.span = S.guarded(values, self.stride, offset)
        self.buf = dev(self.host)
        self.view = S.operand(self.buf, self.span, self.shape, self.stride)
        assert self.view.data_ptr() == self.buf.data_ptr() + self.span.start * self.buf.element_size()

    def operand(self):
        """The operand as the device holds it now."""
        return S.operand(host(self.buf), self.span, self.shape, self.stride).copy()

    def unchanged(self):
        return S.same_bits(host(self.buf), self.host)

    def holds(self, values):
        """Every element of the buffer: `values` in the operand, the uploaded bits elsewhere."""
        want = self.host.copy()
        want[self.span].reshape(-1, self.stride)[:, :self.C] = np.asarray(values).reshape(-1, self.C)
        return S.same_bits(host(self.buf), want)


def blank(shape, stride=None, offset=0, dtype=np.float32):
    """A guarded output that holds the sentinel itself: an element a kernel skips shows."""
    return Put(np.full(shape, S.sentinel_of(dtype), dtype), stride, offset)


# ---------------------------------------------------------------- embedding
@pytest.mark.parametrize('with_err', [True, False], ids=['err', 'no_err'])
@pytest.mark.parametrize('rows,dim,shape,seed', S.EMBED)
def test_embedding(rows, dim, shape, seed, with_err):
    """In-table ids gather their rows, every other id (-1, rows, 2^32, 2^32 + 1, -2^40) gives a
    zero row.  The err word becomes 1 exactly with the first id outside the table and is not
    cleared by the clean call that follows; err=None (generate_masked's PAD_ID) runs clean."""
    L = _lib.load()
    table = S.embed_table(rows, dim, seed)
    tab = Put(table)
    errw = dev(np.array([S.INT_SENTINEL, 0, S.INT_SENTINEL], np.int32))
    err = errw[1:2] if with_err else None
    sets = S.embed_id_sets(rows, shape, seed)
    order = sorted(sets, key=lambda k: not k.startswith('clean')) + ['clean']
    seen_outside = False
    for name in order:
        want, outside = S.embedding_ref(sets[name], table)
        ids = Put(sets[name])
        y = ops.embedding(ids.view, tab.view, err)
        assert S.same_bits(host(y), want), name
        out = blank(want.shape)  # the library directly, into a guarded output
        assert L.ftmi_embedding(ids.view.data_ptr(), ids.view.numel(), tab.view.data_ptr(), rows, dim,
                                out.view.data_ptr(), ops._ptr(err), ops._stream()) == 0
        assert out.holds(want), name
        seen_outside |= outside
        assert host(errw).tolist() == [S.INT_SENTINEL, int(seen_outside and with_err), S.INT_SENTINEL], name
        assert ids.unchanged()
    assert seen_outside and tab.unchanged()


def test_embedding_refusals_launch_nothing():
    """dim % 4 != 0 is the shape status, a table or an output off 16 bytes the alignment status;
    neither launches: the outputs still hold the sentinel."""
    L = _lib.load()
    ids = dev(np.zeros(3, np.int64))
    tab, tab1 = Put(S.embed_table(7, 8, 1)), Put(S.embed_table(7, 8, 1), offset=1)
    out, out1 = blank((3, 8)), blank((3, 8), offset=1)
    assert tab.view.data_ptr() % 16 == 0 and tab1.view.data_ptr() % 16 == 4
    assert out.view.data_ptr() % 16 == 0 and out1.view.data_ptr() % 16 == 4

    def call(t, dim, o):
        return L.ftmi_embedding(ids.data_ptr(), 3, t.view.data_ptr(), 7, dim, o.view.data_ptr(), None,
                                ops._stream())
    assert call(tab, 6, out) == E_SHAPE
    assert call(tab1, 8, out) == E_ALIGN
    assert call(tab, 8, out1) == E_ALIGN
    assert out.unchanged() and out1.unchanged()
    with pytest.raises(_lib.FtmiError, match=f'status {E_SHAPE}'):
        ops.embedding(ids.view(1, 3), dev(S.embed_table(7, 6, 1)))
    assert call(tab, 8, out) == 0  # the same arguments, aligned and with dim % 4 == 0, run
    assert out.holds(np.tile(S.embed_table(7, 8, 1)[0], (3, 1)))


# ---------------------------------------------------------------- duration kernels
def check_counts(dur, apply_fill, ext_sum=None):
    want_dur, want_off, want_tot, want_flag = S.duration_counts_ref(dur, apply_fill, ext_sum=ext_sum)
    d = Put(dur)
    if ext_sum is None:
        off, tot, flag = ops.duration_counts(d.view, apply_fill)
    else:
        s = dev(np.array([S.INT_SENTINEL, ext_sum, S.INT_SENTINEL], np.int64))
        off, tot, flag = ops.duration_counts_global(d.view, s[1:2])
        assert host(s).tolist() == [S.INT_SENTINEL, ext_sum, S.INT_SENTINEL]
    assert host(flag).tolist() == [want_flag]
    assert d.holds(want_dur)
    assert S.same_bits(host(off), want_off) and S.same_bits(host(tot), want_tot)
    return want_flag


@pytest.mark.parametrize('apply_fill', [False, True], ids=['clip', 'fill'])
@pytest.mark.parametrize('B,T,seed', S.DUR)
def test_duration_counts(B, T, seed, apply_fill):
    """Clip, counts and the exclusive scan across the 64-lane chunks and the 16 waves, with and
    without the fill-2 rule (B > 16 with apply_fill among them)."""
    check_counts(S.dur_tensor(B, T, seed), apply_fill)


@pytest.mark.parametrize('p,neg', S.FILL)
def test_fill_rule_sums_every_element(p, neg):
    """The one 1.25 sits at thread 0, the last thread of wave 15, the second pass, the last
    element: a lost partial or a lost pass flips the decision of one of the eight cases."""
    assert check_counts(S.fill_tensor(p, neg), True) == int(neg)


@pytest.mark.parametrize('ext', S.EXT_SUMS)
@pytest.mark.parametrize('name', list(S.global_tensors()))
def test_duration_counts_global_follows_ext_sum(name, ext):
    """The sharded rule: the decision is ext_sum <= 0 on the whole 64-bit word, whatever the
    tensor's own sum says."""
    assert check_counts(S.global_tensors()[name], True, ext_sum=ext) == int(ext <= 0)


@pytest.mark.parametrize('n,seed', S.TRUNC)
def test_duration_trunc_sum(n, seed):
    v = S.trunc_tensor(n, seed)
    want = S.trunc_sum_ref(v)
    shapes = [(1, n), (n, 1)] + ([(20, 130)] if n == 2600 else [])
    for shape in shapes:
        d = Put(v.reshape(shape))
        out = ops.duration_trunc_sum(d.view)
        assert out.dtype == torch.int64 and host(out).tolist() == [want]
        assert d.unchanged()


def test_duration_trunc_sum_refuses_what_duration_counts_refuses():
    d = dev(S.dur_tensor(3, 65, 24))
    for bad in (d.t(), d[:, ::2], d.double(), d.reshape(-1), d.reshape(3, 5, 13)):
        with pytest.raises(ValueError, match='contiguous'):
            ops.duration_trunc_sum(bad)
        if bad.dim() == 2:
            with pytest.raises(ValueError, match='contiguous'):
                ops.duration_counts(bad, False)
    assert host(ops.duration_trunc_sum(d)).tolist() == [S.trunc_sum_ref(S.dur_tensor(3, 65, 24))]


# ---------------------------------------------------------------- LengthRegulator
@pytest.mark.parametrize('name', list(S.LR))
def test_lr_index(name):
    """Zero-count runs at both ends, T = 1, a row without frames, more than two index blocks;
    T_mel at, beyond and below the largest total, 1, and 0 (an empty map, nothing launched).
    Offsets from the host and from duration_counts alike; the map also into a guarded output."""
    L = _lib.load()
    counts = S.LR[name]
    B, T = counts.shape
    want_off = S.exclusive_offsets(counts)
    off_dev, tot, _ = ops.duration_counts(dev(counts.astype(np.float32)), False)
    assert S.same_bits(host(off_dev), want_off) and host(tot).tolist() == counts.sum(axis=1).tolist()
    off_host = Put(want_off)
    for T_mel in S.lr_tmels(counts):
        want = S.lr_index_ref(want_off, T_mel)
        for off in (off_dev, off_host.view):
            idx = ops.lr_index(off, T_mel)
            assert idx.dtype == torch.int32 and S.same_bits(host(idx), want), T_mel
        if T_mel:
            out = blank((B, T_mel), dtype=np.int32)
            assert L.ftmi_lr_index(off_host.view.data_ptr(), B, T, T_mel, out.view.data_ptr(), ops._stream()) == 0
            assert out.holds(want), T_mel
        else:
            assert L.ftmi_lr_index(off_host.view.data_ptr(), B, T, 0, None, ops._stream()) == 0
    assert off_host.unchanged()


@pytest.mark.parametrize('case', S.EXPAND_LR, ids=lambda c: c[0])
def test_length_regulate(case):
    """C / 4 = 1, 64 and 65 float4 lanes, x contiguous and as a view into wider rows, B * T_mel
    no multiple of the 4 rows of a workgroup; y from the wrapper and, with a row stride of its
    own, inside a guard."""
    name, B, T, T_mel, C, stride, seed = case
    x, index, _ = S.expand_inputs(B, T, T_mel, C, seed)
    want = S.length_regulate_ref(x, index)
    xd, idx = Put(x, stride), Put(index)
    assert S.same_bits(host(ops.length_regulate(xd.view, idx.view)), want)
    y = blank((B, T_mel, C), stride=C + 4)
    assert _lib.load().ftmi_length_regulate(xd.view.data_ptr(), stride, B, T, C, idx.view.data_ptr(), T_mel,
                                            y.view.data_ptr(), C + 4, ops._stream()) == 0
    assert y.holds(want) and xd.unchanged() and idx.unchanged()


@pytest.mark.parametrize('case', S.EXPAND_LRPE, ids=lambda c: c[0])
def test_lr_posenc(case):
    """The same expansion plus scale * pe[t], product and sum each rounded to fp32; widths that
    are no multiple of 4; 'grid' is beyond one pass of the capped grid (the grid-stride loop)."""
    name, B, T, T_mel, C, stride, seed = case
    x, index, pe = S.expand_inputs(B, T, T_mel, C, seed)
    want = S.lr_posenc_ref(x, index, pe, S.PE_SCALE)
    xd, idx, ped = Put(x, stride), Put(index), Put(pe)
    scale = dev(np.array([S.PE_SCALE], np.float32))
    assert S.same_bits(host(ops.lr_posenc(xd.view, idx.view, ped.view, scale)), want)
    y = blank((B, T_mel, C), stride=C + 4)
    assert _lib.load().ftmi_lr_posenc(xd.view.data_ptr(), stride, B, T, C, idx.view.data_ptr(), T_mel,
                                      ped.view.data_ptr(), scale.data_ptr(), y.view.data_ptr(), C + 4,
                                      ops._stream()) == 0
    assert y.holds(want) and xd.unchanged() and idx.unchanged() and ped.unchanged()


@pytest.mark.parametrize('case', S.EXPAND_EMBPE, ids=lambda c: c[0])
def test_embedding_posenc(case):
    """Ids outside the table give 0 + scale * pe[t]; the library's err word reports them."""
    name, B, T, rows, dim, seed = case
    ids, table, pe = S.embpe_inputs(B, T, rows, dim, seed)
    want, outside = S.embedding_posenc_ref(ids, table, pe, S.PE_SCALE)
    idd, tab, ped = Put(ids), Put(table), Put(pe)
    scale = dev(np.array([S.PE_SCALE], np.float32))
    assert S.same_bits(host(ops.embedding_posenc(idd.view, tab.view, ped.view, scale)), want)
    out = blank((B, T, dim))
    errw = dev(np.array([S.INT_SENTINEL, 0, S.INT_SENTINEL], np.int32))
    L = _lib.load()
    args = (B, T, tab.view.data_ptr(), rows, dim, ped.view.data_ptr(), scale.data_ptr(), out.view.data_ptr(),
            errw[1:2].data_ptr(), ops._stream())
    clean = Put(np.where((ids >= 0) & (ids < rows), ids, 0))
    assert L.ftmi_embedding_posenc(clean.view.data_ptr(), *args) == 0
    assert host(errw).tolist() == [S.INT_SENTINEL, 0, S.INT_SENTINEL]
    assert L.ftmi_embedding_posenc(idd.view.data_ptr(), *args) == 0
    assert out.holds(want) and outside
    assert host(errw).tolist() == [S.INT_SENTINEL, 1, S.INT_SENTINEL]
    assert idd.unchanged() and tab.unchanged() and ped.unchanged()


def test_posenc_wrappers_refuse_a_pe_they_would_overrun():
    """Fewer pe rows than T / T_mel, or another width than the operand: a ValueError before any
    launch (only the refusal is run, never the read)."""
    B, T, T_mel, C = 2, 5, 7, 8
    x, index, pe = S.expand_inputs(B, T, T_mel, C, 70)
    ids = dev(np.zeros((B, T), np.int64))
    xd, idx, scale = dev(x), dev(index), dev(np.array([S.PE_SCALE], np.float32))
    table = dev(S.embed_table(9, C, 1))
    for bad in (dev(pe[:T_mel - 1]), dev(pe[:, :C - 4]), dev(np.pad(pe, ((0, 0), (0, 4)))),
                dev(np.pad(pe, ((0, 0), (0, 4))))[:, :C], dev(pe).double(), dev(pe)[:, None, :]):
        with pytest.raises(ValueError, match='pe must be'):
            ops.lr_posenc(xd, idx, bad, scale)
    for bad in (dev(pe[:T - 1]), dev(pe[:, :C - 4]), dev(np.pad(pe, ((0, 0), (0, 4)))), dev(pe).double()):
        with pytest.raises(ValueError, match='pe must be'):
            ops.embedding_posenc(ids, table, bad, scale)
    # exactly enough rows is enough
    assert S.same_bits(host(ops.lr_posenc(xd, idx, dev(pe[:T_mel]), scale)),
                       S.lr_posenc_ref(x, index, pe, S.PE_SCALE))
    assert ops.embedding_posenc(ids, table, dev(pe[:T]), scale).shape == (B, T, C)


# ---------------------------------------------------------------- series_proj_add, rowdot
@pytest.mark.parametrize('name', list(S.SPA))
def test_series_proj_add(name):
    """Both kernels of ftmi_series_proj_add, each by every reason the choice knows: in place on
    a guarded buffer, against float64 under the fp32 parity bar; the stride gap, the guards and
    the one-float lead-in keep their bits."""
    B, T, C, stride, x_off, wp_off, vec, seed = S.SPA[name]
    x, p, e, wp, bp, we, be = S.spa_inputs(B, T, C, seed)
    ps, es = S.STRENGTHS
    ref = S.series_proj_add_ref(x, p, wp, bp, ps, e, we, be, es)
    xd, wpd = Put(x, stride, x_off), Put(wp, offset=wp_off)
    pd, ed, bpd, wed, bed = Put(p), Put(e), Put(bp[None]), Put(we), Put(be[None])
    offs = [(t.view.data_ptr() % 16) // 4 for t in (xd, wpd, wed, bpd, bed)]
    assert offs == [x_off, wp_off, 0, 0, 0] and S.spa_vector_path(C, stride, *offs) == vec
    y = ops.series_proj_add(xd.view, pd.view, wpd.view, bpd.view[0], ps, ed.view, wed.view, bed.view[0], es)
    assert y.data_ptr() == xd.view.data_ptr()
    got = xd.operand()
    ratio = S.bound_ratio(got, ref, RTOL, ATOL)
    print(f'    series_proj_add {name} ({"vector" if vec else "scalar"}): worst |err| / bound = {ratio:.3g}')
    close(got, ref)
    assert xd.holds(got)  # nothing but the operand changed
    assert all(t.unchanged() for t in (wpd, pd, ed, bpd, wed, bed))


@pytest.mark.parametrize('C', S.ROWDOT_C)
def test_rowdot(C):
    """C below, at and beyond the 64 lanes, M across the 4 rows of a workgroup, x contiguous and
    with a row stride of C + 3, with and without the bias, three alphas."""
    worst = 0.0
    for M, (B, T) in S.ROWDOT_M.items():
        x, w = S.rowdot_inputs(C, M)
        wd = Put(w[None])
        for stride in (C, C + 3):
            xd = Put(x.reshape(B, T, C), stride)
            for bias in (S.ROWDOT_BIAS, None):
                bd = None if bias is None else dev(np.array([bias], np.float32))
                for alpha in S.ROWDOT_ALPHA:
                    got = host(ops.rowdot(xd.view, wd.view[0], bd, alpha))
                    ref = S.rowdot_ref(x, w, bias, alpha).reshape(B, T)
                    assert got.shape == (B, T) and got.dtype == np.float32
                    worst = max(worst, S.bound_ratio(got, ref, RTOL, ATOL))
                    close(got, ref)
            assert xd.unchanged() and wd.unchanged()
    print(f'    rowdot C={C}: worst |err| / bound = {worst:.3g}')
