"""The table-gather conv bank (ftmi_embed_bank / ops.embed_bank / CBHG.forward_ids) against
the fp64 numpy oracle: embedding -> Conv1d(pad k//2)[:T] -> ReLU -> BatchNorm(eval) ->
maxpool(2, 1), held to `close` at rtol = atol = 1e-5 (the tightest bank bound of
tests/test_gpu_kernels.py; the table form's own error, fp64 products rounded once and k <= 16
fp32 adds, is ~4e-7).  BN scales take both signs: BN folded in front of the ReLU would show."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import ft_oracle as O
from test_gpu_kernels import close, dev, host

gpu = pytest.mark.gpu

S, K, C = 135, 16, 256  # the prenet bank of the reference config: 135 symbols, k = 1..16, 256 ch
TOL = dict(rtol=1e-5, atol=1e-5)


def _bn(rng, n):
    """BatchNorm1d parameters with weights of both signs, and their fp32 fold."""
    w = rng.uniform(0.5, 1.5, n) * rng.choice([-1.0, 1.0], n)
    b, rm, rv = rng.normal(0, 0.1, n), rng.normal(0, 0.1, n), rng.uniform(0.5, 1.5, n)
    scale = w / np.sqrt(rv + 1e-5)
    return (w, b, rm, rv), scale.astype(np.float32), (b - rm * scale).astype(np.float32)


def _ids(rng, B, T, s=S):
    """Random ids with 0 and s-1 at both ends of every sequence, the edge symbols swapped
    between neighbouring sequences (a tap read across a sequence boundary changes the sum)."""
    ids = rng.integers(0, s, (B, T))
    for b in range(B):
        lo, hi = (0, s - 1) if b % 2 == 0 else (s - 1, 0)
        ids[b, 0], ids[b, -1] = lo, hi
        if T >= 4:
            ids[b, 1], ids[b, -2] = hi, lo
    return ids.astype(np.int64)


def oracle_bank(ids, E, ws, bn, pool):
    """(B, T, len(ws) * Cout) in fp64; ids outside the table take a zero embedding row."""
    Ez = np.concatenate([E.astype(np.float64), np.zeros((1, E.shape[1]))])
    safe = np.where((ids >= 0) & (ids < E.shape[0]), ids, E.shape[0])
    x = O.embedding(safe, Ez).transpose(0, 2, 1)
    T = ids.shape[1]
    y = np.concatenate([np.maximum(O.conv1d(x, w.astype(np.float64), w.shape[2] // 2)[:, :, :T], 0)
                        for w in ws], 1)
    y = O.batchnorm_eval(y, *bn)
    if pool:
        y = O.maxpool_k2_s1_p1(y)
    return y.transpose(0, 2, 1)


def decode_split(y, n):
    """f16x3 split rows (include/ftmi.h) -> values: h + 2^-11 t."""
    h = y.view(np.float16).astype(np.float64)
    return h[..., :n] + h[..., n:] / 2048.0


class Bank:
    """One set of bank weights, its table and folded BN on the device (built once)."""

    def __init__(self, seed, ks, cin, s=S, gain=1.0):
        from forwardtacotron_amd import ops
        rng = np.random.Generator(np.random.PCG64(seed))
        self.ks, self.s = ks, s
        self.E = rng.normal(0, 1, (s, cin)).astype(np.float32)
        self.ws = [(gain * rng.normal(0, 1 / np.sqrt(cin * k), (C, cin, k))).astype(np.float32)
                   for k in ks]
        self.bn, sc, sh = _bn(rng, len(ks) * C)
        self.sc, self.sh = dev(sc), dev(sh)
        self.table = ops.embed_bank_table(dev(self.E), [dev(w) for w in self.ws])

    def run(self, ids, pool=True, split=False):
        from forwardtacotron_amd import ops
        return host(ops.embed_bank(dev(ids), self.table, self.ks[0], self.ks[-1], C, self.sc,
                                   self.sh, pool=pool, split_out=split))

    def ref(self, ids, pool=True):
        return oracle_bank(ids, self.E, self.ws, self.bn, pool)


@pytest.fixture(scope='module')
def bank():
    return Bank(11, list(range(1, K + 1)), 256)


@pytest.fixture(scope='module')
def pred():
    return Bank(12, [5], 64)


@gpu
def test_table_layout(bank):
    """[S][taps][Cout], taps ordered (k = 1..K, j = 0..k-1): Tab[s][(k, j)] = W_k[:, :, j] E[s]."""
    from forwardtacotron_amd import ops
    assert tuple(bank.table.shape) == (S, ops.embed_bank_taps(1, K), C) == (S, 136, C)
    tab = host(bank.table)
    for k, j in ((1, 0), (2, 1), (7, 3), (16, 0), (16, 15)):
        ref = bank.E.astype(np.float64) @ bank.ws[k - 1][:, :, j].astype(np.float64).T
        np.testing.assert_allclose(tab[:, k * (k - 1) // 2 + j], ref, rtol=1e-6, atol=1e-7)


@gpu
@pytest.mark.parametrize('T', [1, 3, 8, 17, 200])
def test_real_bank(bank, T):
    """K = 16, Cin = Cout = 256, S = 135, B = 3: T = 1 (every tap but the centre off the edge),
    T < K/2, T just over K, the workload's T; fp32 rows and split rows; unpooled too."""
    from forwardtacotron_amd import ops
    ids = _ids(np.random.Generator(np.random.PCG64(T)), 3, T)
    ref = bank.ref(ids)
    st = ops.status_word('cuda')
    st.zero_()
    y = bank.run(ids)
    close(y, ref, **TOL)
    ys = bank.run(ids, split=True)
    close(decode_split(ys, K * C), ref, **TOL)
    # the split rows are the fp32 rows split (head = f16(v), tail = f16((v - head) 2^11))
    hd = y.astype(np.float16)
    tl = ((y - hd.astype(np.float32)) * np.float32(2048)).astype(np.float16)
    np.testing.assert_array_equal(ys.view(np.float16), np.concatenate([hd, tl], -1))
    close(bank.run(ids, pool=False), bank.ref(ids, pool=False), **TOL)
    assert int(st.item()) == 0


def _tile_shapes():
    from forwardtacotron_amd import ops
    rows, wg = ops.EMBED_BANK_TILE  # rows per wave, rows per workgroup
    shapes = [(1, n) for t in (rows, wg) for n in (t - 1, t, t + 1)]
    return shapes + [(3, 23), (5, 13), (5, 1), (2, wg + rows // 2)]


@gpu
@pytest.mark.parametrize('B,T', _tile_shapes())
def test_tile_edges(bank, B, T):
    """Rows per wave and per workgroup at tile - 1, tile, tile + 1; B*T not a multiple of
    either tile; sequences that start inside a wave's run; T = 1 with B = 5."""
    ids = _ids(np.random.Generator(np.random.PCG64(100 * B + T)), B, T)
    close(bank.run(ids), bank.ref(ids), **TOL)
    close(decode_split(bank.run(ids, split=True), K * C), bank.ref(ids), **TOL)


@gpu
def test_agrees_with_gemm_bank_through_proj1(bank):
    """conv_bank(embedding(x), pool, split_out) -> proj1 against embed_bank -> proj1, same ids,
    within the 5e-5 bound of test_split_rows_bank_to_proj1."""
    from forwardtacotron_amd import ops
    from forwardtacotron_amd.common_layers import pack_conv
    rng = np.random.Generator(np.random.PCG64(5))
    ids = dev(_ids(rng, 3, 200))
    wp = torch.cat([pack_conv(torch.from_numpy(w)).reshape(-1) for w in bank.ws]).cuda()
    w3 = ops.split_bank_weights(wp, K, 256, C, 2)
    x = ops.embedding(ids, dev(bank.E))
    assert ops.bank_pools(x, K, C, w_split=w3)
    old = ops.conv_bank(x, wp, K, C, bank.sc, bank.sh, mma=2, w_split=w3, pool=True, split_out=True)
    new = ops.embed_bank(ids, bank.table, 1, K, C, bank.sc, bank.sh, pool=True, split_out=True)
    w1 = dev(rng.normal(0, 1 / np.sqrt(3 * K * C), (256, 3 * K * C)).astype(np.float32))
    w13 = ops.split_weights_f16(w1)
    bn = (dev(rng.uniform(0.5, 1.5, 256).astype(np.float32)), dev(rng.normal(0, .1, 256).astype(np.float32)))
    a, _ = ops.conv1d(old, w1, 3, 1, relu=True, bn=bn, mma=2, w_split=w13, x_split=True)
    b, _ = ops.conv1d(new, w1, 3, 1, relu=True, bn=bn, mma=2, w_split=w13, x_split=True)
    close(host(b), host(a), rtol=5e-5, atol=5e-5)


@gpu
def test_range_guard(monkeypatch):
    """Bank weights scaled until a pooled value exceeds 65504: split rows set status bit 0,
    fp32 rows do not, and run_checked reruns CBHG.forward_ids with the bank on fp32 rows."""
    from forwardtacotron_amd import ops
    from forwardtacotron_amd.common_layers import CBHG
    big = Bank(13, list(range(1, K + 1)), 256, gain=3e5)
    ids = _ids(np.random.Generator(np.random.PCG64(6)), 2, 150)
    assert np.abs(big.ref(ids)).max() > 65504
    st = ops.status_word('cuda')
    st.zero_()
    y = big.run(ids)
    assert int(st.item()) == 0
    close(y, big.ref(ids), **TOL)
    big.run(ids, split=True)
    assert int(st.item()) & 1
    st.zero_()

    torch.manual_seed(4)
    m = CBHG(K=K, in_channels=256, channels=C, proj_channels=[256, 256], num_highways=4).cuda()
    with torch.no_grad():
        for conv, w in zip(m.conv1d_bank, big.ws):
            conv.conv.weight.copy_(torch.from_numpy(w))
    emb = dev(big.E)
    modes = []
    real = ops.embed_bank
    monkeypatch.setattr(ops, 'embed_bank', lambda *a, **k: (modes.append(k['split_out']), real(*a, **k))[1])
    with torch.no_grad():
        out = ops.run_checked(lambda: m.forward_ids(dev(ids), emb), emb.device)
        assert modes == [True, False]  # f16x3 pass flagged, exact-path rerun on fp32 rows
        assert int(st.item()) & 1      # the word keeps the bits that caused the rerun
        with ops.exact_paths():
            want = m.forward_ids(dev(ids), emb)
    assert torch.isfinite(out).all()
    np.testing.assert_array_equal(host(out), host(want))
    st.zero_()


@gpu
def test_out_of_range_ids(bank):
    """Ids -1 and S give the rows of a zero embedding row, and nothing outside y is written
    (canary rows on both sides of y)."""
    from forwardtacotron_amd import _lib, ops
    B, T, pad = 2, 37, 4
    ids = _ids(np.random.Generator(np.random.PCG64(7)), B, T)
    ids[0, 0], ids[0, 5], ids[1, T - 1], ids[1, 20] = -1, S, S, -1
    ref = bank.ref(ids)
    for flags, n in ((1, K * C), (3, K * C)):
        buf = torch.full((B * T + 2 * pad, K * C), 12345.0, device='cuda')
        y = buf[pad:pad + B * T]
        _lib.call('ftmi_embed_bank', dev(ids).data_ptr(), B, T, bank.table.data_ptr(), S, 1, K, C,
                  bank.sc.data_ptr(), bank.sh.data_ptr(), y.data_ptr(), K * C, flags,
                  ops.status_word('cuda').data_ptr(), None)
        got = host(buf)
        assert (got[:pad] == 12345.0).all() and (got[pad + B * T:] == 12345.0).all()
        rows = got[pad:pad + B * T].reshape(B, T, K * C)
        close(decode_split(rows, n) if flags & 2 else rows, ref, **TOL)


@gpu
def test_deterministic(bank):
    ids = _ids(np.random.Generator(np.random.PCG64(8)), 3, 200)
    for split in (False, True):
        a, b = bank.run(ids, split=split), bank.run(ids, split=split)
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


@gpu
def test_table_cache():
    """CBHG.embed_bank_table: the same object between two calls with nothing changed; rebuilt
    after an in-place copy_ into the embedding weight, after load_state_dict (of the embedding
    and of the CBHG) and after a bank conv weight changes."""
    from forwardtacotron_amd.common_layers import CBHG
    from forwardtacotron_amd.forward_tacotron import Embedding
    torch.manual_seed(2)
    m = CBHG(K=3, in_channels=32, channels=32, proj_channels=[32, 32], num_highways=1).cuda()
    emb = Embedding(20, 32).cuda()
    t0 = m.embed_bank_table(emb.weight)
    assert m.embed_bank_table(emb.weight) is t0
    assert tuple(t0.shape) == (20, 6, 32)
    with torch.no_grad():
        emb.weight.copy_(torch.randn(20, 32, device='cuda'))
    t1 = m.embed_bank_table(emb.weight)
    assert t1 is not t0 and not torch.equal(t1, t0)
    assert m.embed_bank_table(emb.weight) is t1
    emb.load_state_dict({'weight': torch.randn(20, 32)})
    t2 = m.embed_bank_table(emb.weight)
    assert t2 is not t1 and not torch.equal(t2, t1)
    m.load_state_dict({k: torch.randn_like(v) if v.is_floating_point() else v
                       for k, v in m.state_dict().items()})
    t3 = m.embed_bank_table(emb.weight)
    assert t3 is not t2 and not torch.equal(t3, t2)
    with torch.no_grad():
        m.conv1d_bank[1].conv.weight.mul_(2.0)
    t4 = m.embed_bank_table(emb.weight)
    assert t4 is not t3 and not torch.equal(t4, t3)
    assert m.embed_bank_table(emb.weight) is t4
    ref = torch.einsum('ncj,sc->sjn', m.conv1d_bank[1].conv.weight.double(), emb.weight.double())
    torch.testing.assert_close(t4[:, 1:3], ref.float(), rtol=1e-6, atol=1e-7)


@gpu
def test_forward_ids_matches_forward_cl():
    """CBHG.forward_ids (table bank) against forward_cl(embedding) (GEMM bank) at a row count on
    each side of ops.EMBED_BANK_MIN_ROWS: the same module output within the f16x3 bound."""
    from forwardtacotron_amd import ops
    from forwardtacotron_amd.common_layers import CBHG
    torch.manual_seed(9)
    m = CBHG(K=K, in_channels=256, channels=C, proj_channels=[256, 256], num_highways=4).cuda()
    emb = torch.randn(S, 256, device='cuda')
    rng = np.random.Generator(np.random.PCG64(9))
    with torch.no_grad():
        for B, T in ((3, 200), (1, 120)):
            ids = dev(_ids(rng, B, T))
            for rows in (1, 10 ** 9):
                ops_rows = ops.EMBED_BANK_MIN_ROWS
                ops.EMBED_BANK_MIN_ROWS = rows
                try:
                    got = m.forward_ids(ids, emb)
                finally:
                    ops.EMBED_BANK_MIN_ROWS = ops_rows
                want = m.forward_cl(ops.embedding(ids, emb))
                close(host(got), host(want), rtol=5e-5, atol=5e-5)


@gpu
@pytest.mark.parametrize('Kb,ch,table', [(8, 256, True), (4, 128, False), (3, 64, False)])
def test_forward_ids_other_bank_shapes(Kb, ch, table, monkeypatch):
    """forward_ids on banks other than the 16-kernel one, 2 x 150 = 300 rows (above
    ops.EMBED_BANK_MIN_ROWS): K = 8 at 256 channels takes the table kernel kernel size by
    kernel size and agrees with forward_cl within the f16x3 bound; channel counts the kernel has
    no panel for (ops.embed_bank_ok) keep the GEMM bank — no embed_bank launch, no table, the
    output of forward_cl(embedding) bit for bit."""
    from forwardtacotron_amd import ops
    from forwardtacotron_amd.common_layers import CBHG
    torch.manual_seed(Kb)
    m = CBHG(K=Kb, in_channels=64, channels=ch, proj_channels=[ch, 64], num_highways=2).cuda()
    emb = torch.randn(S, 64, device='cuda')
    ids = dev(_ids(np.random.Generator(np.random.PCG64(Kb)), 2, 150))
    assert ids.numel() >= ops.EMBED_BANK_MIN_ROWS and ops.embed_bank_ok(S, 1, Kb, ch) == table
    calls = []
    real = ops.embed_bank
    monkeypatch.setattr(ops, 'embed_bank', lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    with torch.no_grad():
        got = m.forward_ids(ids, emb)
        want = m.forward_cl(ops.embedding(ids, emb))
    assert len(calls) == int(table) and ('_ftmi_embed_table' in m.__dict__) == table
    if table:
        close(host(got), host(want), rtol=5e-5, atol=5e-5)
    else:
        np.testing.assert_array_equal(host(got), host(want))


@gpu
def test_range_guard_not_a_number():
    """A bank value that is not a number (an overflowed table entry, inf, times a BN scale of
    0; the ReLU itself maps a NaN sum to 0) sets status bit 0 in split rows, pooled (where the
    max drops it from the stored rows) or not, like a value beyond the f16 range; fp32 rows
    leave the word alone and, unpooled, carry the NaN."""
    from forwardtacotron_amd import ops
    nb = Bank(14, [2, 3], 64, s=20)
    ids = _ids(np.random.Generator(np.random.PCG64(3)), 2, 40, s=20)
    ids[1, 17] = 7
    tab, sc = nb.table.clone(), nb.sc.clone()
    tab[7, 1, 33] = float('inf')  # kernel size 2, centre tap, channel 33
    sc[33] = 0.0
    st = ops.status_word('cuda')
    for pool in (True, False):
        for split in (False, True):
            st.zero_()
            y = ops.embed_bank(dev(ids), tab, 2, 3, C, sc, nb.sh, pool=pool, split_out=split)
            torch.cuda.synchronize()
            assert int(st.item()) & 1 == int(split), (pool, split)
            if not split and not pool:
                want = np.zeros(y.shape, bool)  # exactly where symbol 7 sits, channel 33
                want[..., 33] = ids == 7
                np.testing.assert_array_equal(np.isnan(host(y)), want)
    st.zero_()


@gpu
@pytest.mark.parametrize('T', [1, 3, 8, 17, 200])
def test_predictor_form(pred, T):
    """One kernel size (k = 5), Cin = 64, Cout = 256, no pool: a SeriesPredictor's embedding +
    first BatchNormConv, against the oracle's batch_norm_conv on the embedded ids."""
    ids = _ids(np.random.Generator(np.random.PCG64(50 + T)), 3, T)
    w, b, rm, rv = pred.bn
    sd = {'c.conv.weight': pred.ws[0].astype(np.float64), 'c.bnorm.weight': w, 'c.bnorm.bias': b,
          'c.bnorm.running_mean': rm, 'c.bnorm.running_var': rv}
    x = O.embedding(ids, pred.E.astype(np.float64)).transpose(0, 2, 1)
    ref = O.batch_norm_conv(sd, 'c', x, True, np.float64).transpose(0, 2, 1)
    close(pred.run(ids, pool=False), ref, **TOL)


def test_argument_errors():
    """Host-side validation (no launch): null pointers, flags, kernel sizes, Cout, stride,
    alignment, a table of 2 GiB or more."""
    from forwardtacotron_amd import _lib
    L = _lib.load()
    a, mis = ctypes.c_void_p(256), ctypes.c_void_p(260)

    def call(ids=a, B=2, T=8, tab=a, s=S, kmin=1, kmax=K, cout=C, sc=a, sh=a, y=a, ys=K * C, fl=3):
        return L.ftmi_embed_bank(ids, B, T, tab, s, kmin, kmax, cout, sc, sh, y, ys, fl, None, None)
    assert call(ids=None) == 1001 and call(y=None) == 1001 and call(T=0) == 1001
    assert call(kmin=0) == 1001 and call(kmin=5, kmax=4) == 1001 and call(fl=4) == 1001
    assert call(kmax=17) == 1003 and call(cout=128, ys=K * 128) == 1003
    assert call(s=1 << 16) == 1003  # table beyond the 2 GiB a buffer descriptor addresses
    assert call(ys=K * C - 4) == 1002
    # ops.embed_bank_ok mirrors the shapes the entry point refuses as unsupported (kernel sizes,
    # Cout panel, the 2 GiB table: 15,420 symbols fit, 15,421 do not)
    from forwardtacotron_amd import ops
    for s_, kmin, kmax, cout in ((S, 1, K, C), (S, 5, 5, C), (S, 1, 17, C), (S, 1, 20, C), (S, 1, K, 128),
                                 (S, 1, 8, 384), (1 << 16, 1, K, C), (15420, 1, K, C), (15421, 1, K, C)):
        # y misaligned: a supported shape stops at the alignment check, never at a launch
        rc = call(s=s_, kmin=kmin, kmax=kmax, cout=cout, ys=(kmax - kmin + 1) * cout, y=mis)
        assert rc == (1004 if ops.embed_bank_ok(s_, kmin, kmax, cout) else 1003), (s_, kmin, kmax, cout)
    assert call(tab=mis) == 1004 and call(y=mis) == 1004 and call(ys=K * C + 2) == 1004
