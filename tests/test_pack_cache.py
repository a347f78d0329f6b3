"""The host's pack cache (common_layers.weights_key / cached_pack / held_packs) on CPU
tensors with stub builders: what it is keyed on, when it rebuilds, what it holds."""
import pytest
import torch
import torch.nn as nn

from forwardtacotron_amd import common_layers
from forwardtacotron_amd.common_layers import (HighwayNetwork, LinearParams, Packed,
                                               cached_pack, held_packs, weights_key)


class Counting:
    """A builder that counts its calls and returns a fresh object each time."""

    def __init__(self):
        self.n = 0

    def __call__(self):
        self.n += 1
        assert not torch.is_grad_enabled()  # builders run under no_grad
        return [self.n]


@pytest.fixture
def stub_presplit(monkeypatch):
    """LinearParams packs without the device-side split of its weight."""
    monkeypatch.setattr(common_layers, 'presplit', lambda w: None)


def _net():
    return nn.Sequential(LinearParams(4, 3), nn.Sequential(LinearParams(3, 2, bias=False)))


def _parent_pack_key(self):
    """Packed._pack_key as it stood before weights_key, restated."""
    refs = self.__dict__.get('_test_refs')
    if refs is None or any(d.get(n) is not t for d, n, t in refs):
        refs = [(d, n, t) for m in self.modules() for d in (m._parameters, m._buffers)
                for n, t in d.items() if t is not None]
        self.__dict__['_test_refs'] = refs
    return tuple((t.data_ptr(), t._version) for _, _, t in refs)


def test_unchanged_key_builds_nothing():
    net, build = _net(), Counting()
    first = cached_pack(net, '_slot', build)
    assert cached_pack(net, '_slot', build) is first and build.n == 1
    assert cached_pack(net, '_slot', build, extra=None) is first and build.n == 1


def test_each_change_rebuilds_once():
    net, build = _net(), Counting()
    get = lambda extra=None: cached_pack(net, '_slot', build, extra)  # noqa: E731
    get()
    with torch.no_grad():  # in place
        net[1][0].weight.mul_(2.0)
    assert get() == [2] and get() == [2]
    net.load_state_dict({k: torch.randn_like(v) for k, v in net.state_dict().items()})
    assert get() == [3] and get() == [3]
    net[1][0].weight = nn.Parameter(net[1][0].weight.detach().clone())  # replaced in a submodule
    assert get() == [4] and get() == [4]
    assert get(extra=(1, 'a')) == [5] and get(extra=(1, 'a')) == [5]  # a changed extra key part
    assert get(extra=(2, 'a')) == [6] and get(extra=(2, 'a')) == [6]
    assert build.n == 6


def test_weights_key_is_the_parents_pack_key():
    hw = HighwayNetwork(32)
    hw.register_buffer('stat', torch.zeros(3))
    assert weights_key(hw) == _parent_pack_key(hw) == hw._pack_key()
    assert len(weights_key(hw)) == 5
    with torch.no_grad():
        hw.W2.bias.add_(1.0)
    hw.W1.weight = nn.Parameter(torch.zeros(32, 32))
    assert weights_key(hw) == _parent_pack_key(hw) == hw._pack_key()
    net = _net()
    assert weights_key(net) == _parent_pack_key(net)


def test_packed_modules_go_through_the_cache(stub_presplit):
    class Twice(Packed):
        def __init__(self):
            super().__init__()
            self.lin = LinearParams(4, 4)
            self.packs = 0

        def _pack(self):
            self.packs += 1
            return (self.lin.weight.detach() * 2,)

    m = Twice()
    assert m.packed_weights() is m.packed_weights() and m.packs == 1
    w, b, w3 = m.lin.packed_weights()
    assert w.data_ptr() == m.lin.weight.data_ptr() and b.data_ptr() == m.lin.bias.data_ptr()
    with torch.no_grad():
        m.lin.bias.zero_()
    assert torch.equal(m.packed_weights()[0], m.lin.weight * 2) and m.packs == 2


def test_held_packs_finds_every_slot(stub_presplit):
    net = _net()
    assert held_packs(net) == []
    a = cached_pack(net, '_slot_a', Counting())
    b = cached_pack(net[0], '_slot_b', Counting())
    c = cached_pack(net[1][0], '_slot_c', Counting(), extra=7)
    p = net[1][0].packed_weights()
    held = held_packs(net)
    assert len(held) == 4 and all(any(h is v for h in held) for v in (a, b, c, p))
    c2 = cached_pack(net[1][0], '_slot_c', Counting(), extra=8)  # rebuilt: the new value only
    held = held_packs(net)
    assert len(held) == 4 and any(h is c2 for h in held) and not any(h is c for h in held)
    assert held_packs(net[0]) == [b]
    assert held_packs(_net()) == []
