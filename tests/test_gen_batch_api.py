"""generate_batch / generate_masked without a GPU: the chunk plan, the argument checks (each
error names its argument) and the new entry points' host-side checks, which return before
any launch."""
import ctypes

import pytest
import torch

from forwardtacotron_amd import _lib
from forwardtacotron_amd.forward_tacotron import ForwardTacotron, batch_plan


def test_plan_sorts_chunks_and_inverts():
    lengths = [40, 39, 37, 33, 9, 2, 40]
    chunks, inverse = batch_plan(lengths, max_batch=3)
    assert [len(c) for c in chunks] == [3, 3, 1]
    flat = [i for c in chunks for i in c]
    assert sorted(flat) == list(range(7))
    # sorted by length, longest first, ties in input order
    assert flat == [0, 6, 1, 2, 3, 4, 5]
    assert [lengths[i] for i in flat] == sorted(lengths, reverse=True)
    assert [flat[inverse[i]] for i in range(7)] == list(range(7))


@pytest.mark.parametrize('n,max_batch', [(1, 1), (5, 1), (5, 2), (5, 5), (5, 64), (17, 4)])
def test_plan_chunk_sizes(n, max_batch):
    lengths = [(7 * i) % 11 + 1 for i in range(n)]
    chunks, inverse = batch_plan(lengths, max_batch)
    assert all(1 <= len(c) <= max_batch for c in chunks)
    assert len(chunks) == -(-n // max_batch)
    flat = [i for c in chunks for i in c]
    assert sorted(flat) == list(range(n))
    assert [flat[p] for p in inverse] == list(range(n))
    ls = [lengths[i] for i in flat]
    assert ls == sorted(ls, reverse=True)


def test_plan_without_max_batch_is_one_chunk_in_input_order():
    chunks, inverse = batch_plan([3, 9, 1, 9], None)
    assert chunks == [[0, 1, 2, 3]] and inverse == [0, 1, 2, 3]


def test_plan_errors():
    with pytest.raises(ValueError, match='xs'):
        batch_plan([], 4)
    with pytest.raises(ValueError, match='max_batch'):
        batch_plan([3, 4], 0)


@pytest.fixture(scope='module')
def cpu_model():
    from forwardtacotron_amd.synthetic import default_config
    return ForwardTacotron.from_config(default_config()).eval()


def test_generate_batch_argument_errors(cpu_model):
    with pytest.raises(ValueError, match='xs'):
        cpu_model.generate_batch([])
    with pytest.raises(ValueError, match=r'xs\[1\]'):
        cpu_model.generate_batch([[1, 2, 3], []])
    with pytest.raises(ValueError, match=r'xs\[0\]'):
        cpu_model.generate_batch([torch.zeros(2, 3, dtype=torch.long)])
    with pytest.raises(ValueError, match=r'xs\[0\]'):
        cpu_model.generate_batch([[0.5, 1.5]])
    with pytest.raises(ValueError, match='xs'):
        cpu_model.generate_batch(torch.zeros(2, 3, dtype=torch.long))
    with pytest.raises(ValueError, match='max_batch'):
        cpu_model.generate_batch([[1, 2, 3]], max_batch=0)
    with pytest.raises(RuntimeError, match='HIP device'):  # a model that was never moved
        cpu_model.generate_batch([[1, 2, 3]])


def test_generate_masked_argument_errors(cpu_model):
    x = torch.ones(2, 5, dtype=torch.long)
    for bad in ([0, 5], [1, 6], [-1, 3]):
        with pytest.raises(ValueError, match='x_len'):
            cpu_model.generate_masked(x, torch.tensor(bad))
    with pytest.raises(ValueError, match='x_len'):  # one length for two rows
        cpu_model.generate_masked(x, torch.tensor([5]))
    with pytest.raises(ValueError, match='x_len'):
        cpu_model.generate_masked(x, torch.tensor([[5, 5]]))
    with pytest.raises(ValueError, match='x_len'):
        cpu_model.generate_masked(x, torch.tensor([2.0, 3.0]))
    with pytest.raises(ValueError, match=r'\bx\b'):
        cpu_model.generate_masked(torch.ones(5, dtype=torch.long), [5])
    with pytest.raises(RuntimeError, match=r'^x: .*CPU tensor'):
        cpu_model.generate_masked(x, [5, 3])


P = ctypes.c_void_p


@pytest.mark.parametrize('call,code', [
    (lambda L: L.ftmi_fill_tail(None, 4, 1, 4, 4, None, 1, 0.0, 0, None), 1001),
    (lambda L: L.ftmi_fill_tail(P(256), 4, 1, 4, 4, None, 1, 0.0, 0, None), 1001),
    (lambda L: L.ftmi_fill_tail(None, 4, 1, 4, 4, P(256), 1, 0.0, 0, None), 1001),
    (lambda L: L.ftmi_fill_tail(P(256), 4, 0, 4, 4, P(256), 1, 0.0, 0, None), 1001),
    (lambda L: L.ftmi_fill_tail(P(256), 4, 1, 4, 4, P(256), 1, 0.0, 3, None), 1001),  # mode
    (lambda L: L.ftmi_fill_tail(P(256), 3, 1, 4, 4, P(256), 1, 0.0, 0, None), 1002),  # stride < C
    (lambda L: L.ftmi_fill_tail(P(256), 3, 1, 4, 2, P(256), 1, 0.0, 1, None), 1002),  # stride < T
    (lambda L: L.ftmi_fill_tail(P(256), 8, 1, 4, 5, P(256), 1, 0.0, 2, None), 1002),  # split, odd C
    (lambda L: L.ftmi_fill_tail(P(256), 4, 1, 4, 4, P(256), 0, 0.0, 0, None), 0),     # reach 0
    (lambda L: L.ftmi_maxpool_rows(None, 4, 1, 4, 4, None, None, 4, None), 1001),
    (lambda L: L.ftmi_maxpool_rows(P(256), 4, 1, 4, 4, P(256), None, 4, None), 1001),
    (lambda L: L.ftmi_maxpool_rows(P(256), 2, 1, 4, 4, P(256), P(512), 4, None), 1002),
    (lambda L: L.ftmi_maxpool_rows(P(256), 6, 1, 4, 6, P(256), P(512), 6, None), 1004),
    (lambda L: L.ftmi_maxpool_rows(P(260), 4, 1, 4, 4, P(256), P(512), 4, None), 1004),
    (lambda L: L.ftmi_duration_counts_rows(None, 1, 1, None, 1, 2.0, None, None, None, None), 1001),
    (lambda L: L.ftmi_duration_counts_rows(P(256), 1, 1, None, 1, 2.0, P(256), P(256), None, None), 1001),
    (lambda L: L.ftmi_duration_counts_rows(P(256), 1, 0, P(256), 1, 2.0, P(256), P(256), None, None), 1001),
])
def test_new_entry_points_check_arguments(call, code):
    assert call(_lib.load()) == code
