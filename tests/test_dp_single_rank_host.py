"""A one-rank process group that counts as data parallel (dtc_amd.distributed.force_data_parallel / DTC_DP_FORCE), on the CPU: gloo,
world_size = 1.  Forced, the helpers issue and record their collectives and return their tensors bit for bit; unforced, or without a
group, nothing is issued and nothing changes."""
import importlib

import pytest
import torch
import torch.distributed as dist

from dtc_amd import distributed as dp


@pytest.fixture
def one_rank_group(tmp_path):
    assert not dist.is_initialized()
    dist.init_process_group("gloo", init_method=f"file://{tmp_path / 'rendezvous'}", rank=0, world_size=1)
    dp.force_data_parallel(False)
    dp.trace_collectives(True)
    try:
        yield
    finally:
        dp.force_data_parallel(False)
        dp.trace_collectives(False)
        dist.destroy_process_group()


def _tensors():
    """a float32 vector with a denormal, a negative zero and an inf in it, and a float64 scalar"""
    vec = torch.tensor([1.5, 1e-42, -0.0, float("inf"), -3.25e-7, 2.0 ** -126], dtype=torch.float32)
    assert 0 < float(vec[1]) < 2.0 ** -126 and torch.signbit(vec[2])
    return vec, torch.tensor(0.1 + 1e-17, dtype=torch.float64)


def _bits(t):
    return t.clone().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def test_forcing_without_a_group_has_no_effect(monkeypatch):
    assert not dist.is_initialized()
    try:
        dp.force_data_parallel(True)
        assert dp.data_parallel() is False
        with dp.force_data_parallel(True):
            assert dp.data_parallel() is False and dp.world_size() == 1 and dp.rank() == 0
        vec, _ = _tensors()
        assert torch.equal(_bits(dp.allreduce_mean_(vec.clone())), _bits(vec))
        assert torch.equal(_bits(dp.allreduce_sum_(vec.clone())), _bits(vec))
        assert torch.equal(_bits(dp.broadcast_parameters_(vec.clone())), _bits(vec))
    finally:
        dp.force_data_parallel(False)
    monkeypatch.setenv("DTC_DP_FORCE", "1")
    try:
        importlib.reload(dp)                              # the switch is read at import, as DTC_DP_TRACE is
        assert dp._FORCE is True and dp.data_parallel() is False
    finally:
        monkeypatch.delenv("DTC_DP_FORCE")
        importlib.reload(dp)
    assert dp._FORCE is False


def test_environment_switch_forces_a_one_rank_group(one_rank_group, monkeypatch):
    monkeypatch.setenv("DTC_DP_FORCE", "1")
    try:
        importlib.reload(dp)
        assert dp.data_parallel() is True
    finally:
        monkeypatch.delenv("DTC_DP_FORCE")
        importlib.reload(dp)
    assert dp.data_parallel() is False


def test_unforced_one_rank_group_issues_nothing(one_rank_group):
    assert dp.world_size() == 1 and dp.data_parallel() is False
    for t in _tensors():
        for fn in (dp.allreduce_mean_, dp.allreduce_sum_, dp.broadcast_parameters_):
            got = t.clone()
            assert fn(got) is got and torch.equal(_bits(got), _bits(t))
    assert dp.collective_log() == [] and dp.assert_same_collective_sequence() == []


def test_forced_one_rank_group_issues_and_records_every_collective(one_rank_group):
    dp.force_data_parallel(True)
    assert dp.data_parallel() is True and dp.world_size() == 1 and dp.rank() == 0
    expected = []
    for t in _tensors():
        name = str(t.dtype).replace("torch.", "")
        for fn, op in ((dp.allreduce_mean_, "all_reduce_mean"), (dp.allreduce_sum_, "all_reduce_sum"), (dp.broadcast_parameters_, "broadcast")):
            got = t.clone()
            assert fn(got) is got
            assert torch.equal(_bits(got), _bits(t)), (op, name)
            expected.append((op, t.numel(), name, "cpu"))
            assert dp.collective_log() == expected
    assert dp.assert_same_collective_sequence() == expected
    vec, scalar = _tensors()
    assert dp.bytes_reduced() == 2 * (4 * vec.numel() + 8)


def test_context_manager_restores_the_previous_state(one_rank_group):
    assert dp.data_parallel() is False
    with dp.force_data_parallel():
        assert dp.data_parallel() is True
        with dp.force_data_parallel(False):
            assert dp.data_parallel() is False
        assert dp.data_parallel() is True
    assert dp.data_parallel() is False
    with pytest.raises(RuntimeError, match="inside"):
        with dp.force_data_parallel(True):
            assert dp.data_parallel() is True
            raise RuntimeError("inside")
    assert dp.data_parallel() is False
    dp.force_data_parallel(True)
    with dp.force_data_parallel(False):
        assert dp.data_parallel() is False
    assert dp.data_parallel() is True                     # the previous value was "on"


def test_shard_range_and_world_size_do_not_follow_forcing(one_rank_group):
    before = (dp.world_size(), dp.rank(), dp.shard_range(4096), dp.shard_range(4096, 3, 8))
    with dp.force_data_parallel():
        assert (dp.world_size(), dp.rank(), dp.shard_range(4096), dp.shard_range(4096, 3, 8)) == before
    assert before == (1, 0, (0, 4096), (1536, 2048))
