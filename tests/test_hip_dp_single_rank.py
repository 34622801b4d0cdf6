"""The production exchange on ONE rank: a one-rank `nccl` (RCCL) group forced to count as data parallel
(dtc_amd.distributed.force_data_parallel) runs the trainers' real collective sequence -- the rank-0 broadcast, the two advantage
statistics, every gradient bucket on the weight-gradient stream with ReduceOp.AVG, the KL mean in the first bucket's header (kl_mirror)
and the learning-rate rule after the exchange -- on the library-owned lanes.  An average over one rank multiplies by exactly 1 and every
other launch is the launch of the plain step, so the bound is bit-identity with the same update without the exchange: weights, Adam
state, device and host learning rate.  Every case runs in a freshly spawned child with its own process group."""
import datetime
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = 24


def _trainer(kind, n, epochs):
    """A trainer of `kind` on the synthetic rollout of n envs x 24 steps, from the same weights every time it is called."""
    import test_hip_dp as D
    from dtc_amd import synthetic as S
    full = S.rollout(n, T, seed=4)
    if kind in ("decoder", "composite"):
        if kind == "composite":
            full["dones"][:, 0] = 0
        return D._make(0, 1, full, kind, n_per_rank=n, epochs=epochs)          # (adaptive schedule: the trainers' default)
    from dtc_amd.algorithms import RecurrentPPO
    from dtc_amd.modules import ActorCriticRecurrent
    full["dones"][:, 0] = 0
    torch.manual_seed(3)
    ac = ActorCriticRecurrent(53, 1389, 12, actor_hidden_dims=[512, 256, 128], critic_hidden_dims=[512, 256, 128], activation='elu',
                              rnn_type='gru', rnn_hidden_size=512, rnn_num_layers=1)
    alg = RecurrentPPO(ac, learning_rate=1e-3, entropy_coef=0.003, device=DEV, num_learning_epochs=epochs, schedule="adaptive")
    alg.init_storage(n, T, [53], [1389], [12])
    for k, v in full.items():
        if k not in ("last_values", "observation_histories"):          # the recurrent storage keeps no observation history
            getattr(alg.storage, k).copy_(v.to(DEV))
    alg.storage.compute_returns(full["last_values"].to(DEV), 0.99, 0.95)
    alg.storage.step = T
    g = torch.Generator().manual_seed(55)
    hid = [0.1 * torch.randn(T, 1, n, 512, generator=g).to(DEV) for _ in range(2)]
    alg.storage.saved_hidden_states_a, alg.storage.saved_hidden_states_c = [hid[0]], [hid[1]]
    return alg


def _one_update(kind, n, epochs, forced):
    """One update of a fresh trainer, constructed and run with forcing on or off, on identical weights, rollout, permutation and noise."""
    from dtc_amd import distributed as dp
    with dp.force_data_parallel(forced):
        dp.trace_collectives(True)
        alg = _trainer(kind, n, epochs)
        B = n * T // 4
        g = torch.Generator().manual_seed(100)
        perm = torch.randperm(4 * B, generator=g)
        e1, e2 = torch.randn(4 * epochs, B, 16, generator=g), torch.randn(4 * epochs, B, 16, generator=g)
        if kind == "decoder":
            alg.update(perm.to(DEV), e1.to(DEV), e2.to(DEV))
        elif kind == "composite":
            alg.update(e1.to(DEV), e2.to(DEV))
        else:
            alg.update()
        torch.cuda.synchronize()
        log = dp.assert_same_collective_sequence()
        assert log == dp.collective_log()
        tw = next(iter(alg._tws.values()))
        opts = [alg.optimizer] + ([alg.vae_optimizer] if hasattr(alg, "vae_optimizer") else [])
        state = dict(flat=alg.actor_critic.arena.flat.cpu().clone(), lr=alg.learning_rate)
        for i, opt in enumerate(opts):
            state[f"m{i}"], state[f"v{i}"] = opt.exp_avg.cpu().clone(), opt.exp_avg_sq.cpu().clone()
            state[f"lr_dev{i}"] = opt.lr_dev.cpu().clone()
        return dict(state=state, log=log, bytes=dp.bytes_reduced(log), data_parallel=dp.data_parallel(),
                    lanes=[type(s).__name__ for s in (tw.side, tw.aux)],
                    own_lanes=all(isinstance(s, torch.cuda.ExternalStream) for s in (tw.side, tw.aux)))


def _child(port, out, kind, n, epochs, modes, env):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), **env)
    torch.cuda.set_device(0)
    # a stuck collective ends this child (and fails its test), not the suite
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device(DEV), timeout=datetime.timedelta(seconds=120))
    try:
        for forced in modes:
            out["forced" if forced else "plain"] = _one_update(kind, n, epochs, forced)
    finally:
        dist.destroy_process_group()


def _spawn(kind, n, epochs, modes=(True, False), env=None, limit=300):
    import test_hip_dp as D
    ctx = mp.get_context("spawn")
    out = ctx.Manager().dict()
    p = ctx.Process(target=_child, args=(D._free_port(), out, kind, n, epochs, modes, env or {}))
    p.start()
    p.join(limit)
    assert p.exitcode == 0, f"child exited with {p.exitcode}"
    return dict(out)


def _first_difference(a, b):
    """Name of the first buffer that differs between two trainer states, None when all are equal bit for bit."""
    assert a.keys() == b.keys()
    for k in a:
        same = torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k]
        if not same:
            return k
    return None


@pytest.fixture(scope="module")
def small_decoder():
    """Decoder PPO, 64 envs x 24 steps, 2 epochs: forced and plain update in ONE child."""
    return _spawn("decoder", 64, 2)


def test_forced_exchange_is_bit_identical_to_the_plain_update(small_decoder):
    forced, plain = small_decoder["forced"], small_decoder["plain"]
    assert forced["data_parallel"] is True and plain["data_parallel"] is False
    ops = [e[0] for e in forced["log"]]
    assert ops, "the forced one-rank group issued no collective"
    assert ops[0] == "broadcast" and ops.count("broadcast") == 1           # rank 0's weights, at construction
    assert ops.count("all_reduce_sum") == 2                                 # the advantage statistics
    means = [e for e in forced["log"] if e[0] == "all_reduce_mean"]
    assert len(means) == 8 * 4                                              # 8 mini-batch steps x (2 VAE + 2 policy buckets)
    assert all(e[1] > 1 for e in means) and {e[3] for e in means} == {"side"}
    assert plain["log"] == [] and plain["bytes"] == 0
    assert _first_difference(forced["state"], plain["state"]) is None
    assert torch.isfinite(forced["state"]["flat"]).all()
    assert set(forced["state"]) == {"flat", "lr", "m0", "v0", "lr_dev0", "m1", "v1", "lr_dev1"}


def test_forced_rccl_rank_runs_on_the_librarys_own_lanes(small_decoder):
    assert small_decoder["forced"]["own_lanes"], small_decoder["forced"]["lanes"]


def test_default_priority_lanes_give_the_same_bits(small_decoder):
    out = _spawn("decoder", 64, 2, modes=(True,), env=dict(DTC_LANE_PRIO="none"))
    assert out["forced"]["log"] == small_decoder["forced"]["log"]
    assert _first_difference(out["forced"]["state"], small_decoder["forced"]["state"]) is None


def test_forced_update_repeats_bit_for_bit_in_fresh_processes(small_decoder):
    runs = [small_decoder["forced"]] + [_spawn("decoder", 64, 2, modes=(True,))["forced"] for _ in range(2)]
    for i, other in enumerate(runs[1:], 1):
        assert _first_difference(runs[0]["state"], other["state"]) is None, f"run {i} differs from run 0"
        assert other["log"] == runs[0]["log"]


@pytest.mark.parametrize("kind", ["gru", "composite"])
def test_recurrent_trainers_take_the_same_learning_rate_decisions(kind):
    """RecurrentPPO and RecurrentDecoderPPO, 16 envs x 24 steps, adaptive schedule: forced, the KL mean travels in the gradient header
    and the rule runs after the exchange (kl_mirror + dtc_lr_adapt); plain, the loss kernel adapts the rate itself."""
    out = _spawn(kind, 16, 2)
    forced, plain = out["forced"], out["plain"]
    means = [e for e in forced["log"] if e[0] == "all_reduce_mean"]
    assert means and all(e[1] > 1 for e in means) and {e[3] for e in means} == {"side"}
    assert [e[0] for e in forced["log"]].count("broadcast") == 1
    assert plain["log"] == []
    assert _first_difference(forced["state"], plain["state"]) is None
    assert forced["state"]["lr"] != 1e-3, "the adaptive schedule never moved the learning rate: the comparison shows nothing"
    assert forced["own_lanes"], forced["lanes"]


def test_forced_exchange_at_real_bucket_sizes():
    """Decoder PPO at 4096 envs x 24 steps, 1 epoch: 4 mini-batches of 24576 rows, the buckets of the production step."""
    out = _spawn("decoder", 4096, 1, limit=600)
    forced, plain = out["forced"], out["plain"]
    assert _first_difference(forced["state"], plain["state"]) is None
    assert plain["log"] == []
    # per mini-batch the VAE step's buckets (encoders + decoders: 1 855 245 floats) and the policy step's (4-float header with the KL
    # mean + actor + critic + std + encoders: 1 940 412 floats), and the two advantage statistics
    assert forced["bytes"] == 4 * 4 * (1855245 + 1940412 + 4) + 2 * 8, forced["bytes"]
