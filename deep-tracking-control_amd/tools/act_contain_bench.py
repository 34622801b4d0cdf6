"""What contain_nonfinite_act=True costs, in one process on one GPU.

    timeout -k 10 600 python deep-tracking-control_amd/tools/act_contain_bench.py [--envs 4096] [--rounds 3] [--reps 50] >> profiles/act_contain.txt

For each of three models -- PPO with the decoder, RecurrentPPO with a 2-layer LSTM (H = 50), RecurrentDecoderPPO (1-layer GRU, H = 512):
(a) the kernel: ops.act_contain over the tensors of one clean rollout step (what act() hands it: the step's inputs, mean, value,
    log-probability, actions, live states), beside torch.Tensor.copy_ of the same bytes (one copy_ per tensor into preallocated
    buffers: it reads AND writes them, the kernel only reads).  Device events around each repetition;
(b) act() + process_env_step() with the flag on against off: host clock around a device synchronise, per step.
`rounds` interleaved rounds of `reps` repetitions each; medians per round and over all, and the spread.

Nothing here is a pass / fail threshold; bench.py is the project's yardstick, this tool only prices the feature.  One JSON line per
measurement."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dtc_amd import ops, synthetic as S  # noqa: E402
from dtc_amd.algorithms import PPO, RecurrentDecoderPPO, RecurrentPPO  # noqa: E402
from dtc_amd.modules import ActorCriticDecoder, ActorCriticDecoderRecurrent, ActorCriticRecurrent  # noqa: E402

DEV = "cuda:0"
T = 24
MODELS = ("ppo", "rppo_lstm2", "rdppo")


def emit(**kw):
    print(json.dumps(kw), flush=True)


def make(kind, n_envs, flag):
    common = dict(learning_rate=1e-3, entropy_coef=0.003, device=DEV, contain_nonfinite_envs=True, contain_nonfinite_act=flag)
    torch.manual_seed(3)
    if kind == "ppo":
        alg = PPO(ActorCriticDecoder(53, 1389, 12), **common)
    elif kind == "rdppo":
        alg = RecurrentDecoderPPO(ActorCriticDecoderRecurrent(53, 1389, 12), **common)
    else:
        alg = RecurrentPPO(ActorCriticRecurrent(53, 1389, 12, actor_hidden_dims=[512, 256, 128], critic_hidden_dims=[512, 256, 128],
                                                 activation='elu', rnn_type="lstm", rnn_hidden_size=50, rnn_num_layers=2), **common)
    if kind.startswith("rppo"):
        alg.init_storage(n_envs, T, [53], [1389], [12])
    else:
        alg.init_storage(n_envs, T, [53], [1389], [265], [12])
    return alg


def stepper(kind, alg, d):
    """-> one rollout step (act + process_env_step; the storage is cleared when full, which a trainer's update() does)"""
    plain = kind.startswith("rppo")
    state = dict(t=0)

    def step():
        t = state["t"]
        if alg.storage.step == T:
            alg.storage.clear()
        if plain:
            alg.act(d["observations"][t], d["privileged_observations"][t])
        else:
            alg.act(d["observations"][t], d["privileged_observations"][t], d["observation_histories"][t], d["base_vel"][t])
        alg.process_env_step(rewards=d["rewards"][t, :, 0], dones=d["dones"][t, :, 0], next_obs=d["next_observations"][t], infos={})
        state["t"] = (t + 1) % T
    return step


def step_tensors(kind, alg, d):
    """the scan and repair lists of contain_act for the step act() ran last, as clones (the measurement keeps them to itself)"""
    tr, ac = alg.transition, alg.actor_critic
    plain = kind.startswith("rppo")
    inputs = [d["observations"][0], d["privileged_observations"][0]] + ([] if plain else [d["observation_histories"][0], d["base_vel"][0]])
    alg.act(*inputs)
    states = []
    if hasattr(ac, "memory_a"):
        for h in ac.get_hidden_states():
            states += list(h) if isinstance(h, (tuple, list)) else [h]
    scan = [t.clone() for t in (*inputs, tr.action_mean, tr.values, tr.actions_log_prob)]
    repair = [t.clone() for t in (tr.actions, *states)]
    alg.process_env_step(rewards=d["rewards"][0, :, 0], dones=d["dones"][0, :, 0], next_obs=d["next_observations"][0], infos={})
    alg.storage.clear()
    return scan, repair


def event_times(fn, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)          # us
    return out


def host_times(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6)  # us
    return out


def summary(name, rounds):
    every = sum(rounds, [])
    return {f"{name}_us": round(statistics.median(every), 1), f"{name}_round_medians_us": [round(statistics.median(r), 1) for r in rounds],
            f"{name}_spread_us": [round(min(every), 1), round(max(every), 1)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    assert a.rounds >= 3, "at least three interleaved rounds"
    emit(what="setup", device=torch.cuda.get_device_name(0), envs=a.envs, rounds=a.rounds, reps_per_round=a.reps,
         note="one process, one GPU; every comparison interleaved")
    d = S.rollout(a.envs, T, seed=4, device=DEV)
    for kind in MODELS:
        off, on = make(kind, a.envs, False), make(kind, a.envs, True)
        scan, repair = step_tensors(kind, on, d)
        tensors = scan + repair
        copies = [torch.empty_like(t) for t in tensors]
        valid, bad = torch.ones(a.envs, dtype=torch.uint8, device=DEV), torch.zeros(a.envs, dtype=torch.uint8, device=DEV)
        nbytes = sum(t.numel() * 4 for t in tensors)

        def kernel():
            ops.act_contain(scan=scan, repair=repair, act_valid_row=valid, env_bad=bad)

        def copy():
            for dst, src in zip(copies, tensors):
                dst.copy_(src)
        fns = dict(kernel=kernel, copy=copy, act_off=stepper(kind, off, d), act_on=stepper(kind, on, d))
        for fn in fns.values():
            for _ in range(T + 2):
                fn()
        torch.cuda.synchronize()
        assert bool((valid == 1).all()) and not bool(bad.any())
        times = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, fn in fns.items():
                times[k].append((event_times if k in ("kernel", "copy") else host_times)(fn, a.reps))
        med = {k: statistics.median(sum(v, [])) for k, v in times.items()}
        emit(what="act_contain_kernel", model=kind, envs=a.envs, tensors=len(tensors), bytes=nbytes, **summary("kernel", times["kernel"]),
             **summary("copy", times["copy"]), kernel_read_GBps=round(nbytes / med["kernel"] / 1e3, 1), kernel_over_copy=round(med["kernel"] / med["copy"], 4),
             note="device events; `copy` is one copy_ per tensor of the same bytes")
        emit(what="act_step", model=kind, envs=a.envs, step="act + process_env_step, clean rollout", **summary("act_off", times["act_off"]),
             **summary("act_on", times["act_on"]), difference_us=round(med["act_on"] - med["act_off"], 1), ratio=round(med["act_on"] / med["act_off"], 4),
             note="host clock around a device synchronise, per step")
        assert bool((on.storage.act_valid == 1).all()) and not bool(on.nonfinite_act_envs.any())
        del off, on, fns, scan, repair, tensors, copies
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
