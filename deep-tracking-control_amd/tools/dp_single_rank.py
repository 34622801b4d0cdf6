"""The data-parallel exchange of the PPO update on ONE rank, against the same step without it: A/B in one process on one GPU.

    timeout -k 10 600 python deep-tracking-control_amd/tools/dp_single_rank.py [--pairs 3] [--steps 3] [--warmup 2] > profiles/dp_single_rank.txt

One process, a one-rank `nccl` (RCCL) process group.  The step is the closure bench.py times at its second configuration: 4096 envs x 24
steps -- foothold planner + compute_returns + PPO.update (5 epochs x 4 mini-batches of 24 576 rows) on a synthetic recorded rollout
resident in HBM.  Two trainers on the same weights and rollout: one constructed and stepped under distributed.force_data_parallel() --
every gradient bucket goes through ncclAllReduce (ReduceOp.AVG) on the weight-gradient stream, the KL mean rides in the first bucket's
header, the learning-rate rule runs after the exchange, the advantage statistics are all-reduced --, one plain.  `pairs` times: `steps`
timed steps of the forced trainer, then `steps` of the plain one (interleaved, so both see the same clocks and the same box).  Reported:
ms per step of both, their difference against the run-to-run spread of the pairs, and the number and bytes of collectives per step from
the collective trace.

What this measures: the cost of ISSUING the production collective sequence and of the ordering it imposes on the lanes.  What it cannot
measure: a one-rank all-reduce moves no data between devices, so the xGMI transfer time of N > 1 ranks is not in these numbers.

bench.py is the project's yardstick; this tool only compares the two modes.  One JSON line per measurement."""
import argparse
import datetime
import json
import os
import socket
import statistics
import sys
import time

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dtc_amd import distributed as dp, foothold, synthetic as S  # noqa: E402
from dtc_amd.algorithms import PPO  # noqa: E402
from dtc_amd.modules import ActorCriticDecoder  # noqa: E402

DEV = "cuda:0"
T, N_ENVS = 24, 4096


def emit(**kw):
    print(json.dumps(kw), flush=True)


def workload(forced):
    """(trainer, step closure) as bench.py's make_workload on one rank at 4096 envs; constructed and stepped with forcing on or off."""
    data = S.rollout(N_ENVS, T, seed=4, device=DEV)
    sc = S.scorer_inputs(N_ENVS * T, seed=7, device=DEV)
    last = {k: data[k][-1].clone() for k in ("observations", "privileged_observations", "base_vel")}
    torch.manual_seed(3)
    with dp.force_data_parallel(forced):
        alg = PPO(ActorCriticDecoder(53, 1389, 12), learning_rate=1e-3, entropy_coef=0.003, device=DEV)
    alg.init_storage(N_ENVS, T, [53], [1389], [265], [12])
    for k in list(data):
        if k != "last_values":
            getattr(alg.storage, k).copy_(data.pop(k))

    def step():
        with dp.force_data_parallel(forced):
            foothold.plan(sc["measured_heights"], sc["root_states"], sc["thigh_pos"], sc["commands"])
            alg.compute_returns(last["observations"], last["privileged_observations"], last["base_vel"])
            alg.storage.step = T
            return alg.update()
    return alg, step


def timed(step, n):
    times = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        step()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    assert a.pairs >= 3, "at least three interleaved pairs"
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device(DEV), timeout=datetime.timedelta(seconds=120))
    try:
        emit(what="setup", device=torch.cuda.get_device_name(0), backend=dp.backend(), world_size=dp.world_size(), envs=N_ENVS, steps_per_env=T,
             mini_batch_rows=N_ENVS * T // 4, pairs=a.pairs, steps_per_pair=a.steps, warmup=a.warmup,
             note="one process, one GPU, a one-rank process group; forced-exchange and plain steps interleaved")
        (algf, stepf), (algp, stepp) = workload(True), workload(False)
        for _ in range(a.warmup):
            stepf()
            stepp()
        tw = next(iter(algf._tws.values()))
        emit(what="lanes", side=type(tw.side).__name__, aux=type(tw.aux).__name__,
             note="ExternalStream: a stream of the library's own (dtc_stream_create), not an entry of torch's pool")
        med = dict(forced=[], plain=[])
        every = dict(forced=[], plain=[])
        for _ in range(a.pairs):
            for name, step in (("forced", stepf), ("plain", stepp)):
                t = timed(step, a.steps)
                med[name].append(statistics.median(t))
                every[name] += t
        for name in ("forced", "plain"):
            emit(what="step", mode=name, ms_per_step=round(statistics.median(every[name]), 2), pair_medians_ms=[round(t, 2) for t in med[name]],
                 spread_ms=[round(min(every[name]), 2), round(max(every[name]), 2)],
                 env_steps_per_s=round(N_ENVS * T / (statistics.median(every[name]) * 1e-3)))
        mf, mp_ = statistics.median(every["forced"]), statistics.median(every["plain"])
        per_pair = [round(f - p, 2) for f, p in zip(med["forced"], med["plain"])]
        spread = max(max(med[name]) - min(med[name]) for name in ("forced", "plain"))
        emit(what="forced_exchange_against_plain", ms_per_step=[round(mf, 2), round(mp_, 2)], difference_ms=round(mf - mp_, 2),
             per_pair_difference_ms=per_pair, pair_median_spread_ms=round(spread, 2),
             inside_run_to_run_spread=bool(abs(mf - mp_) <= spread),
             note="difference = issuing the collectives + the ordering they impose; a one-rank exchange moves no data between devices")
        # the collectives of one step, from the trace
        for name, step in (("forced", stepf), ("plain", stepp)):
            dp.trace_collectives(True)
            step()
            torch.cuda.synchronize()
            log = dp.collective_log()
            dp.trace_collectives(False)
            kinds = {}
            for op, numel, dtype, stream in log:
                k = f"{op}/{dtype}/{stream}"
                kinds[k] = kinds.get(k, 0) + 1
            buckets = sorted({numel for op, numel, _, _ in log if op == "all_reduce_mean"})
            emit(what="collectives_per_step", mode=name, count=len(log), all_reduce_bytes=dp.bytes_reduced(log), by_kind=kinds,
                 bucket_floats=buckets)
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
