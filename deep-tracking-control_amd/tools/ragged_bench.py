"""PPO.update on the operand-image schedule against round 4's converting kernels at mini-batch row counts that are no multiple of 128,
A/B in one process on one GPU.

    timeout -k 10 900 python deep-tracking-control_amd/tools/ragged_bench.py [--pairs 3] [--steps 3] [--warmup 2] >> profiles/ragged_ab.txt

Per env count (default 8, 32, 100, 2000, 4000 envs x 24 steps, 4 mini-batches: 48, 192, 600, 12000, 24000 rows -- the reference's
x30_dtc / lite3_dtc / legged_robot configs and two large ragged sizes): two trainers, PPO(...) and PPO(..., ragged_images=True), same
weights and rollout; the step is compute_returns + PPO.update (5 epochs x 4 mini-batches) on a synthetic recorded rollout resident in
HBM.  `pairs` times: `steps` timed steps of the default trainer, then `steps` of the ragged one (interleaved: both see the same clocks
and the same box); medians and the spread over all timed steps are reported, and which schedule each trainer really ran.

One process, one GPU; bench.py is the project's yardstick, this tool only compares the two schedules.  One JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dtc_amd import synthetic as S  # noqa: E402
from dtc_amd.algorithms import PPO  # noqa: E402
from dtc_amd.modules import ActorCriticDecoder  # noqa: E402

DEV = "cuda:0"
T = 24


def emit(**kw):
    print(json.dumps(kw), flush=True)


def workload(n_envs, ragged):
    data = S.rollout(n_envs, T, seed=4, device=DEV)
    last = {k: data[k][-1].clone() for k in ("observations", "privileged_observations", "base_vel")}
    torch.manual_seed(3)
    ac = ActorCriticDecoder(53, 1389, 12)
    alg = PPO(ac, learning_rate=1e-3, entropy_coef=0.003, device=DEV, ragged_images=ragged)
    alg.init_storage(n_envs, T, [53], [1389], [265], [12])
    for k in list(data):
        if k != "last_values":
            getattr(alg.storage, k).copy_(data.pop(k))
    torch.manual_seed(123)

    def step():
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
    ap.add_argument("--envs", type=int, nargs="+", default=[8, 32, 100, 2000, 4000])
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    assert a.pairs >= 3, "at least three interleaved pairs"
    emit(what="setup", device=torch.cuda.get_device_name(0), steps_per_env=T, mini_batches=4, epochs=5, pairs=a.pairs, steps_per_pair=a.steps,
         warmup=a.warmup, note="one process, one GPU; default and ragged_images=True steps interleaved; step = compute_returns + PPO.update")
    for n in a.envs:
        B = n * T // 4
        (alg0, step0), (alg1, step1) = workload(n, False), workload(n, True)
        for _ in range(a.warmup):
            step0()
            step1()
        on_images = [bool(alg._image_mode(alg.actor_critic._fwd_ws(B))) for alg in (alg0, alg1)]
        every, med = {0: [], 1: []}, {0: [], 1: []}
        for _ in range(a.pairs):
            for p, step in ((0, step0), (1, step1)):
                t = timed(step, a.steps)
                med[p].append(statistics.median(t))
                every[p] += t
        m0, m1 = statistics.median(every[0]), statistics.median(every[1])
        emit(what="update_step", envs=n, mini_batch_rows=B, row_tiles=-(-B // 128), tail_rows=B % 128,
             default_on_images=on_images[0], ragged_on_images=on_images[1],
             default_ms=round(m0, 3), ragged_ms=round(m1, 3), ratio=round(m1 / m0, 4),
             default_pair_medians_ms=[round(t, 3) for t in med[0]], ragged_pair_medians_ms=[round(t, 3) for t in med[1]],
             default_spread_ms=[round(min(every[0]), 3), round(max(every[0]), 3)], ragged_spread_ms=[round(min(every[1]), 3), round(max(every[1]), 3)],
             per_pair_ratio=[round(b / c, 4) for b, c in zip(med[1], med[0])])
        del alg0, alg1, step0, step1
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
