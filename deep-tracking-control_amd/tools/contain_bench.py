"""What PPO(..., contain_nonfinite=True) costs, in one process on one GPU.

    timeout -k 10 900 python deep-tracking-control_amd/tools/contain_bench.py [--pairs 3] [--reps 20] [--steps 3] [--warmup 2] >> profiles/contain_scan.txt

1. The row scan (ops.rows_finite) over the eleven stored fp32 tensors of a rollout of `envs` x 24 steps (7.2 KB per row), beside
   torch.Tensor.copy_ of the same eleven tensors into preallocated buffers: the scan reads what the copy reads and writes almost
   nothing, so it has to take no longer than the copy, which moves twice the bytes.  `pairs` interleaved pairs of `reps` timed
   repetitions each (device events around each repetition); at 4096 envs and, where the device has the memory, at 32768.
2. The iteration: compute_returns + PPO.update (5 epochs x 4 mini-batches) on a clean synthetic rollout of 4096 envs resident in HBM,
   flag on against flag off, `pairs` interleaved pairs of `steps` timed steps (host clock around a device synchronise).

bench.py is the project's yardstick; this tool only prices the feature.  One JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dtc_amd import ops, synthetic as S  # noqa: E402
from dtc_amd.algorithms import PPO  # noqa: E402
from dtc_amd.modules import ActorCriticDecoder  # noqa: E402

DEV = "cuda:0"
T = 24
WIDTHS = dict(observations=53, next_observations=53, privileged_observations=1389, observation_histories=265, actions=12, rewards=1,
              values=1, actions_log_prob=1, mu=12, sigma=12, base_vel=3)


def emit(**kw):
    print(json.dumps(kw), flush=True)


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


def scan_against_copy(n_envs, pairs, reps):
    rows = n_envs * T
    nbytes = 4 * rows * sum(WIDTHS.values())
    free, _ = torch.cuda.mem_get_info()
    if free < 2.2 * nbytes + (1 << 30):
        emit(what="scan", envs=n_envs, rows=rows, skipped=f"needs {2.2 * nbytes / 2 ** 30:.1f} GiB for the tensors and their copies, {free / 2 ** 30:.1f} GiB free")
        return
    g = torch.Generator(device=DEV).manual_seed(1)
    src = [torch.empty(rows, w, device=DEV).normal_(generator=g) for w in WIDTHS.values()]
    dst = [torch.empty_like(t) for t in src]
    rec = torch.ones(rows, dtype=torch.uint8, device=DEV)

    def scan():
        ops.rows_finite(src, out=rec)

    def copy():
        for d, s in zip(dst, src):
            d.copy_(s)

    for _ in range(3):
        scan()
        copy()
    torch.cuda.synchronize()
    assert bool((rec == 1).all())
    ts, tc = [], []
    for _ in range(pairs):
        ts.append(event_times(scan, reps))
        tc.append(event_times(copy, reps))
    ms, mc = statistics.median(sum(ts, [])), statistics.median(sum(tc, []))
    emit(what="scan", envs=n_envs, rows=rows, tensors=len(src), read_bytes=nbytes, scan_us=round(ms, 1), scan_GBps=round(nbytes / ms / 1e3, 1),
         copy_us=round(mc, 1), copy_read_GBps=round(nbytes / mc / 1e3, 1), scan_over_copy=round(ms / mc, 4),
         scan_pair_medians_us=[round(statistics.median(t), 1) for t in ts], copy_pair_medians_us=[round(statistics.median(t), 1) for t in tc],
         scan_spread_us=[round(min(sum(ts, [])), 1), round(max(sum(ts, [])), 1)], copy_spread_us=[round(min(sum(tc, [])), 1), round(max(sum(tc, [])), 1)],
         scan_no_longer_than_copy=bool(ms <= mc))
    del src, dst, rec
    torch.cuda.empty_cache()


def workload(n_envs, contain):
    data = S.rollout(n_envs, T, seed=4, device=DEV)
    last = {k: data[k][-1].clone() for k in ("observations", "privileged_observations", "base_vel")}
    torch.manual_seed(3)
    ac = ActorCriticDecoder(53, 1389, 12)
    alg = PPO(ac, learning_rate=1e-3, entropy_coef=0.003, device=DEV, contain_nonfinite=contain)
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


def iteration(n_envs, pairs, steps, warmup):
    (alg0, step0), (alg1, step1) = workload(n_envs, False), workload(n_envs, True)
    for _ in range(warmup):
        step0()
        step1()
    every, med = {0: [], 1: []}, {0: [], 1: []}
    for _ in range(pairs):
        for p, step in ((0, step0), (1, step1)):
            t = timed(step, steps)
            med[p].append(statistics.median(t))
            every[p] += t
    m0, m1 = statistics.median(every[0]), statistics.median(every[1])
    emit(what="iteration", envs=n_envs, mini_batch_rows=n_envs * T // 4, step="compute_returns + PPO.update, clean rollout",
         off_ms=round(m0, 3), on_ms=round(m1, 3), difference_ms=round(m1 - m0, 3), ratio=round(m1 / m0, 5),
         off_pair_medians_ms=[round(t, 3) for t in med[0]], on_pair_medians_ms=[round(t, 3) for t in med[1]],
         off_spread_ms=[round(min(every[0]), 3), round(max(every[0]), 3)], on_spread_ms=[round(min(every[1]), 3), round(max(every[1]), 3)],
         nonfinite_rows=alg1.last_nonfinite_rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[4096, 32768])
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    assert a.pairs >= 3, "at least three interleaved pairs"
    emit(what="setup", device=torch.cuda.get_device_name(0), steps_per_env=T, pairs=a.pairs, reps_per_pair=a.reps, steps_per_pair=a.steps,
         warmup=a.warmup, note="one process, one GPU; scan / copy and flag on / off interleaved")
    for n in a.envs:
        scan_against_copy(n, a.pairs, a.reps)
    iteration(a.envs[0], a.pairs, a.steps, a.warmup)


if __name__ == "__main__":
    main()
