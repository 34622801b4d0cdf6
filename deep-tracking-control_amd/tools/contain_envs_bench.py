"""What contain_nonfinite_envs=True costs, in one process on one GPU.

    timeout -k 10 900 python deep-tracking-control_amd/tools/contain_envs_bench.py [--pairs 3] [--reps 20] [--steps 3] [--warmup 2] >> profiles/contain_envs.txt

(a) The hidden-state scan (ops.states_finite) over one saved-state tensor of the GRU + CE-net composite at `envs` x 24 steps
    ([24, 1, envs, 512] fp32: 201 MB at 4096 envs), beside torch.Tensor.copy_ of the same tensor into a preallocated buffer and the
    existing row scan (ops.rows_finite) on a contiguous [24 * envs, 512] view of it.  `pairs` interleaved rounds of `reps` timed
    repetitions each (device events around each repetition).
(b) The iteration: RolloutStorage.compute_returns + RecurrentDecoderPPO.update (5 epochs x 4 mini-batches) on a clean synthetic rollout
    resident in HBM, flag on against flag off, `pairs` interleaved pairs of `steps` timed steps (host clock around a device synchronise).
    The difference is reported next to the spread of the flag-off steps.
(c) The same step with the flag on and 1, 64 and 2048 envs made invalid before every step (a NaN reward at step 0 of each), interleaved
    with the clean flag-on step.  A repaired env takes its source's `dones`, so the update that follows runs on other trajectory counts
    than the clean one: the whole-step difference is not the repair's cost alone.  RolloutStorage.compute_returns by itself (device
    events, `reps` repetitions) is therefore reported for (b) and for every invalid count: that figure follows the invalid count.

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
from dtc_amd.algorithms import RecurrentDecoderPPO  # noqa: E402
from dtc_amd.modules import ActorCriticDecoderRecurrent  # noqa: E402

DEV = "cuda:0"
T, H = 24, 512


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
    g = torch.Generator(device=DEV).manual_seed(1)
    src = torch.empty(T, 1, n_envs, H, device=DEV).normal_(generator=g)
    dst = torch.empty_like(src)
    flat = src.view(T * n_envs, H)
    rec = torch.ones(T * n_envs, dtype=torch.uint8, device=DEV)
    nbytes = src.numel() * 4
    fns = dict(states_finite=lambda: ops.states_finite(src, rec), copy=lambda: dst.copy_(src), rows_finite=lambda: ops.rows_finite([flat], out=rec))
    for _ in range(3):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    assert bool((rec == 1).all())
    times = {k: [] for k in fns}
    for _ in range(pairs):
        for k, fn in fns.items():
            times[k].append(event_times(fn, reps))
    med = {k: statistics.median(sum(v, [])) for k, v in times.items()}
    emit(what="states_scan", envs=n_envs, shape=list(src.shape), read_bytes=nbytes,
         **{f"{k}_us": round(m, 1) for k, m in med.items()}, **{f"{k}_read_GBps": round(nbytes / m / 1e3, 1) for k, m in med.items()},
         **{f"{k}_round_medians_us": [round(statistics.median(t), 1) for t in times[k]] for k in fns},
         **{f"{k}_spread_us": [round(min(sum(times[k], [])), 1), round(max(sum(times[k], [])), 1)] for k in fns},
         states_over_rows_finite=round(med["states_finite"] / med["rows_finite"], 4), states_over_copy=round(med["states_finite"] / med["copy"], 4))
    del src, dst, rec
    torch.cuda.empty_cache()


def workload(n_envs, contain, n_invalid=0):
    data = S.rollout(n_envs, T, seed=4, device=DEV)
    data["dones"][:, 0] = 0
    torch.manual_seed(3)
    alg = RecurrentDecoderPPO(ActorCriticDecoderRecurrent(53, 1389, 12), learning_rate=1e-3, entropy_coef=0.003, device=DEV,
                              contain_nonfinite_envs=contain)
    alg.init_storage(n_envs, T, [53], [1389], [265], [12])
    last_values = data.pop("last_values")
    for k in list(data):
        getattr(alg.storage, k).copy_(data.pop(k))
    g = torch.Generator(device=DEV).manual_seed(55)
    alg.storage.saved_hidden_states_a, alg.storage.saved_hidden_states_c = ([0.1 * torch.empty(T, 1, n_envs, H, device=DEV).normal_(generator=g)]
                                                                            for _ in range(2))
    # the invalid envs of every step, spread over the env range (the repair cleans them: planted again in front of every step)
    bad = (torch.arange(n_invalid, device=DEV) * (n_envs // max(n_invalid, 1))) if n_invalid else torch.zeros(0, dtype=torch.int64, device=DEV)
    torch.manual_seed(123)

    def returns_only():
        alg.storage.compute_returns(last_values, 0.99, 0.95)

    def step():
        alg.storage.rewards[0, bad] = float("nan")
        returns_only()
        alg.storage.step = T
        return alg.update()

    def returns_us(reps):
        """device time of compute_returns alone (the planting stays outside the events)"""
        out = []
        for _ in range(reps):
            alg.storage.rewards[0, bad] = float("nan")
            out += event_times(returns_only, 1)
        alg.storage.clear()
        return out
    step.returns_us = returns_us
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


def interleaved(variants, pairs, steps, warmup):
    """variants: name -> step function; returns name -> (every time, the medians of its rounds)"""
    for _ in range(warmup):
        for step in variants.values():
            step()
    every, med = {k: [] for k in variants}, {k: [] for k in variants}
    for _ in range(pairs):
        for k, step in variants.items():
            t = timed(step, steps)
            med[k].append(statistics.median(t))
            every[k] += t
    return every, med


def report(every, med, k):
    return {f"{k}_ms": round(statistics.median(every[k]), 3), f"{k}_round_medians_ms": [round(t, 3) for t in med[k]],
            f"{k}_spread_ms": [round(min(every[k]), 3), round(max(every[k]), 3)]}


def iteration(n_envs, pairs, steps, warmup, reps):
    (alg0, step0), (alg1, step1) = workload(n_envs, False), workload(n_envs, True)
    every, med = interleaved(dict(off=step0, on=step1), pairs, steps, warmup)
    m0, m1 = statistics.median(every["off"]), statistics.median(every["on"])
    r0, r1 = step0.returns_us(reps), step1.returns_us(reps)
    emit(what="compute_returns", envs=n_envs, invalid=0, off_us=round(statistics.median(r0), 1), on_us=round(statistics.median(r1), 1),
         off_spread_us=[round(min(r0), 1), round(max(r0), 1)], on_spread_us=[round(min(r1), 1), round(max(r1), 1)],
         note="device events around RolloutStorage.compute_returns alone")
    emit(what="iteration", envs=n_envs, step="compute_returns + RecurrentDecoderPPO.update, clean rollout", **report(every, med, "off"),
         **report(every, med, "on"), difference_ms=round(m1 - m0, 3), ratio=round(m1 / m0, 5),
         off_run_to_run_ms=round(max(every["off"]) - min(every["off"]), 3), nonfinite_envs=alg1.last_nonfinite_envs)
    assert alg1.last_nonfinite_envs == 0
    del alg0, step0
    torch.cuda.empty_cache()
    return alg1, step1


def invalid_counts(n_envs, clean, counts, pairs, steps, warmup, reps):
    for n_bad in counts:
        alg, step = workload(n_envs, True, n_bad)
        every, med = interleaved(dict(clean=clean[1], dirty=step), pairs, steps, warmup)
        m0, m1 = statistics.median(every["clean"]), statistics.median(every["dirty"])
        assert alg.last_nonfinite_envs == n_bad, (alg.last_nonfinite_envs, n_bad)
        assert bool(torch.isfinite(alg.actor_critic.arena.flat).all())
        r = step.returns_us(reps)
        emit(what="compute_returns", envs=n_envs, invalid=n_bad, on_us=round(statistics.median(r), 1), on_spread_us=[round(min(r), 1), round(max(r), 1)],
             note="device events around RolloutStorage.compute_returns alone, the invalid envs planted in front of every repetition")
        emit(what="invalid_envs", envs=n_envs, invalid=n_bad, step="compute_returns + RecurrentDecoderPPO.update, flag on", **report(every, med, "clean"),
             **report(every, med, "dirty"), difference_ms=round(m1 - m0, 3), nonfinite_envs=alg.last_nonfinite_envs,
             note="`dirty` includes the indexed write that plants the NaN rewards; `clean` runs the same write with an empty index")
        del alg, step
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--invalid", type=int, nargs="*", default=[1, 64, 2048])
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    assert a.pairs >= 3, "at least three interleaved pairs"
    emit(what="setup", device=torch.cuda.get_device_name(0), steps_per_env=T, pairs=a.pairs, reps_per_pair=a.reps, steps_per_pair=a.steps,
         warmup=a.warmup, note="one process, one GPU; every comparison interleaved")
    scan_against_copy(a.envs, a.pairs, a.reps)
    clean = iteration(a.envs, a.pairs, a.steps, a.warmup, a.reps)
    invalid_counts(a.envs, clean, a.invalid, a.pairs, a.steps, a.warmup, a.reps)


if __name__ == "__main__":
    main()
