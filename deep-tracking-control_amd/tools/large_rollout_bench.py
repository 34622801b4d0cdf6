"""Rollouts beyond 2 GiB per tensor on one GPU: the benchmark's step at 4096, 16 000 and 32 768 envs x 24 steps.

    timeout -k 10 900 python deep-tracking-control_amd/tools/large_rollout_bench.py [--sizes 4096,16000,32768] [--steps 3] [--warmup 1]
                                                                                     [--composite] > profiles/large_rollout.txt

Per size, on a synthetic recorded rollout resident in HBM (dtc_amd.synthetic, as bench.py): foothold planner over all (step, env) height
maps + compute_returns + PPO.update (5 epochs x 4 mini-batches), `warmup` untimed steps, then the median of `steps` timed ones: ms per
step, env-steps/s, torch.cuda.max_memory_allocated.  At 32 768 envs the privileged observations are a 4.37 GB tensor: the image packs and
the loss layer's target load run their 64-bit instantiations (csrc/gemm_h2i.hip); 16 000 envs is the largest round size below 2 GiB.
When the largest size's env-steps/s falls more than 4 % below the smallest's, the per-kernel table of one more step at both sizes follows.
--composite: the same for RecurrentDecoderPPO (GRU + CE-net composite) at the largest size.

Then, interleaved in this process on ONE source below 2 GiB (98 304 x 1389 floats) so that both instantiations can read it: the time per
launch of the image pack of 24 576 gathered rows (the three operand forms of a training step) and of the fused MSE layer
(24 576 x 512 -> 693), narrow against wide.  The wide forms are reached through descriptors that declare the source with the rows of a
32 768-env rollout (the kernels bound their reads by it; the gathered rows all exist).

One process, one GPU.  Multi-GPU scaling is not measured here and this tool does not stand in for it.  One JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dtc_amd import _ffi, foothold, h2i, synthetic as S  # noqa: E402
from dtc_amd.algorithms import PPO, RecurrentDecoderPPO  # noqa: E402
from dtc_amd.modules import ActorCriticDecoder, ActorCriticDecoderRecurrent  # noqa: E402

DEV = "cuda:0"
T = 24
BIG_ROWS = 32768 * T


def emit(**kw):
    print(json.dumps(kw), flush=True)


def workload(n_envs, composite=False):
    """(trainer, step closure) as bench.py's make_workload on one rank."""
    data = S.rollout(n_envs, T, seed=4, device=DEV)
    sc = S.scorer_inputs(n_envs * T, seed=7, device=DEV)
    last = {k: data[k][-1].clone() for k in ("observations", "privileged_observations", "base_vel")}
    torch.manual_seed(3)
    ac = (ActorCriticDecoderRecurrent if composite else ActorCriticDecoder)(53, 1389, 12)
    alg = (RecurrentDecoderPPO if composite else PPO)(ac, learning_rate=1e-3, entropy_coef=0.003, device=DEV)
    alg.init_storage(n_envs, T, [53], [1389], [265], [12])
    for k in list(data):
        if k != "last_values":
            getattr(alg.storage, k).copy_(data.pop(k))
    hid = None
    if composite:
        g = torch.Generator(device=DEV).manual_seed(77)
        hid = [0.1 * torch.randn(T, 1, n_envs, 512, generator=g, device=DEV) for _ in range(2)]
    torch.manual_seed(123)

    def step():
        foothold.plan(sc["measured_heights"], sc["root_states"], sc["thigh_pos"], sc["commands"])
        alg.compute_returns(last["observations"], last["privileged_observations"], last["base_vel"])
        alg.storage.step = T
        if composite:
            alg.storage.saved_hidden_states_a, alg.storage.saved_hidden_states_c = [hid[0]], [hid[1]]
        return alg.update()
    return alg, step


def run_size(n_envs, steps, warmup, composite=False, kernel_table=False):
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    alg, step = workload(n_envs, composite)
    for _ in range(warmup):
        out = step()
    torch.cuda.synchronize()
    times = []
    for _ in range(steps):
        t0 = time.perf_counter()
        out = step()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    ms = statistics.median(times)
    rec = dict(what="composite_step" if composite else "step", envs=n_envs, steps_per_env=T, mini_batch_rows=n_envs * T // 4,
               privileged_bytes=alg.storage.privileged_observations.numel() * 4, ms_per_step=round(ms, 2), ms_all=[round(t, 2) for t in times],
               env_steps_per_s=round(n_envs * T / (ms * 1e-3)), peak_memory_bytes=torch.cuda.max_memory_allocated(),
               mean_losses=[round(float(v), 6) for v in out])
    emit(**rec)
    if kernel_table:
        lib = _ffi.lib()
        lib.dtc_prof_reset()
        lib.dtc_prof_enable(1)
        step()
        torch.cuda.synchronize()
        lib.dtc_prof_enable(0)
        rows = sorted(_ffi.prof_report(), key=lambda r: -r["ms_total"])
        total = sum(r["ms_total"] for r in rows)
        emit(what="kernel_table", envs=n_envs, note="one profiled step (serialising events: clocks lower than the timed steps); ms summed per family",
             ms_total=round(total, 2), rows=[dict(name=r["name"], ms=round(r["ms_total"], 3), launches=r["launches"]) for r in rows[:24]])
    return rec


def per_launch(fn, reps=20, inner=10):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / inner)
    return round(statistics.median(times), 1)


def narrow_against_wide(reps):
    """Both instantiations on the same source below 2 GiB, interleaved: narrow, wide, narrow, wide ... per measurement."""
    from dtc_amd._ffi import seg, segmat
    rows, M = 4096 * T, 24576
    g = torch.Generator(device=DEV).manual_seed(5)
    priv, obs, vel = (torch.randn(rows, w, generator=g, device=DEV) for w in (1389, 53, 3))
    idx = torch.randperm(rows, generator=g, device=DEV)[:M].contiguous()

    def declare(m, wide):
        for i in range(m.nseg):
            if m.seg[i].gather:
                m.seg[i].rows = BIG_ROWS if wide else rows           # the wide kernel is chosen from rows x ld of the descriptor
        return m
    forms = dict(heights_693=lambda: segmat([seg(priv, 0, 693, gather=True)], idx),
                 critic_752=lambda: segmat([seg(obs, 0, 53, gather=True), seg(vel, 0, 3, gather=True), seg(priv, 693, 696, gather=True)], idx),
                 observations_53=lambda: segmat([seg(obs, 0, 53, gather=True)], idx))
    lib = _ffi.lib()
    for name, make in forms.items():
        mn, mw = declare(make(), False), declare(make(), True)
        img_n, img_w = h2i.HImage(M, mn.cols, DEV), h2i.HImage(M, mn.cols, DEV)
        res = {}
        for rnd in range(3):
            for key, m, img in (("narrow", mn, img_n), ("wide", mw, img_w)):
                res.setdefault(key, []).append(per_launch(lambda: _ffi.check(lib.dtc_h2i_pack(m, M, img.ptr(), _ffi.stream()), "dtc_h2i_pack"), reps))
        assert torch.equal(img_n.buf.view(torch.int64), img_w.buf.view(torch.int64))
        emit(what="h2i_pack_us_per_launch", operand=name, rows=M, source_rows=rows, narrow=res["narrow"], wide=res["wide"], images_equal=True)
    K, N = 512, 693
    X = h2i.HImage.from_tensor(torch.randn(M, K, generator=g, device=DEV))
    W, b = torch.randn(N, K, generator=g, device=DEV) / K ** 0.5, torch.randn(N, generator=g, device=DEV)
    wimg = h2i.WeightSet().get(W, 0, [(0, N)], [(0, K)])
    op, _ = h2i._operand(X)
    outs = {}
    for key in ("narrow", "wide"):
        outs[key] = (h2i.HImage(M, N, DEV), torch.zeros(h2i.mse_parts(M, N), dtype=torch.float64, device=DEV))

    def mse(key):
        img, part = outs[key]
        _ffi.check(lib.dtc_linear_fwd_mse_h2i(op, _ffi.ptr(wimg), _ffi.ptr(b), _ffi.ptr(priv), priv.stride(0), BIG_ROWS if key == "wide" else rows,
                                              696, _ffi.ptr(idx), 2.0 / (M * N), None, 0, img.ptr(), _ffi.ptr(part), M, N, _ffi.stream()),
                   "dtc_linear_fwd_mse_h2i")
    res = {}
    for rnd in range(3):
        for key in ("narrow", "wide"):
            res.setdefault(key, []).append(per_launch(lambda: mse(key), reps))
    assert torch.equal(outs["narrow"][0].buf.view(torch.int64), outs["wide"][0].buf.view(torch.int64)) and torch.equal(outs["narrow"][1], outs["wide"][1])
    emit(what="linear_fwd_mse_us_per_launch", M=M, K=K, N=N, source_rows=rows, narrow=res["narrow"], wide=res["wide"], results_equal=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,16000,32768")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--composite", action="store_true")
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]
    emit(what="setup", device=torch.cuda.get_device_name(0), sizes=sizes, steps=a.steps, warmup=a.warmup,
         note="one process, one GPU; multi-GPU scaling is not measured by this tool")
    recs = [run_size(n, a.steps, a.warmup) for n in sizes]
    lo, hi = recs[0], recs[-1]
    ratio = hi["env_steps_per_s"] / lo["env_steps_per_s"]
    emit(what="largest_against_smallest", envs=[lo["envs"], hi["envs"]], env_steps_per_s_ratio=round(ratio, 4), kernel_table_follows=ratio < 0.96)
    if ratio < 0.96:
        for n in (lo["envs"], hi["envs"]):
            run_size(n, 1, 1, kernel_table=True)
    if a.composite:
        run_size(sizes[-1], a.steps, a.warmup, composite=True)
    torch.cuda.empty_cache()
    narrow_against_wide(a.reps)


if __name__ == "__main__":
    main()
