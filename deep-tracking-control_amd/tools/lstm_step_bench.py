"""The fused LSTM time step against the GEMM + gate-kernel pair, and the LSTM composite's update step.

    python deep-tracking-control_amd/tools/lstm_step_bench.py [--update] [--reps 20]

(1) dtc_lstm_fwd_fused vs dtc_lstm_fwd: one forward recurrence of T = 24 steps over R = 1024 / 1470 / 1536 rows, H = 512 (the
    recurrent mini-batch of 4096 envs), microseconds per recurrence (median of `reps` timed calls after warm-up).  Run it under
    `rocprofv3 --kernel-trace --stats -- python ...` for the kernel counts (24 lstm_step_fwd_kernel launches per fused recurrence
    against 24 linear_fwd_kernel + 24 lstm_gate_fwd_kernel).
(2) --update: ms per optimisation step of RecurrentDecoderPPO.update() on ActorCriticDecoderRecurrent(rnn_type='lstm', 1 layer,
    H = 512) at 4096 envs x 24 steps (5 epochs x 4 mini-batches = 20 steps per update), after one warm-up update.
Prints one JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dtc_amd import ops  # noqa: E402

DEV = "cuda:0"


def recurrence(R, H, T=24, reps=20):
    g = torch.Generator(device=DEV).manual_seed(R + H)
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g)
    gi, h0, c0 = rn(T, R, 4 * H), 0.5 * rn(R, H), 0.5 * rn(R, H)
    W, b = rn(4 * H, H) / H ** 0.5, 0.1 * rn(4 * H)
    hs, cs, gates = (torch.empty(T + 1, R, H, device=DEV), torch.empty(T + 1, R, H, device=DEV), torch.empty(T, R, 4 * H, device=DEV))
    ws = ops.workspace(ops.lstm_workspace_bytes(T, R, H), DEV)
    out = {}
    for name, fn in (("lstm_fwd", ops.lstm_fwd), ("lstm_fwd_fused", ops.lstm_fwd_fused)):
        for _ in range(3):
            fn(gi, h0, c0, W, b, hs, cs, gates, ws)
        torch.cuda.synchronize()
        times = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(gi, h0, c0, W, b, hs, cs, gates, ws)
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3)
        out[name] = statistics.median(times)
    print(json.dumps(dict(what="lstm_recurrence_us", T=T, R=R, H=H, lstm_fwd=round(out["lstm_fwd"], 1),
                          lstm_fwd_fused=round(out["lstm_fwd_fused"], 1), speedup=round(out["lstm_fwd"] / out["lstm_fwd_fused"], 3))))


def update_step(n=4096, T=24, layers=1, H=512):
    from dtc_amd import synthetic as S
    from dtc_amd.algorithms import RecurrentDecoderPPO
    from dtc_amd.modules import ActorCriticDecoderRecurrent
    torch.manual_seed(3)
    ac = ActorCriticDecoderRecurrent(53, 1389, 12, rnn_type="lstm", rnn_num_layers=layers, rnn_hidden_size=H)
    alg = RecurrentDecoderPPO(ac, learning_rate=1e-3, entropy_coef=0.003, device=DEV)
    alg.init_storage(n, T, [53], [1389], [265], [12])
    d = S.rollout(n, T, seed=9, device=DEV)
    times = []
    for it in range(3):
        with torch.inference_mode():
            for t in range(T):
                alg.act(d["observations"][t], d["privileged_observations"][t], d["observation_histories"][t], d["base_vel"][t])
                alg.process_env_step(d["rewards"][t, :, 0], d["dones"][t, :, 0], d["next_observations"][t], {})
            alg.compute_returns(d["observations"][-1], d["privileged_observations"][-1], d["base_vel"][-1])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        alg.update()
        torch.cuda.synchronize()
        if it > 0:
            times.append((time.perf_counter() - t0) * 1e3 / (alg.num_learning_epochs * alg.num_mini_batches))
    print(json.dumps(dict(what="lstm_composite_update_ms_per_step", envs=n, T=T, layers=layers, H=H,
                          ms_per_step=round(statistics.median(times), 2), runs=[round(x, 2) for x in times])))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--update", action="store_true")
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    for R in (1024, 1470, 1536):
        recurrence(R, 512, reps=a.reps)
    if a.update:
        update_step()
