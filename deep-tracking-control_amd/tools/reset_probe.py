"""Time and count the env reset: the torch restatement of LeggedRobot.reset_idx (legged_robot.py:200-272, with its
`reset_buf.nonzero()`; what an env runs without dtc_amd.reset) against `dtc_amd.reset.EnvReset` (two launches, no host read).

    python deep-tracking-control_amd/tools/reset_probe.py                       # the timing table (needs the GPU)
    python deep-tracking-control_amd/tools/reset_probe.py --launches DIR        # + kernel launches per call from rocprofv3 runs

Timing: for each env count and reset mask, (a) and (b) alternate in one process; every timed call is a host-clock window that
ends in a device synchronise; the figure is the median of --calls (>= 200) such windows after --warmup calls of each side.
Launch counts: child runs of this file (`--count-side a|b --count-calls K`) under `rocprofv3 --kernel-trace --stats`, one per
(side, mask, K); launches per call = (kernels at K = 25 - kernels at K = 5) / 20, which cancels the set-up kernels.
"""
import argparse
import csv
import glob
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from dtc_amd import reset as RS  # noqa: E402
from dtc_amd import synthetic as S  # noqa: E402

DEV = "cuda"
MASKS = (("N/1000", 0.001), ("N/8", 0.125), ("N", 1.0))
ROW_ITEMS = RS.ROW_ITEMS[:-1]


def rand_float(lo, hi, shape):
    return (hi - lo) * torch.rand(*shape, device=DEV) + lo


def torch_reset_idx(e, cfg, extras):
    """reset_idx and its callees as the reference writes them (indexed torch ops on `env_ids = reset_buf.nonzero()`), on a dict."""
    ids = e["reset_buf"].nonzero(as_tuple=False).flatten()
    if len(ids) == 0:
        return
    n = len(ids)
    if cfg.terrain_curriculum and cfg.init_done:
        dist = torch.norm(e["root_states"][ids, :2] - e["env_origins"][ids, :2], dim=1)
        up = dist > cfg.env_length * 0.6
        down = (dist < torch.norm(e["commands"][ids, :2], dim=1) * cfg.max_episode_length_s * 0.5) * ~up
        e["terrain_levels"][ids] += 1 * up - 1 * down
        e["terrain_levels"][ids] = torch.where(e["terrain_levels"][ids] >= cfg.max_terrain_level,
                                               torch.randint_like(e["terrain_levels"][ids], cfg.max_terrain_level),
                                               torch.clip(e["terrain_levels"][ids], 0))
        e["env_origins"][ids] = e["terrain_origins"][e["terrain_levels"][ids], e["terrain_types"][ids]]
    e["dof_pos"][ids] = e["default_dof_pos"] * rand_float(0.5, 1.5, (n, e["dof_pos"].shape[1]))
    e["dof_vel"][ids] = 0.
    e["root_states"][ids] = e["base_init_state"]
    e["root_states"][ids, :3] += e["env_origins"][ids]
    if cfg.custom_origins:
        e["root_states"][ids, :2] += rand_float(cfg.origin_xy[0], cfg.origin_xy[1], (n, 2))
    e["root_states"][ids, 7:13] = rand_float(-0.5, 0.5, (n, 6))
    e["commands"][ids, 0] = rand_float(cfg.lin_vel_x[0], cfg.lin_vel_x[1], (n, 1)).squeeze(1)
    e["commands"][ids, 1] = rand_float(cfg.lin_vel_y[0], cfg.lin_vel_y[1], (n, 1)).squeeze(1)
    if cfg.heading_command:
        e["commands"][ids, 3] = rand_float(cfg.heading[0], cfg.heading[1], (n, 1)).squeeze(1)
    else:
        e["commands"][ids, 2] = rand_float(cfg.ang_vel_yaw[0], cfg.ang_vel_yaw[1], (n, 1)).squeeze(1)
    e["commands"][ids, :2] *= (torch.norm(e["commands"][ids, :2], dim=1) > 0.1).unsqueeze(1)
    e["forces"][ids, :] = torch.zeros((n, e["forces"].shape[1], 3), device=DEV, dtype=torch.float)
    for flag, name, r in ((cfg.randomize_motor_strength, "motor_strengths", cfg.motor_strength), (cfg.randomize_kp, "Kp_factors", cfg.kp_range),
                          (cfg.randomize_kd, "Kd_factors", cfg.kd_range)):
        if flag:
            e[name][ids, :] = torch.rand(n, dtype=torch.float, device=DEV).unsqueeze(1) * (r[1] - r[0]) + r[0]
    e["height_noise_offset"][ids] = e["height_noise_offset"][ids] * 0.0
    e["height_noise_offset"][ids] += np.random.normal(0, 0.02)
    for k in ROW_ITEMS:
        e[k][ids] = 0
    for b in e["lag_buffer"]:
        b[ids, :] = 0
    for b in e["stumb_buffer"]:
        b[ids, :] = 0
    extras["episode"] = {}
    for i, row in enumerate(e["episode_sums_rows"]):
        extras["episode"][i] = torch.mean(row[ids]) / cfg.max_episode_length_s
        row[ids] = 0.
    if cfg.terrain_curriculum:
        extras["episode"]["terrain_level"] = torch.mean(e["terrain_levels"].float())
    for k in RS.TIME_ITEMS:
        e[k][:, ids] = 0.


def make(N, frac, seed=7):
    st = S.reset_state(N, seed=seed, reset="all" if frac >= 1.0 else "none")
    if frac < 1.0:
        k = max(1, round(N * frac))
        st["reset_buf"][torch.randperm(N, generator=torch.Generator().manual_seed(seed))[:k]] = True
    e = {k: [t.to(DEV) for t in v] if isinstance(v, list) else v.to(DEV) for k, v in st.items()}
    for k in ("dof_pos", "dof_vel", "last_actions", "height_noise_offset", "motor_strengths", "feet_air_time", "forces", "root_states",
              "commands", "episode_sums", "cmd_buffer"):
        e[k].nan_to_num_(0.0)                                   # the NaN marker rows of reset_state are of no use here
    e["episode_sums_rows"] = list(e["episode_sums"].unbind(0))
    cfg = RS.ResetConfig()
    E = RS.EnvReset(N, DEV, cfg, n_sums=e["episode_sums"].shape[0])
    kw = {k: v for k, v in e.items() if k not in ("base_init_state", "episode_sums_rows")}
    extras = {}
    return (lambda: torch_reset_idx(e, cfg, extras)), (lambda: E(**kw)), int(e["reset_buf"].sum())


def timed(f):
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


def table(args):
    lines = [f"{'envs':>6} {'mask':>7} {'reset':>6} | {'(a) torch reset_idx us':>23} {'(b) EnvReset us':>16} {'a/b':>6}"]
    for N in args.envs:
        for name, frac in MASKS:
            a, b, count = make(N, frac)
            for _ in range(args.warmup):
                a(), b()
            torch.cuda.synchronize()
            ta, tb = [], []
            for _ in range(args.calls):
                ta.append(timed(a))
                tb.append(timed(b))
            ma, mb = statistics.median(ta), statistics.median(tb)
            lines.append(f"{N:>6} {name:>7} {count:>6} | {ma:>23.1f} {mb:>16.1f} {ma / mb:>6.1f}")
            print(lines[-1], flush=True)
    return lines


def count_child(args):
    name, frac = MASKS[args.count_mask]
    a, b, _ = make(args.envs[0], frac)
    f = a if args.count_side == "a" else b
    for _ in range(args.count_calls):
        f()
    torch.cuda.synchronize()


def kernels_of(d):
    total = 0
    for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as fh:
            total += sum(int(r["Calls"]) for r in csv.DictReader(fh))
    return total


def launches(args):
    lines = [f"{'envs':>6} {'mask':>7} | {'(a) launches / call':>20} {'(b) launches / call':>20}"]
    N = args.envs[0]
    for mi, (name, _) in enumerate(MASKS):
        per = {}
        for side in "ab":
            tot = {}
            for K in (5, 25):
                d = os.path.join(os.path.abspath(args.launches), f"rp_{side}_{mi}_{K}")
                cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "reset", "--output-format", "csv", "--", sys.executable,
                       os.path.abspath(__file__), "--envs", str(N), "--count-side", side, "--count-mask", str(mi), "--count-calls", str(K)]
                r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=240)
                if r.returncode != 0:
                    raise RuntimeError(f"rocprofv3 run failed ({r.returncode}): {r.stderr.decode()[-600:]}")
                tot[K] = kernels_of(d)
            per[side] = (tot[25] - tot[5]) / 20.0
        lines.append(f"{N:>6} {name:>7} | {per['a']:>20.1f} {per['b']:>20.1f}")
        print(lines[-1], flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[4096, 32768])
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default=None, help="write the table(s) to this file as well")
    ap.add_argument("--launches", default=None, metavar="DIR", help="also count kernel launches per call (rocprofv3 child runs, output under DIR)")
    ap.add_argument("--count-side", choices="ab", default=None)
    ap.add_argument("--count-mask", type=int, default=0)
    ap.add_argument("--count-calls", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("reset_probe.py measures on the GPU; none found")
    if args.count_side:
        return count_child(args)
    if args.calls < 200:
        raise SystemExit("--calls must be >= 200")
    out = [f"# reset probe: median of {args.calls} calls per side, alternating, each window ends in a synchronise; {torch.cuda.get_device_name(0)}"]
    out += table(args)
    if args.launches:
        out += ["", "# kernel launches per call (rocprofv3 --kernel-trace --stats, (K = 25) - (K = 5) calls, / 20)"]
        out += launches(args)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
