"""Time LeggedRobot.compute_reward at Lite3DTCCfg scales: a torch-on-GPU restatement of the reference's reward graph
(legged_robot.py:274-291 and the 24 active `_reward_*` terms) against the fused launch (dtc_env_rewards, csrc/rewards.hip).

    python tools/reward_bench.py [--envs 4096 32768] [--reps 50]     # medians of HIP-event timed calls
    python tools/reward_bench.py --launches                          # kernel launches per call, counted by rocprofv3 in child runs

Inputs are dtc_amd.synthetic.reward_state.  One JSON line per (envs, path).
"""
import argparse
import csv
import glob
import itertools
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from dtc_amd import rewards as R  # noqa: E402
from dtc_amd import synthetic as S  # noqa: E402

DT = 0.005 * 4
GOLDEN = os.path.join(os.path.dirname(os.path.dirname(HERE)), "tests", "golden", "rewards.npz")


def lite3_config():
    """Lite3DTCCfg's 24 active terms and fp32 scales * dt, as the reference resolved them (recorded in tests/golden/rewards.npz)."""
    z = np.load(GOLDEN)
    scales = {str(n): float(v) for n, v in zip(z["lite3_names"], z["lite3_scales"])}
    return R.RewardConfig(scales=scales, dt=DT, base_height_target=0.32, max_acc=100.0, lin_vel_x_max=0.75, ang_vel_yaw_max=0.5)


class TorchRewards:
    """The reference's reward graph, op for op, on the GPU (the terms of Lite3DTCCfg)."""

    def __init__(self, d, rc):
        self.__dict__.update(d)
        self.rc, self.N = rc, d["root_states"].shape[0]
        dev = d["root_states"].device
        self.feet_indices = torch.tensor(S.REWARD_FEET, device=dev)
        self.penalised_contact_indices = torch.tensor(S.REWARD_PENALISED, device=dev)
        self.hip_indices = torch.tensor(S.REWARD_HIPS, device=dev)
        self.default_dof_pos = d["default_dof_pos"].unsqueeze(0)
        self.stumb_buffer = [torch.zeros(self.N, 4, dtype=torch.bool, device=dev) for _ in range(5)]
        pts = S.height_points().to(dev)
        self.height_points = pts.unsqueeze(0).repeat(self.N, 1, 1)
        self.gravity_vec = torch.tensor([0.0, 0.0, -1.0], device=dev).repeat(self.N, 1)
        self.rew_buf = torch.zeros(self.N, device=dev)
        self.episode_sums = {n: torch.zeros(self.N, device=dev) for n in rc.names}
        self.acc_point = torch.tensor((torch.tensor(list(itertools.product([-1, 1], repeat=3))) * torch.tensor([0.3, 0.2, 0.15]).double()
                                       / 2.0).tolist(), device=dev).view(1, 8, 3).repeat(self.N, 1, 1)

    def term(self, n):
        dt, fi = DT, self.feet_indices
        cf = self.contact_forces
        if n == "action_rate":
            return torch.sum(torch.square(self.last_actions - self.actions), dim=1)
        if n == "ang_vel_xy":
            return torch.sum(torch.square(self.base_ang_vel[:, :2]), dim=1)
        if n == "base_height":
            return torch.square(self.root_states[:, 2] - torch.mean(self.foot_positions[:, :, 2], dim=-1) - 0.32)
        if n == "collision":
            return torch.sum(1. * (torch.norm(cf[:, self.penalised_contact_indices, :], dim=-1) > 0.1), dim=1)
        if n == "dof_acc":
            return torch.sum(torch.square((self.last_dof_vel - self.dof_vel) / dt), dim=1)
        if n == "dof_pos_limits":
            o = -(self.dof_pos - self.dof_pos_limits[:, 0]).clip(max=0.)
            o += (self.dof_pos - self.dof_pos_limits[:, 1]).clip(min=0.)
            return torch.sum(o, dim=1)
        if n == "feet_air_time":
            contact = cf[:, fi, 2] > 1.
            filt = torch.logical_or(contact, self.last_contacts)
            self.last_contacts = contact
            first = (self.feet_air_time > 0.) * filt
            self.feet_air_time += dt
            r = torch.sum((self.feet_air_time - 0.5) * first, dim=1)
            r *= torch.norm(self.commands[:, :2], dim=1) > 0.1
            self.feet_air_time *= ~filt
            return r
        if n == "feet_slip":
            filt = torch.logical_or(cf[:, fi, 2] > 1., self.last_contacts)
            v = torch.square(torch.norm(self.foot_velocities[:, :, 0:2], dim=2).view(self.N, -1))
            return torch.sum(filt * v, dim=1)
        if n == "foot_acc":
            mask = torch.where(self.terrain_levels > 5, 0.2, 1.)
            a = torch.norm((self.last_foot_velocities - self.foot_velocities) / dt, dim=-1)
            return torch.sum((mask.view(-1, 1) * (a - 100.)).clip(min=0.), dim=1)
        if n == "foot_clearance":
            stumb = torch.norm(cf[:, fi, :2], dim=2) > 4 * torch.abs(cf[:, fi, 2])
            self.stumb_buffer = self.stumb_buffer[1:] + [stumb.clone()]
            b = self.stumb_buffer
            flag = b[0] | b[1] | b[2] | b[3] | b[4]
            return torch.sum(~flag * (self.measured_foot_clearance > 0.18), dim=1)
        if n == "foothold_miss":
            m = torch.min(self.foot_positions[:, :, -1], dim=-1)[0]
            return torch.where(m < 0, 1., 0.)
        if n == "hip_pos":
            return torch.sum(torch.square(self.dof_pos[:, self.hip_indices]), dim=1)
        if n == "lin_vel_z":
            return torch.square(self.base_lin_vel[:, 2])
        if n == "orientation":
            A = self.height_points.clone()
            A[:, :, 2] = 1
            At = A.transpose(1, 2)
            X = torch.bmm(torch.bmm(torch.linalg.inv(torch.bmm(At, A)), At), self.measured_heights.unsqueeze(-1))
            pv = torch.cat([X[:, 0, :], X[:, 1, :], -torch.ones_like(X[:, 1, :])], 1).reshape(-1, 3)
            p = -(pv / torch.norm(pv, dim=-1, keepdim=True))
            pitch, roll = torch.atan(p[:, 0]), -torch.atan(p[:, 1])
            zero = torch.tensor(0., device=p.device)
            pc = torch.where((pitch >= -0.1) & (pitch <= 0.1), zero, pitch)
            rc = torch.where((roll >= -0.1) & (roll <= 0.1), zero, roll)
            self.pitch_est = self.pitch_est.clone() * 0.2 + 0.8 * pc
            cr, sr, cp, sp = torch.cos(rc * 0.5), torch.sin(rc * 0.5), torch.cos(self.pitch_est * 0.5), torch.sin(self.pitch_est * 0.5)
            q = torch.stack([sr * cp, cr * sp, -sr * sp, cr * cp], dim=-1)
            w, qv, v = q[:, -1], q[:, :3], self.gravity_vec
            loc = v * (2.0 * w ** 2 - 1.0).unsqueeze(-1) - torch.cross(qv, v, dim=-1) * w.unsqueeze(-1) * 2.0 + \
                qv * torch.bmm(qv.view(self.N, 1, 3), v.view(self.N, 3, 1)).squeeze(-1) * 2.0
            return torch.sum(torch.square(self.projected_gravity[:, :1] - loc[:, :1]), dim=1)
        if n == "pos_acc":
            v = self.base_lin_vel.reshape(self.N, 1, 3).repeat(1, 8, 1) + \
                torch.cross(self.base_ang_vel.reshape(self.N, 1, 3).repeat(1, 8, 1), self.acc_point, dim=-1)
            return torch.sum(torch.square(torch.norm(v, dim=-1)), dim=1)
        if n == "power":
            return torch.sum(torch.clip(self.torques * self.dof_vel, min=0), dim=1)
        if n == "powerchange":
            co = self.commands[:, 0].clone().clip(min=1.0)
            return (torch.sum((self.torques * self.dof_vel).clip(min=0.0), dim=1) / (self.robot_mass * 9.815 * co)) ** 2
        if n == "smooth":
            return torch.sum(torch.square(self.actions - 2 * self.last_actions + self.last_actions_2), dim=1)
        if n == "soft_tracking_ang_vel":
            d = torch.square((self.cmd_buffer[-4:, :, 2] - self.ang_vel_buffer[-4:, :].squeeze(-1)) / 0.5)
            d = torch.where(d <= 0.15 ** 2, 0., 1.)
            return torch.mean(torch.exp(-d / 0.25), dim=0)
        if n == "soft_tracking_lin_vel":
            d = torch.sum(torch.square((self.cmd_buffer[-3:, :, :2] - self.lin_vel_buffer[-3, :, :2]) / 0.75), dim=-1)
            return torch.mean(torch.exp(-d / 0.25), dim=0)
        if n == "stand_still":
            return torch.sum(torch.abs(self.dof_pos - self.default_dof_pos), dim=1) * (torch.norm(self.commands[:, :2], dim=1) < 0.1)
        if n == "termination":
            return self.reset_buf * ~self.time_out_buf
        if n == "torques":
            return torch.sum(torch.square(self.torques), dim=1)
        if n == "tracking_optimal_footholds":
            dis = torch.norm(self.foot_positions[:, :, :-1] - self.optimal_footholds_world[:, :, :-1], dim=-1)
            r = -torch.log(0.8 + dis)
            return torch.sum(torch.where(self.contact_filt.float() == 1, r, torch.tensor(0., device=r.device)), dim=-1)
        raise KeyError(n)

    def compute_reward(self):
        self.rew_buf[:] = 0.
        for n, s in self.rc.scales.items():
            if n == "termination":
                continue
            r = self.term(n) * s
            self.rew_buf += r
            self.episode_sums[n] += r
        if self.rc.only_positive_rewards:
            self.rew_buf[:] = torch.clip(self.rew_buf[:], min=0.)
        if "termination" in self.rc.scales:
            r = self.term("termination") * self.rc.scales["termination"]
            self.rew_buf += r
            self.episode_sums["termination"] += r


def setup(N, path):
    rc = lite3_config()
    d = {k: v.cuda() for k, v in S.reward_state(N, seed=3).items()}
    if path == "torch":
        env = TorchRewards(d, rc)
        return env.compute_reward
    E = R.EnvRewards(N, "cuda", rc, feet_indices=S.REWARD_FEET, penalised_contact_indices=S.REWARD_PENALISED, hip_indices=S.REWARD_HIPS)
    inp = {k: v for k, v in d.items() if k in R._shapes(1, 1, 1, 1, 1)}
    lc = d["last_contacts"]
    return lambda: E(last_contacts=lc, **inp)


def time_path(N, path, reps, warmup=5):
    fn = setup(N, path)
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1000.0)
    ts.sort()
    return ts[len(ts) // 2]


def count_launches(N, path, calls):
    """Kernel launches of `calls` calls in a child run under rocprofv3 --kernel-trace --stats (setup counted apart)."""
    totals = []
    for k in (0, calls):
        with tempfile.TemporaryDirectory() as d:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "run", "--output-format", "csv", "--",
                   sys.executable, os.path.abspath(__file__), "--child", path, "--envs", str(N), "--reps", str(k)]
            subprocess.run(cmd, check=True, capture_output=True, timeout=600)
            f = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
            totals.append(sum(int(row["Calls"]) for row in csv.DictReader(open(f[0]))))
    return (totals[1] - totals[0]) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[4096, 32768])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--launches", action="store_true")
    ap.add_argument("--child", choices=["torch", "fused"])
    a = ap.parse_args()
    if a.child:
        fn = setup(a.envs[0], a.child)
        torch.cuda.synchronize()
        for _ in range(a.reps):
            fn()
        torch.cuda.synchronize()
        return
    for N in a.envs:
        for path in ("torch", "fused"):
            if a.launches:
                print(json.dumps(dict(envs=N, path=path, launches_per_call=count_launches(N, path, 10))), flush=True)
            else:
                print(json.dumps(dict(envs=N, path=path, median_us=round(time_path(N, path, max(a.reps, 20)), 1))), flush=True)


if __name__ == "__main__":
    main()
