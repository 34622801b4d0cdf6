"""GPU: dtc_env_reset (csrc/reset.hip) through dtc_amd.reset against the numpy oracle (tests/golden/reset_oracle.py) and the
reference-captured tests/golden/reset.npz: teacher-forced draws, generated draws, block edges, determinism, no host
synchronisation, patch_env in a rewards -> reset -> observations sequence, argument validation."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import reset_oracle as O  # noqa: E402
from dtc_amd import _ffi, reset as RS  # noqa: E402
from dtc_amd import synthetic as S  # noqa: E402
from test_reset_oracle import TAGS, case_inputs, check_against_fixture, oracle_cfg, ulp_diff  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
D = 12
SKIP = ("base_init_state",)                 # a config value, not an env tensor


@pytest.fixture(scope="module")
def fx(golden):
    return golden("reset")


def reset_config(cfg: dict, base_init) -> RS.ResetConfig:
    keys = ("terrain_curriculum", "init_done", "custom_origins", "heading_command", "play_command", "randomize_motor_strength",
            "randomize_kp", "randomize_kd", "max_terrain_level", "env_length", "max_episode_length_s", "origin_xy", "lin_vel_x",
            "lin_vel_y", "ang_vel_yaw", "heading", "motor_strength", "kp_range", "kd_range")
    return RS.ResetConfig(base_init_state=tuple(float(v) for v in base_init), **{k: cfg[k] for k in keys})


def to_dev(state: dict) -> dict:
    mv = lambda t: t.to(DEV).contiguous()          # noqa: E731
    return {k: [mv(t) for t in v] if isinstance(v, list) else mv(v) for k, v in state.items() if k not in SKIP}


def to_np(dev: dict) -> dict:
    cv = lambda t: t.cpu().numpy()          # noqa: E731
    return {k: [cv(t) for t in v] if isinstance(v, list) else cv(v) for k, v in dev.items()}


def leaves(d: dict):
    for k in sorted(d):
        if k in SKIP:
            continue
        v = d[k]
        for j, a in enumerate(v if isinstance(v, list) else [v]):
            yield (f"{k}[{j}]" if isinstance(v, list) else k), a


def same_bits(a, b, msg):
    np.testing.assert_array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8), err_msg=msg)


def call(E, dev, u=None, lv=None, s=None):
    kw = dict(dev)
    if u is not None:
        kw["u"] = torch.as_tensor(u).to(DEV)
    if lv is not None:
        kw["level_draw"] = torch.as_tensor(lv).to(DEV)
    ids, count, means, tlm = E(height_noise=s, **kw)
    n = int(count.item())
    return dict(env_ids=ids[:n].cpu().numpy(), count=n, episode_means=means.cpu().numpy().copy(),
                terrain_level_mean=tlm.cpu().numpy().copy()[0])


def run_case(state, cfg, u, lv, s, E=None):
    """One call on the device and the oracle on the same inputs.  Returns (device env as numpy, device results, oracle env, oracle
    results, inputs as numpy)."""
    E = E or RS.EnvReset(state["reset_buf"].shape[0], DEV, reset_config(cfg, state["base_init_state"]),
                         n_sums=state["episode_sums"].shape[0])
    dev = to_dev(state)
    got = call(E, dev, u, lv, s)
    ref_env = O.np_state(state)
    ref = O.reset_idx(ref_env, cfg, u, lv, s)
    return to_np(dev), got, ref_env, ref, O.np_state(state)


def check_against_oracle(env, got, ref_env, ref, before, cfg, what):
    np.testing.assert_array_equal(got["env_ids"], ref["env_ids"], err_msg=f"{what} env_ids")
    assert got["count"] == ref["count"] == int(before["reset_buf"].sum())
    keep = ~before["reset_buf"].astype(bool)
    for (k, a), (_, r), (_, b) in zip(leaves(env), leaves(ref_env), leaves(before)):
        assert a.dtype == r.dtype and a.shape == r.shape, (what, k)
        np.testing.assert_array_equal(a, r, err_msg=f"{what} {k}")           # values: -0.0 == 0.0, NaN == NaN
        if k in ("terrain_origins", "default_dof_pos"):           # no env axis: read only
            same_bits(a, b, f"{what} {k}")
        elif k.split("[")[0] in O.TIME_ITEMS or k == "episode_sums":
            same_bits(a[:, keep], b[:, keep], f"{what} untouched rows of {k}")
        else:
            same_bits(a[keep], b[keep], f"{what} untouched rows of {k}")
    if ref["count"]:
        d = ulp_diff(got["episode_means"], ref["episode_means"])
        assert d.max() <= 1, (what, "episode means", d.max())
        if cfg["terrain_curriculum"]:
            assert ulp_diff(got["terrain_level_mean"], ref["terrain_level_mean"]).max() <= 1, what


@pytest.mark.parametrize("tag", TAGS)
def test_fixture_cases_teacher_forced(fx, tag):
    state, cfg, u, lv, s = case_inputs(fx, tag)
    env, got, ref_env, ref, before = run_case(state, cfg, u, lv, s)
    check_against_oracle(env, got, ref_env, ref, before, cfg, tag)
    # and against the reference's own outputs
    res = dict(ref)
    res.update(env_ids=got["env_ids"], count=got["count"])
    check_against_fixture(fx, tag, env, res, "kernel")
    if got["count"]:
        r = fx[f"{tag}_episode_means"].astype(np.float64)
        assert (np.abs(got["episode_means"] - r) / np.maximum(np.abs(r), 1e-30)).max() <= 1e-5


def test_no_env_reset_changes_nothing(fx):
    state, cfg, u, lv, s = case_inputs(fx, "none")
    E = RS.EnvReset(state["reset_buf"].shape[0], DEV, reset_config(cfg, state["base_init_state"]), n_sums=state["episode_sums"].shape[0])
    E.episode_means.copy_(torch.linspace(1, 2, E.n_sums))
    E.terrain_level_mean.fill_(7.25)
    E.env_ids.fill_(-3)
    E.count.fill_(99)
    means0 = E.episode_means.cpu().numpy().copy()
    dev = to_dev(state)
    got = call(E, dev, u, lv, s)
    assert got["count"] == 0 and int(E.count.item()) == 0
    for (k, a), (_, b) in zip(leaves(to_np(dev)), leaves(O.np_state(state))):
        same_bits(a, b, k)
    same_bits(got["episode_means"], means0, "episode means")
    assert got["terrain_level_mean"] == np.float32(7.25) and bool((E.env_ids == -3).all())


@pytest.mark.parametrize("N,mode", [(1, "all"), (255, "some"), (256, "some"), (257, "some"), (4096, "some"), (32768, "some")])
def test_block_edges_and_sizes(fx, N, mode):
    state, cfg, u, lv, s = case_inputs(fx, "lite3", N=N, seed=2000 + N, mode=mode)
    if N >= 255:                                   # the envs either side of a 256-env block edge reset
        for n in (0, 254, 255, 256, N - 1):
            if n < N:
                state["reset_buf"][n] = True
    env, got, ref_env, ref, before = run_case(state, cfg, u, lv, s)
    check_against_oracle(env, got, ref_env, ref, before, cfg, f"N={N}")
    np.testing.assert_array_equal(got["env_ids"], np.nonzero(before["reset_buf"])[0])


def test_two_calls_same_bits(fx):
    state, cfg, u, lv, s = case_inputs(fx, "x30", N=4099, seed=77, mode="some")
    a = run_case(state, cfg, u, lv, s)
    b = run_case(state, cfg, u, lv, s)
    for (k, x), (_, y) in zip(leaves(a[0]), leaves(b[0])):
        same_bits(x, y, k)
    same_bits(a[1]["episode_means"], b[1]["episode_means"], "means")
    same_bits(a[1]["terrain_level_mean"], b[1]["terrain_level_mean"], "terrain level mean")
    same_bits(a[1]["env_ids"], b[1]["env_ids"], "env_ids")


def _generated(fx, N, mode, seed, state_seed=3000):
    state, cfg, _, _, s = case_inputs(fx, "lite3", N=N, seed=state_seed, mode=mode)
    cfg = dict(cfg, randomize_kp=True, randomize_kd=True)
    E = RS.EnvReset(N, DEV, reset_config(cfg, state["base_init_state"]), n_sums=state["episode_sums"].shape[0], seed=seed)
    dev = to_dev(state)
    got = call(E, dev, None, None, s)
    return to_np(dev), got, O.np_state(state), cfg


def test_generated_draws(fx):
    N = 32768
    env, got, before, cfg = _generated(fx, N, "all", seed=11)
    assert got["count"] == N
    base = before["base_init_state"]
    org = env["env_origins"]
    dflt = before["default_dof_pos"]
    # every written value inside its range; (name, values [N], lo, hi) per draw slot
    slots = [(f"dof_pos[{j}]", env["dof_pos"][:, j], min(0.5 * dflt[j], 1.5 * dflt[j]), max(0.5 * dflt[j], 1.5 * dflt[j])) for j in range(D)]
    slots += [(f"origin[{j}]", env["root_states"][:, j].astype(np.float64) - (np.float32(base[j]) + org[:, j]), -0.5, 0.5) for j in range(2)]
    slots += [(f"root_states[{j}]", env["root_states"][:, j], -0.5, 0.5) for j in range(7, 13)]
    slots += [("commands[0]", env["commands"][:, 0], -0.75, 0.75), ("commands[1]", env["commands"][:, 1], -0.75, 0.75),
              ("commands[3]", env["commands"][:, 3], -3.14, 3.14), ("motor_strengths", env["motor_strengths"][:, 0], 0.9, 1.1),
              ("Kp_factors", env["Kp_factors"][:, 0], 0.95, 1.05), ("Kd_factors", env["Kd_factors"][:, 0], 0.95, 1.05)]
    for name, v, lo, hi in slots:
        v = np.asarray(v, dtype=np.float64)
        eps = 1e-5 if name.startswith("origin") else 1e-6            # fp32 rounding; origin: recovered through an addition at ~50 m
        assert v.min() >= lo - eps and v.max() <= hi + eps, (name, v.min(), v.max())
        se = (hi - lo) / np.sqrt(12.0 * N)
        assert abs(v.mean() - 0.5 * (lo + hi)) <= 5 * se, (name, v.mean(), se)
    assert env["terrain_levels"].min() >= 0 and env["terrain_levels"].max() < cfg["max_terrain_level"]
    for k in ("motor_strengths", "Kp_factors", "Kd_factors"):
        assert (env[k] == env[k][:, :1]).all()                    # one draw per env, broadcast over the dofs
    # same (seed, counter) -> same bits; another seed -> other draws
    again, _, _, _ = _generated(fx, N, "all", seed=11)
    for (k, x), (_, y) in zip(leaves(env), leaves(again)):
        same_bits(x, y, k)
    other, _, _, _ = _generated(fx, N, "all", seed=12)
    assert not np.array_equal(env["dof_pos"], other["dof_pos"])
    # another reset mask leaves everything drawn for the envs common to both unchanged (the level draw included)
    a, ga, _, _ = _generated(fx, 4096, "all", seed=5)
    b, gb, bb, _ = _generated(fx, 4096, "some", seed=5)
    common = bb["reset_buf"].astype(bool)
    assert 0 < gb["count"] < ga["count"]
    for k in ("dof_pos", "root_states", "commands", "motor_strengths", "Kp_factors", "Kd_factors", "terrain_levels", "env_origins"):
        same_bits(a[k][common], b[k][common], k)


def test_call_does_not_synchronise_the_host(fx):
    """The call runs under torch.cuda.set_sync_debug_mode("error"): any synchronising torch call inside it raises.  The mode is
    probed first (`.item()` must raise under it); the installed torch is expected to honour it on ROCm."""
    state, cfg, u, lv, s = case_inputs(fx, "lite3")
    E = RS.EnvReset(state["reset_buf"].shape[0], DEV, reset_config(cfg, state["base_init_state"]), n_sums=state["episode_sums"].shape[0])
    dev = to_dev(state)
    ud, lvd = torch.as_tensor(u).to(DEV), torch.as_tensor(lv).to(DEV)
    probe = torch.ones(1, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        honoured = False
        try:
            probe.item()
        except RuntimeError:
            honoured = True
        E(height_noise=s, u=ud, level_draw=lvd, **dev)
        E(height_noise=None, **dev)                               # generated draws, host-drawn height noise
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert honoured, "torch.cuda.set_sync_debug_mode('error') did not flag .item(): the no-synchronisation check is void"


# ---------------------------------------------------------------------------------------------------------------- patch_env
def _reward_fixture_cfg(golden):
    from test_reward_oracle import cfg_from_fixture
    base = cfg_from_fixture(golden("rewards"), "lite3")
    ns = lambda **k: type("ns", (), k)          # noqa: E731
    base.terrain = ns(mesh_type="trimesh", curriculum=True, num_rows=6, num_cols=2, terrain_length=8.0,
                      measured_points_x=S.MEASURED_POINTS_X, measured_points_y=S.MEASURED_POINTS_Y)
    base.commands = ns(ranges=ns(lin_vel_x=[-0.75, 0.75], lin_vel_y=[-0.75, 0.75], ang_vel_yaw=[-0.5, 0.5], heading=[-3.14, 3.14]),
                       heading_command=True, curriculum=False, max_curriculum=1.0)
    base.domain_rand = ns(randomize_motor_strength=True, randomize_Kp_factor=False, randomize_Kd_factor=False, motor_strength=[0.9, 1.1],
                          kp_range=[0.95, 1.05], kd_range=[0.95, 1.05])
    base.env = ns(play_commond=False, episode_length_s=20, send_timeouts=True)
    base.init_state = ns(pos=[0.0, 0.0, 0.4], rot=[0.0, 0.0, 0.0, 1.0], lin_vel=[0.0, 0.0, 0.0], ang_vel=[0.0, 0.0, 0.0])
    return base


class _MockEnv:
    """The attributes of LeggedRobotDTC that compute_reward, reset_idx and compute_observations touch, on the device."""

    def __init__(self, cfg, N):
        self.cfg, self.num_envs, self.device, self.num_dof = cfg, N, DEV, D
        self.feet_indices = torch.tensor(S.REWARD_FEET, device=DEV)
        self.penalised_contact_indices = torch.tensor(S.REWARD_PENALISED, device=DEV)
        self.hip_indices = torch.tensor(S.REWARD_HIPS, device=DEV)
        self.command_ranges = {k: list(getattr(cfg.commands.ranges, k)) for k in ("lin_vel_x", "lin_vel_y", "ang_vel_yaw", "heading")}
        self.rew_buf = torch.zeros(N, device=DEV)
        self.extras, self.init_done, self.custom_origins = {}, True, True
        self.owned = {"episode_sums"}              # attributes a patch has taken over: not reloaded from the driver's env

    def reset_idx(self, env_ids):
        raise AssertionError("the env's own reset_idx must have been replaced by reset.patch_env")

    def load(self, env, only=None):
        for k, v in env.items():
            if (only is not None and k not in only) or k in self.owned:
                continue
            if isinstance(v, list):
                setattr(self, k, [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in v])
                continue
            t = torch.from_numpy(np.ascontiguousarray(v)).to(DEV)
            setattr(self, k, t.unsqueeze(0) if k == "default_dof_pos" else t)
        if only is None or "dof_pos" in only:
            # legged_robot.py:772-775: dof_pos / dof_vel are the two interleaved views of dof_state, the tensor the simulator takes
            self.dof_state = torch.stack([self.dof_pos, self.dof_vel], dim=-1).reshape(self.num_envs * D, 2).contiguous()
            self.dof_pos = self.dof_state.view(self.num_envs, D, 2)[..., 0]
            self.dof_vel = self.dof_state.view(self.num_envs, D, 2)[..., 1]


def _merged_state(N, seed):
    """reward_state + the tensors only reset_idx touches + the observation inputs, as numpy (the env of the sequence)."""
    import reward_oracle as RO
    env = RO.seq_begin(S.reward_state(N, seed=seed), list(S.REWARD_FEET))
    extra = O.np_state(S.reset_state(N, seed=seed + 1))
    for k, v in extra.items():
        if k not in env and k not in ("episode_sums", "stumb_buffer"):
            env[k] = v
    obs = S.env_state(N, seed=seed + 2)
    for k in ("foothold_obs", "u_obs", "u_heights", "noise_scale_vec"):
        env[k] = obs[k].numpy().copy()
    return env


@pytest.mark.parametrize("with_rewards", [True, False])
def test_patch_env_sequence(golden, with_rewards):
    """Three consecutive steps of compute_reward -> reset_idx -> compute_observations(where = reset_buf) on a patched mock env equal
    the oracle sequence; extras["episode"] holds the oracle's means as device views."""
    import reward_oracle as RO
    from dtc_amd import foothold, rewards as RW
    from oracle import observations as OO
    from test_reward_oracle import oracle_cfg as reward_oracle_cfg
    N, F = 1024, list(S.REWARD_FEET)
    cfg = _reward_fixture_cfg(golden)
    rc = RW.RewardConfig.from_cfg(cfg)
    names = rc.names
    rcfg = reward_oracle_cfg(rc)
    ocfg = O.config()
    env = _merged_state(N, 4000)
    env["stumb_buffer"] = [((env["stumble"] >> (4 - i)) & 1).astype(bool) for i in range(5)]
    m = _MockEnv(cfg, N)
    m.load(env)
    m.episode_sums = {n: torch.zeros(N, device=DEV) for n in names}
    Rw = RW.patch_env(m) if with_rewards else None
    if with_rewards:
        m.owned |= {"feet_air_time", "pitch_est"}
    E = RS.patch_env(m)
    assert (E.n_sums == len(names)) and (Rw is None or m.env_rewards is Rw)
    sums = {n: np.zeros(N) for n in names}
    obs_keys = ("base_ang_vel", "projected_gravity", "commands", "dof_pos", "default_dof_pos", "dof_vel", "actions", "foothold_obs",
                "root_states", "measured_heights", "forces", "height_noise_offset", "u_obs", "noise_scale_vec", "u_heights")
    for t in range(3):
        # rewards: on the device when patched, and always in the oracle (the driver's env then follows the device's sums / state)
        RO.compute_reward(env, rcfg, env, sums)
        if with_rewards:
            m.compute_reward()
            env["feet_air_time"], env["pitch_est"] = m.feet_air_time.cpu().numpy(), m.pitch_est.cpu().numpy()
            env["stumble"], env["last_contacts"] = Rw.stumble.cpu().numpy(), m.last_contacts.cpu().numpy().astype(bool)
            env["episode_sums"] = Rw.episode_sums.cpu().numpy()
        else:
            env["episode_sums"] = np.stack([sums[n] for n in names]).astype(np.float32)
            for i, n in enumerate(names):
                m.episode_sums[n].copy_(torch.from_numpy(env["episode_sums"][i]))
            m.load(env, only=("feet_air_time", "pitch_est", "last_contacts"))
            env["stumb_buffer"] = [((env["stumble"] >> (4 - i)) & 1).astype(bool) for i in range(5)]
            m.load(env, only=("stumb_buffer",))
        # the observation rows of the pre-reset state (what dtc_env_post_physics leaves), then the reset and the refresh
        dev_obs = lambda: [getattr(m, k) for k in obs_keys]          # noqa: E731
        got = foothold.compute_observations(*dev_obs())
        u, lv = S.reset_draws(N, seed=4100 + t)
        s = 0.01 * (t + 1)
        m.reset_idx(None, u=u.to(DEV), level_draw=lv.to(DEV), height_noise=s)
        foothold.compute_observations(*dev_obs(), where=m.reset_buf, out=got)
        ref = O.reset_idx(env, ocfg, u.numpy(), lv.numpy(), s)
        assert ref["count"] > 0
        # every env tensor the reset touches
        for k in ("root_states", "env_origins", "commands", "dof_pos", "dof_vel", "terrain_levels", "forces", "motor_strengths",
                  "height_noise_offset") + O.ROW_ITEMS + O.TIME_ITEMS:
            np.testing.assert_array_equal(getattr(m, k).cpu().numpy(), env[k], err_msg=f"step {t} {k}")
        assert not m.dof_pos.is_contiguous() and m.dof_pos.data_ptr() == m.dof_state.data_ptr()
        np.testing.assert_array_equal(m.dof_state.cpu().numpy().reshape(N, D, 2), np.stack([env["dof_pos"], env["dof_vel"]], axis=-1),
                                      err_msg=f"step {t} dof_state")
        for j, b in enumerate(m.lag_buffer):
            np.testing.assert_array_equal(b.cpu().numpy(), env["lag_buffer"][j], err_msg=f"step {t} lag_buffer[{j}]")
        if with_rewards:
            np.testing.assert_array_equal(Rw.stumble.cpu().numpy(), env["stumble"])
        else:
            for j, b in enumerate(m.stumb_buffer):
                np.testing.assert_array_equal(b.cpu().numpy(), env["stumb_buffer"][j])
            env["stumble"][ref["env_ids"]] = 0
        np.testing.assert_array_equal(np.stack([m.episode_sums[n].cpu().numpy() for n in names]), env["episode_sums"])
        np.testing.assert_array_equal(E.env_ids[:ref["count"]].cpu().numpy(), ref["env_ids"])
        # extras["episode"]: device views of the oracle's means
        ep = m.extras["episode"]
        assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in ep.values())
        means = np.array([ep["rew_" + n].item() for n in names], dtype=np.float32)
        assert ulp_diff(means, ref["episode_means"]).max() <= 1
        assert ulp_diff(np.float32(ep["terrain_level"].item()), ref["terrain_level_mean"]).max() <= 1
        assert m.extras["time_outs"] is m.time_out_buf
        # observations: all rows equal the oracle's pass over the post-reset state
        o_ref, p_ref, h_ref = OO.compute_observations({k: env[k] for k in obs_keys})
        np.testing.assert_array_equal(got["obs_buf"].cpu().numpy(), o_ref)
        np.testing.assert_array_equal(got["privileged_obs_buf"].cpu().numpy(), p_ref)
        np.testing.assert_array_equal(got["heights"].cpu().numpy(), h_ref)
        # the oracle's sums follow the zeroed rows; next step's fresh quantities
        for i, n in enumerate(names):
            sums[n] = env["episode_sums"][i].astype(np.float64)
        keep = {k: env[k] for k in env if k not in S.reward_state(1, seed=0)}
        carried = {k: env[k] for k in ("root_states", "commands", "dof_pos", "dof_vel", "terrain_levels")}
        RO.seq_next(env, S.reward_state(N, seed=4001 + t), F)
        env.update(keep)
        env.update(carried)                       # the reset state stays (the mock has no physics), only the reset flags are new
        m.load(env)


def test_dof_state_views_and_other_layouts(fx):
    """dof_pos / dof_vel as the reference holds them -- dof_state.view(N, D, 2)[..., 0] / [..., 1] (legged_robot.py:774-775) -- are
    written through their strides: dof_state holds the oracle's values afterwards, its untouched rows keep their bits.  Two other
    layouts of the same call: a height_noise_offset wider than the register path of the kernel (800 > 768 columns) and a reset_buf
    that starts at an odd address (the byte-wise head of the flag count)."""
    N = 1500
    state, cfg, u, lv, s = case_inputs(fx, "lite3", N=N, seed=5100, mode="some")
    state["height_noise_offset"] = torch.cat([state["height_noise_offset"], state["height_noise_offset"][:, :107] + 0.5], dim=1).contiguous()
    assert state["height_noise_offset"].shape == (N, 800)
    dev = to_dev(state)
    dof_state = torch.stack([dev["dof_pos"], dev["dof_vel"]], dim=-1).reshape(N * D, 2).contiguous()
    before_state = dof_state.cpu().numpy().copy()
    dev["dof_pos"], dev["dof_vel"] = dof_state.view(N, D, 2)[..., 0], dof_state.view(N, D, 2)[..., 1]
    big = torch.zeros(N + 8, dtype=torch.bool, device=DEV)
    big[1:N + 1] = dev["reset_buf"]
    dev["reset_buf"] = big[1:N + 1]
    assert dev["reset_buf"].data_ptr() % 4 == 1 and dev["reset_buf"].is_contiguous() and not dev["dof_vel"].is_contiguous()
    E = RS.EnvReset(N, DEV, reset_config(cfg, state["base_init_state"]), n_sums=state["episode_sums"].shape[0])
    got = call(E, dev, u, lv, s)
    ref_env = O.np_state(state)
    ref = O.reset_idx(ref_env, cfg, u, lv, s)
    env = to_np({k: (v.contiguous() if k in ("dof_pos", "dof_vel", "reset_buf") else v) for k, v in dev.items()})
    check_against_oracle(env, got, ref_env, ref, O.np_state(state), cfg, "dof_state views")
    after = dof_state.cpu().numpy().reshape(N, D, 2)
    np.testing.assert_array_equal(after, np.stack([ref_env["dof_pos"], ref_env["dof_vel"]], axis=-1))
    keep = ~state["reset_buf"].numpy()
    same_bits(after[keep], before_state.reshape(N, D, 2)[keep], "untouched rows of dof_state")
    assert not bool(big[0]) and not bool(big[N + 1:].any())


def test_per_call_arguments_leave_the_config_alone(fx):
    state, cfg, u, lv, s = case_inputs(fx, "lite3", N=512, seed=5200, mode="some")
    rc = reset_config(cfg, state["base_init_state"])
    frozen = RS.ResetConfig(**vars(rc))
    E = RS.EnvReset(512, DEV, rc, n_sums=state["episode_sums"].shape[0])
    dev = to_dev(state)
    wide = dict(lin_vel_x=[-2.0, 2.0], lin_vel_y=[-1.5, 1.5], heading=[-1.0, 1.0])
    E(height_noise=s, command_ranges=wide, init_done=False, u=torch.as_tensor(u).to(DEV), level_draw=torch.as_tensor(lv).to(DEV), **dev)
    assert rc == frozen and E.cfg is rc
    ref_env = O.np_state(state)
    O.reset_idx(ref_env, dict(cfg, init_done=False, **{k: tuple(v) for k, v in wide.items()}), u, lv, s)
    for k in ("commands", "terrain_levels", "env_origins", "root_states"):
        np.testing.assert_array_equal(dev[k].cpu().numpy(), ref_env[k], err_msg=k)


def test_command_curriculum_follows_the_reference_early_return(golden):
    """update_command_curriculum in the patched reset_idx: nothing happens on a call in which no env reset (legged_robot.py:210-211),
    whatever mean an earlier reset left behind; with resets and a mean above 0.8 of the scale the range widens by 0.5."""
    N = 512
    cfg = _reward_fixture_cfg(golden)
    cfg.commands.curriculum = True
    env = _merged_state(N, 5300)
    env["stumb_buffer"] = [((env["stumble"] >> (4 - i)) & 1).astype(bool) for i in range(5)]
    m = _MockEnv(cfg, N)
    m.load(env)
    names = ["tracking_lin_vel", "torques"]
    m.episode_sums = {n: torch.full((N,), 30.0, device=DEV) for n in names}
    m.reward_scales = {"tracking_lin_vel": 0.02, "torques": -1e-5}
    m.common_step_counter, m.max_episode_length = 0, 1000.0
    E = RS.patch_env(m)
    E.episode_means.fill_(100.0)                              # a stale mean of some earlier reset
    m.reset_buf.zero_()
    m.reset_idx(None)
    assert m.command_ranges["lin_vel_x"] == [-0.75, 0.75] and int(E.count.item()) == 0
    m.reset_buf[::7] = True
    m.reset_idx(None)                                         # mean 30 -> 30 / 1000 > 0.8 * 0.02
    assert m.command_ranges["lin_vel_x"] == [-1.0, 1.0] and m.extras["episode"]["max_command_x"] == 0.75
    m.common_step_counter = 1                                 # not the curriculum's step: no read, no change
    m.reset_idx(None)
    assert m.command_ranges["lin_vel_x"] == [-1.0, 1.0]


# ------------------------------------------------------------------------------------------------------- argument validation
def test_argument_validation(fx):
    state, cfg, u, lv, s = case_inputs(fx, "lite3", N=512, seed=9, mode="some")
    E = RS.EnvReset(512, DEV, reset_config(cfg, state["base_init_state"]), n_sums=state["episode_sums"].shape[0])
    dev = to_dev(state)
    ok = lambda **k: E(height_noise=s, **{**dev, **k})          # noqa: E731
    with pytest.raises(ValueError, match="shape"):
        ok(dof_pos=dev["dof_pos"][:, :11].contiguous())
    with pytest.raises(ValueError, match="shape"):
        ok(episode_sums=dev["episode_sums"][:5].contiguous())
    with pytest.raises(ValueError, match="float64|expected"):
        ok(root_states=dev["root_states"].double())
    with pytest.raises(ValueError, match="int32|expected"):
        ok(terrain_levels=dev["terrain_levels"].int())
    with pytest.raises(ValueError, match="is on"):
        ok(commands=dev["commands"].cpu())
    with pytest.raises(ValueError, match="strides"):
        ok(dof_vel=torch.zeros(D, 512, device=DEV).t())
    with pytest.raises(ValueError, match="strides"):
        ok(dof_pos=torch.zeros(1, D, device=DEV).expand(512, D))
    with pytest.raises(ValueError, match="contiguous"):
        ok(root_states=torch.zeros(512, 26, device=DEV)[:, ::2])
    with pytest.raises(ValueError, match="contiguous"):
        ok(last_actions=torch.zeros(D, 512, device=DEV).t())
    with pytest.raises(ValueError, match="envs on axis"):
        ok(cmd_buffer=torch.zeros(10, 100, 4, device=DEV))
    with pytest.raises(ValueError, match="unknown input"):
        ok(torques=dev["dof_vel"])
    with pytest.raises(ValueError, match="required"):
        ok(root_states=None)
    with pytest.raises(ValueError, match="row items"):
        ok(extra_rows=[torch.zeros(512, 4, device=DEV) for _ in range(_ffi.RESET_MAX_ROWS)])
    with pytest.raises(ValueError, match="time-major"):
        ok(extra_time_rows=[torch.zeros(10, 512, 2, device=DEV) for _ in range(_ffi.RESET_MAX_TIME_ROWS)])
    with pytest.raises(ValueError):
        RS.EnvReset(512, DEV, E.cfg, n_sums=_ffi.RESET_MAX_SUMS + 1)
    # nothing above launched anything: the state is still the input
    for (k, a), (_, b) in zip(leaves(to_np(dev)), leaves(O.np_state(state))):
        same_bits(a, b, k)
    # extra items are cleared like the named ones
    extra, extra_t = torch.ones(512, 5, dtype=torch.uint8, device=DEV), torch.ones(3, 512, 6, dtype=torch.float16, device=DEV)
    ok(extra_rows=[extra], extra_time_rows=[extra_t])
    flag = state["reset_buf"].to(DEV)
    assert bool((extra[flag] == 0).all()) and bool((extra[~flag] == 1).all())
    assert bool((extra_t[:, flag] == 0).all()) and bool((extra_t[:, ~flag] == 1).all())
