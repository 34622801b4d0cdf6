"""GPU: dtc_env_rewards (csrc/rewards.hip) through dtc_amd.rewards against the float64 oracle (tests/golden/reward_oracle.py) on
dtc_amd.synthetic.reward_state inputs, and rewards.patch_env against the reference-captured tests/golden/rewards.npz."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import reward_oracle as O  # noqa: E402
from dtc_amd import rewards as R  # noqa: E402
from dtc_amd import synthetic as S  # noqa: E402
from test_reward_oracle import TAGS, cfg_from_fixture, oracle_cfg  # noqa: E402

pytestmark = pytest.mark.gpu
BOUND = 4e-6
DEV = "cuda"
INPUTS = set(R._shapes(1, 1, 1, 1, 1))


@pytest.fixture(scope="module")
def fx(golden):
    return golden("rewards")


def _err(got, ref):
    ref = np.asarray(ref, dtype=np.float64)
    e = np.abs(np.asarray(got, dtype=np.float64) - ref) / np.maximum(1.0, np.abs(ref))
    return float(np.max(e)) if e.size else 0.0


def _rewards(rc, N):
    return R.EnvRewards(N, DEV, rc, feet_indices=S.REWARD_FEET, penalised_contact_indices=S.REWARD_PENALISED, hip_indices=S.REWARD_HIPS)


def _load_state(E, env):
    E.feet_air_time.copy_(torch.from_numpy(env["feet_air_time"]))
    E.stumble.copy_(torch.from_numpy(env["stumble"]))
    E.pitch_est.copy_(torch.from_numpy(env["pitch_est"]))


def _call(E, env, **kw):
    inp = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in env.items() if k in INPUTS}
    lc = torch.from_numpy(env["last_contacts"].copy()).to(DEV)
    rew, per = E(last_contacts=lc, per_term=True, **inp, **kw)
    return rew.cpu().numpy(), per.cpu().numpy(), lc.cpu().numpy()


def _count(per_term, scale):
    """A discrete term's count from term * scale (fp32 products: the count is the nearest integer)."""
    c = np.asarray(per_term, dtype=np.float64) / scale
    assert np.all(np.isnan(c) | (np.abs(c - np.round(c)) < 1e-5))
    return np.round(c)


def _check_terms(rc, per, ref_per, worst, tag):
    for i, n in enumerate(rc.names):
        if n in O.DISCRETE:
            np.testing.assert_array_equal(_count(per[i], rc.scales[n]), _count(ref_per[n], rc.scales[n]), err_msg=f"{tag} {n}")
        else:
            worst[n] = max(worst.get(n, 0.0), _err(per[i], ref_per[n]))


@pytest.mark.parametrize("only_positive", [False, True])
@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("N", [1, 64, 1024, 4099])
def test_every_term_matches_oracle(fx, tag, N, only_positive):
    rc = R.RewardConfig.from_cfg(cfg_from_fixture(fx, tag))
    rc.only_positive_rewards = only_positive
    cfg = oracle_cfg(rc)
    env = O.np_state(S.reward_state(N, seed=11 + N))
    E = _rewards(rc, N)
    _load_state(E, env)
    E.episode_sums.copy_(torch.linspace(-1, 1, len(rc.names) * N).reshape(len(rc.names), N))
    sums0 = E.episode_sums.cpu().numpy().astype(np.float64)
    rew, per, lc = _call(E, env)
    st = {k: env[k].copy() for k in O.STATE}
    sums = {n: sums0[i].copy() for i, n in enumerate(rc.names)}
    ref_rew, ref_per = O.compute_reward(env, cfg, st, sums)
    worst = {"rew": _err(rew, ref_rew)}
    _check_terms(rc, per, ref_per, worst, tag)
    worst["sums"] = max(_err(E.episode_sums[i].cpu().numpy(), sums[n]) for i, n in enumerate(rc.names))
    if "feet_air_time" in rc.scales:
        np.testing.assert_array_equal(lc.astype(bool), st["last_contacts"])
        worst["air"] = _err(E.feet_air_time.cpu().numpy(), st["feet_air_time"])
    if "foot_clearance" in rc.scales:
        np.testing.assert_array_equal(E.stumble.cpu().numpy(), st["stumble"])
    if "orientation" in rc.scales or "orientation_roll" in rc.scales:
        worst["pitch"] = _err(E.pitch_est.cpu().numpy(), st["pitch_est"])
    print(f"\n{tag} N={N} only_positive={only_positive} max err / max(1,|ref|): "
          + " ".join(f"{k}={v:.1e}" for k, v in sorted(worst.items(), key=lambda kv: -kv[1])[:6]))
    assert max(worst.values()) <= BOUND, worst


@pytest.mark.parametrize("tag", ["lite3", "all"])
def test_twenty_steps_with_resets(fx, tag):
    N, steps, F = 1024, 20, list(S.REWARD_FEET)
    rc = R.RewardConfig.from_cfg(cfg_from_fixture(fx, tag))
    cfg = oracle_cfg(rc)
    env = O.seq_begin(S.reward_state(N, seed=900), F)
    E = _rewards(rc, N)
    _load_state(E, env)
    sums = {n: np.zeros(N) for n in rc.names}
    worst = {}
    for t in range(steps):
        rew, per, lc = _call(E, env)
        ref_rew, ref_per = O.compute_reward(env, cfg, env, sums)
        worst["rew"] = max(worst.get("rew", 0.0), _err(rew, ref_rew))
        _check_terms(rc, per, ref_per, worst, f"{tag} step {t}")
        np.testing.assert_array_equal(lc.astype(bool), env["last_contacts"])
        np.testing.assert_array_equal(E.stumble.cpu().numpy(), env["stumble"])
        worst["air"] = max(worst.get("air", 0.0), _err(E.feet_air_time.cpu().numpy(), env["feet_air_time"]))
        worst["pitch"] = max(worst.get("pitch", 0.0), _err(E.pitch_est.cpu().numpy(), env["pitch_est"]))
        worst["sums"] = max([worst.get("sums", 0.0)] + [_err(E.episode_sums[i].cpu().numpy(), sums[n]) for i, n in enumerate(rc.names)])
        ids = torch.from_numpy(O.seq_reset(env, sums)).to(DEV)
        E.feet_air_time[ids], E.pitch_est[ids], E.stumble[ids], E.episode_sums[:, ids] = 0, 0, 0, 0
        if t + 1 < steps:
            O.seq_next(env, S.reward_state(N, seed=901 + t), F)
    print(f"\n{tag} 20 steps: " + " ".join(f"{k}={v:.1e}" for k, v in sorted(worst.items(), key=lambda kv: -kv[1])[:6]))
    assert max(worst.values()) <= BOUND, worst


def test_foot_clearance_from_table(fx):
    N = 1024
    rc = R.RewardConfig.from_cfg(cfg_from_fixture(fx, "lite3"))
    cfg = oracle_cfg(rc)
    env = O.np_state(S.reward_state(N, seed=77))
    table = S.reward_table()
    # feet at the low edge of the table: index (x + border) / scale < 2 is clipped to 1, and the reference's px - 2 / py - 2
    # (= -1) wraps to the last row / column; non-finite positions clip to index 1 as well
    g = np.random.default_rng(5)
    fp = env["foot_positions"]
    edge = (-20.0 + 0.15 * g.random((192, 4)) - 0.06).astype(np.float32)    # [-20.06, -19.91): indices 0 and 1 after truncation
    fp[:64, :, 0] = edge[:64]
    fp[64:128, :, 1] = edge[64:128]
    fp[128:192, :, 0], fp[128:192, :, 1] = edge[128:192], edge[128:192][:, ::-1]
    fp[192, 0, 0], fp[193, 1, 1], fp[194, 2, 0] = np.nan, np.nan, -np.inf
    clr_ref = O.foot_clearance_from_table(env["foot_positions"], table.numpy(), 20.0, 0.05, 0.005)
    E = _rewards(rc, N)
    _load_state(E, env)
    out = torch.full((N, 4), float("nan"), device=DEV)
    del env["measured_foot_clearance"]
    rew, per, _ = _call(E, env, height_samples=table.to(DEV), foot_clearance_out=out)
    np.testing.assert_array_equal(out.cpu().numpy(), clr_ref)
    assert np.isfinite(clr_ref).all()
    st = {k: env[k].copy() for k in O.STATE}
    env["measured_foot_clearance"] = clr_ref
    i = rc.names.index("foot_clearance")
    ref = O.term("foot_clearance", env, cfg, st) * rc.scales["foot_clearance"]
    np.testing.assert_array_equal(_count(per[i], rc.scales["foot_clearance"]), _count(ref, rc.scales["foot_clearance"]))
    np.testing.assert_array_equal(E.stumble.cpu().numpy(), st["stumble"])


class _MockEnv:
    """The attributes of LeggedRobotDTC that compute_reward / reset_idx touch, on the device."""

    def __init__(self, cfg, env, N):
        self.cfg, self.num_envs, self.device, self.num_dof = cfg, N, DEV, 12
        self.feet_indices = torch.tensor(S.REWARD_FEET, device=DEV)
        self.penalised_contact_indices = torch.tensor(S.REWARD_PENALISED, device=DEV)
        self.hip_indices = torch.tensor(S.REWARD_HIPS, device=DEV)
        self.command_ranges = dict(lin_vel_x=list(cfg.commands.ranges.lin_vel_x), ang_vel_yaw=list(cfg.commands.ranges.ang_vel_yaw))
        self.rew_buf = torch.zeros(N, device=DEV)
        self.load(env)
        self.stumb_buffer = [torch.from_numpy(((env["stumble"] >> (4 - i)) & 1).astype(bool)).to(DEV) for i in range(5)]

    def load(self, env):
        for k, v in env.items():
            t = torch.from_numpy(np.ascontiguousarray(v)).to(DEV)
            if k == "default_dof_pos":
                t = t.unsqueeze(0)
            if k in ("feet_air_time", "pitch_est") and hasattr(self, k):
                continue                                   # the kernel's tensors (patched)
            if k != "stumble":
                setattr(self, k, t)

    def reset_idx(self, env_ids):
        for k in ("feet_air_time", "pitch_est"):
            getattr(self, k)[env_ids] = 0
        for b in self.stumb_buffer:
            b[env_ids] = 0
        for v in self.episode_sums.values():
            v[env_ids] = 0


def test_patch_env_matches_reference_fixture(fx):
    N, steps, stride = (int(v) for v in fx["meta"])
    F = list(S.REWARD_FEET)
    for tag in TAGS:
        seed = int(fx["seeds"][TAGS.index(tag)])
        cfg = cfg_from_fixture(fx, tag)
        env = O.seq_begin(S.reward_state(N, seed=seed), F)
        m = _MockEnv(cfg, env, N)
        m.episode_sums = {n: torch.zeros(N, device=DEV) for n in R.RewardConfig.from_cfg(cfg).names}
        Rw = R.patch_env(m)
        names = Rw.cfg.names
        worst = {}
        for t in range(steps):
            m.load(env)
            m.compute_reward()
            worst["rew"] = max(worst.get("rew", 0.0), _err(m.rew_buf.cpu().numpy(), fx[f"{tag}_rew_{t}"]))
            sums = np.stack([m.episode_sums[n].cpu().numpy()[::stride] for n in names])
            worst["sums"] = max(worst.get("sums", 0.0), _err(sums, fx[f"{tag}_sums_{t}"]))
            lc = m.last_contacts.cpu().numpy()
            np.testing.assert_array_equal(np.packbits(lc), fx[f"{tag}_contacts_{t}"], err_msg=f"{tag} step {t}")
            np.testing.assert_array_equal(Rw.stumble.cpu().numpy(), fx[f"{tag}_stumble_{t}"], err_msg=f"{tag} step {t}")
            worst["air"] = max(worst.get("air", 0.0), _err(m.feet_air_time.cpu().numpy()[::4], fx[f"{tag}_air_{t}"]))
            worst["pitch"] = max(worst.get("pitch", 0.0), _err(m.pitch_est.cpu().numpy()[::2], fx[f"{tag}_pitch_{t}"]))
            # the driver's env follows the kernel's state, as the env would
            env["last_contacts"] = lc.astype(bool)
            env["feet_air_time"], env["pitch_est"] = m.feet_air_time.cpu().numpy(), m.pitch_est.cpu().numpy()
            env["stumble"] = Rw.stumble.cpu().numpy()
            ids = np.nonzero(env["reset_buf"])[0]
            m.reset_idx(torch.from_numpy(ids).to(DEV))
            O.seq_reset(env, {})
            if t + 1 < steps:
                O.seq_next(env, S.reward_state(N, seed=seed + t + 1), F)
        print(f"\n{tag} fixture: " + " ".join(f"{k}={v:.1e}" for k, v in worst.items()))
        assert max(worst.values()) <= BOUND, (tag, worst)


def _run_once(rc, env, N):
    E = _rewards(rc, N)
    _load_state(E, env)
    rew, per, lc = _call(E, env)
    return [rew, per, lc, E.feet_air_time.cpu().numpy(), E.stumble.cpu().numpy(), E.pitch_est.cpu().numpy(), E.episode_sums.cpu().numpy()]


def test_nan_row_stays_in_its_row(fx):
    N, bad = 256, 37
    rc = R.RewardConfig.from_cfg(cfg_from_fixture(fx, "all"))
    env = O.np_state(S.reward_state(N, seed=5))
    clean = _run_once(rc, env, N)
    for k in ("dof_vel", "contact_forces", "measured_heights", "foot_positions", "base_ang_vel", "commands"):
        env[k][bad] = np.nan
    dirty = _run_once(rc, env, N)
    keep = np.arange(N) != bad
    for a, b in zip(clean, dirty):
        rows = (lambda x: np.ascontiguousarray(x.T if x.ndim == 2 and x.shape[0] != N else x))   # env axis first
        np.testing.assert_array_equal(rows(a)[keep].view(np.uint8), rows(b)[keep].view(np.uint8))
    assert np.isnan(dirty[0][bad])


def test_two_launches_same_bits(fx):
    N = 4099
    rc = R.RewardConfig.from_cfg(cfg_from_fixture(fx, "all"))
    env = O.np_state(S.reward_state(N, seed=8))
    a, b = _run_once(rc, env, N), _run_once(rc, env, N)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x.view(np.uint8), y.view(np.uint8))


def test_host_side_arguments(fx):
    """grid= changes the plane-fit grid of the instance, not the caller's config; the clearance comes from ONE source."""
    from dtc_amd.foothold import GridConfig
    rc = R.RewardConfig.from_cfg(cfg_from_fixture(fx, "lite3"))
    before = (rc.points_x, rc.points_y)
    E = R.EnvRewards(64, DEV, rc, GridConfig(points_x=tuple(S.MEASURED_POINTS_X[:11]), points_y=tuple(S.MEASURED_POINTS_Y[:7])),
                     feet_indices=S.REWARD_FEET, penalised_contact_indices=S.REWARD_PENALISED, hip_indices=S.REWARD_HIPS)
    assert (rc.points_x, rc.points_y) == before and E.P == 77
    E = _rewards(rc, 64)
    env = O.np_state(S.reward_state(64, seed=2))
    with pytest.raises(ValueError, match="not both"):
        _call(E, env, height_samples=S.reward_table().to(DEV))
