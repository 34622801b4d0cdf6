"""CPU: the float64 reward oracle (tests/golden/reward_oracle.py) reproduces the reference's compute_reward, captured in
tests/golden/rewards.npz by tests/golden/make_reward_golden.py, step by step; RewardConfig.from_cfg resolves the scales as the
reference's _prepare_reward_function does."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import reward_oracle as O  # noqa: E402
from dtc_amd import synthetic as S  # noqa: E402
from dtc_amd.rewards import RewardConfig, TERMS  # noqa: E402

TAGS = ("lite3", "x30", "all")


@pytest.fixture(scope="module")
def fx(golden):
    return golden("rewards")


def cfg_from_fixture(z, tag):
    """A LeggedRobotCfg-shaped config holding the raw scale attributes and reward settings the fixture recorded."""
    raw = dict(zip([str(n) for n in z[f"{tag}_raw_names"]], [float(v) for v in z[f"{tag}_raw_values"]]))
    p = z[f"{tag}_params"]
    rewards = type("rewards", (), dict(scales=type("scales", (), raw), tracking_sigma=p[1], soft_dof_vel_limit=p[2],
                                       soft_torque_limit=p[3], base_height_target=p[4], max_contact_force=p[5], max_acc=p[6],
                                       only_positive_rewards=bool(p[7])))
    ranges = type("ranges", (), dict(lin_vel_x=[-p[8], p[8]], ang_vel_yaw=[-p[9], p[9]]))
    return type("cfg", (), dict(rewards=rewards, sim=type("sim", (), dict(dt=0.005)), control=type("control", (), dict(decimation=4)),
                                commands=type("commands", (), dict(ranges=ranges)),
                                terrain=type("terrain", (), dict(measured_points_x=S.MEASURED_POINTS_X,
                                                                 measured_points_y=S.MEASURED_POINTS_Y))))


def oracle_cfg(rc: RewardConfig):
    r = dict(tracking_sigma=rc.tracking_sigma, soft_dof_vel_limit=rc.soft_dof_vel_limit, soft_torque_limit=rc.soft_torque_limit,
             base_height_target=rc.base_height_target, max_contact_force=rc.max_contact_force, max_acc=rc.max_acc,
             only_positive_rewards=rc.only_positive_rewards)
    ranges = dict(lin_vel_x=[-rc.lin_vel_x_max, rc.lin_vel_x_max], ang_vel_yaw=[-rc.ang_vel_yaw_max, rc.ang_vel_yaw_max])
    return O.config(rc.scales, r, ranges, rc.dt, S.REWARD_FEET, S.REWARD_PENALISED, S.REWARD_HIPS, rc.points_x, rc.points_y)


def run_oracle_sequence(cfg, N, steps, seed):
    """Yields (rew, per_term dict, episode sums before the reset, env) per step of the fixture's sequence."""
    F = list(S.REWARD_FEET)
    env = O.seq_begin(S.reward_state(N, seed=seed), F)
    sums = {n: np.zeros(N) for n in cfg["scales"]}
    for t in range(steps):
        rew, per = O.compute_reward(env, cfg, env, sums)
        yield rew, per, {k: v.copy() for k, v in sums.items()}, env
        O.seq_reset(env, sums)
        if t + 1 < steps:
            O.seq_next(env, S.reward_state(N, seed=seed + t + 1), F)


def _close(got, ref, rel):
    ref = np.asarray(ref, dtype=np.float64)
    err = np.abs(np.asarray(got, dtype=np.float64) - ref) / np.maximum(1.0, np.abs(ref))
    return float(err.max()) if err.size else 0.0


@pytest.mark.parametrize("tag", TAGS)
def test_from_cfg_matches_reference_scales(fx, tag):
    rc = RewardConfig.from_cfg(cfg_from_fixture(fx, tag))
    names = [str(n) for n in fx[f"{tag}_names"]]
    assert rc.names == names
    np.testing.assert_array_equal(np.array([rc.scales[n] for n in names], dtype=np.float32), fx[f"{tag}_scales"])
    assert all(n in TERMS for n in names)
    if tag == "all":
        assert sorted(names) == sorted(TERMS) and rc.only_positive_rewards


def test_fixture_counts(fx):
    assert len(fx["lite3_names"]) == 24 and len(fx["x30_names"]) == 18 and len(fx["all_names"]) == 34


@pytest.mark.parametrize("tag", TAGS)
def test_oracle_reproduces_reference(fx, tag):
    N, steps, stride = (int(v) for v in fx["meta"])
    seed = int(fx["seeds"][TAGS.index(tag)])
    rc = RewardConfig.from_cfg(cfg_from_fixture(fx, tag))
    cfg = oracle_cfg(rc)
    names = rc.names
    worst = {}
    for t, (rew, per, sums, env) in enumerate(run_oracle_sequence(cfg, N, steps, seed)):
        worst["rew"] = max(worst.get("rew", 0.0), _close(rew, fx[f"{tag}_rew_{t}"], 1e-6))
        ref_per, ref_sums = fx[f"{tag}_per_{t}"], fx[f"{tag}_sums_{t}"]
        for i, n in enumerate(names):
            got = per[n][::stride]
            if n in O.DISCRETE:
                sc = rc.scales[n]
                np.testing.assert_array_equal(got / sc, np.round(ref_per[i].astype(np.float64) / sc), err_msg=f"{tag} step {t} {n}")
            else:
                worst[n] = max(worst.get(n, 0.0), _close(got, ref_per[i], 1e-6))
            worst["sums"] = max(worst.get("sums", 0.0), _close(sums[n][::stride], ref_sums[i], 1e-6))
        np.testing.assert_array_equal(np.packbits(env["last_contacts"]), fx[f"{tag}_contacts_{t}"])
        np.testing.assert_array_equal(env["stumble"], fx[f"{tag}_stumble_{t}"])
        worst["air"] = max(worst.get("air", 0.0), _close(env["feet_air_time"][::4], fx[f"{tag}_air_{t}"], 1e-6))
        worst["pitch"] = max(worst.get("pitch", 0.0), _close(env["pitch_est"][::2], fx[f"{tag}_pitch_{t}"], 1e-6))
    bad = {k: v for k, v in worst.items() if v > 1e-6}
    assert not bad, (bad, worst)


def test_threshold_rows_sides():
    """The rows of synthetic.threshold_rows land on the side their docstring states."""
    d = O.np_state(S.reward_state(16, seed=3))
    rc = RewardConfig(scales={n: 1.0 for n in TERMS}, max_acc=100.0)
    cfg = oracle_cfg(rc)
    st = {k: d[k].copy() for k in O.STATE}
    assert not (d["contact_forces"][0, S.REWARD_FEET[0], 2] > np.float32(1.0))
    assert O.term("stand_still", d, cfg, dict(st))[1] == 0.0
    assert O.term("big_pitch", d, cfg, dict(st))[2] == 0.0
    assert O.term("foothold_miss", d, cfg, dict(st))[4] == 0.0
    f = d["contact_forces"][6, S.REWARD_FEET[0]]
    assert not (np.hypot(f[0], f[1]) > 3 * abs(f[2]))
    assert not (d["measured_foot_clearance"][3, 1] > np.float32(0.18)) and d["terrain_levels"][5] == 5
