"""The surrogate step's numpy restatement (tests/sim_oracle.py) on its own: the properties the surrogate is built to have, the PD
law against the reference's torch expression, and what the seeded fixture of tests/test_hip_sim.py contains.  No GPU."""
import numpy as np
import pytest
import torch

import sim_cases as CASES
import sim_oracle as O

F = np.float32
EPS = float(np.finfo(np.float32).eps)


def _rest_state(N, cfg):
    """Default pose at rest on flat ground, no motor offsets."""
    st = CASES.state(N, cfg)
    t = CASES.tables(cfg)
    st["dof_pos"] = np.tile(t["default_dof_pos"], (N, 1))
    st["dof_vel"] = np.zeros((N, 12), dtype=F)
    st["motor_offsets"] = np.zeros((N, 12), dtype=F)
    return st, t


def test_zero_action_at_the_default_pose_on_flat_ground_is_a_fixed_point():
    cfg, N = CASES.config(), 5
    st, t = _rest_state(N, cfg)
    k = O.config_dict(cfg, CASES.ROWS, CASES.COLS)
    trace = []
    new = O.sim_step(st, k, t, np.zeros((N, 12), dtype=F), CASES.terrain(False), CASES.draws(N, 0), trace=trace)
    assert len(trace) == cfg.decimation
    for s in trace:
        assert s["contact"].all() and (s["n_c"] == 4).all()
        assert (s["tau"] == 0).all() and (s["omega"] == 0).all() and (s["vbx"] == 0).all() and (s["vby"] == 0).all()
        assert (s["base_z"] == F(cfg.nominal_height)).all()
    assert np.array_equal(new["dof_pos"], st["dof_pos"]) and (new["dof_vel"] == 0).all() and (new["torques"] == 0).all()
    assert np.array_equal(new["root_states"][:, :2], st["root_states"][:, :2])
    assert (new["root_states"][:, 2] == F(cfg.nominal_height)).all() and cfg.nominal_height == pytest.approx(0.4 * np.cos(0.8))
    assert (new["root_states"][:, 10:] == 0).all() and (new["root_states"][:, 7:9] == 0).all()
    # unit quaternions stay unit quaternions to rounding; the weight is shared by the four feet
    assert np.allclose(new["root_states"][:, 5] ** 2 + new["root_states"][:, 6] ** 2, 1.0, atol=4 * EPS)
    assert (new["contact_forces"][:, list(cfg.feet), 2] == F(cfg.mass * cfg.gravity) / F(4)).all()
    # a second step from there: z is now the nominal height, so the vertical velocity is zero too
    again = O.sim_step(dict(st, **new), k, t, np.zeros((N, 12), dtype=F), CASES.terrain(False), CASES.draws(N, 1))
    assert (again["root_states"][:, 9] == 0).all() and np.array_equal(again["root_states"][:, :7], new["root_states"][:, :7])


def test_pd_torque_is_the_reference_expression():
    """_compute_torques, control type "P" (legged_robot.py:610-630) with the current action in the lag slot, in torch on the CPU:
    one substep, equal bits."""
    cfg, N = CASES.config(decimation=1), 33
    st, t = CASES.state(N, cfg), CASES.tables(cfg)
    a = CASES.actions(N, cfg, 0)
    trace = []
    O.sim_step(st, O.config_dict(cfg, CASES.ROWS, CASES.COLS), t, a, CASES.terrain(False), CASES.draws(N, 0), trace=trace)
    T = lambda v: torch.from_numpy(np.ascontiguousarray(v))
    actions = torch.clip(T(a), -cfg.clip_actions, cfg.clip_actions)                           # legged_robot_dtc.py step()
    actions_scaled = actions * cfg.action_scale
    lim = T(t["dof_pos_limits"])
    goal_actions = torch.clip(actions_scaled + T(t["default_dof_pos"]), 1.0 * lim[:, 0], 1.0 * lim[:, 1])
    torques = T(t["p_gains"]) * T(st["Kp_factors"]) * (goal_actions - T(st["dof_pos"]) + T(st["motor_offsets"])) \
        - T(t["d_gains"]) * T(st["Kd_factors"]) * T(st["dof_vel"])
    torques = torques * T(st["motor_strengths"])
    ref = torch.clip(torques, -T(t["torque_limits"]), T(t["torque_limits"])).numpy()
    assert np.array_equal(trace[0]["tau"].view(np.int32), ref.view(np.int32))
    assert (np.abs(ref) == cfg.torque_limit).any() and (np.abs(ref) < cfg.torque_limit).any()


@pytest.mark.parametrize("rough", [False, True])
def test_stance_feet_do_not_slip_on_average(rough):
    """At the fitted twist the stance feet's velocities v_b + w z^ x p_l + u_l sum to zero: n_c (v_b + w z^ x pm + um) with the
    centroids pm, um.  Bound: every term is built from at most 8 single-rounded operations on the values summed, so
    |sum| <= 16 eps * sum of the magnitudes entering it (8 roundings, a factor 2 for the centroid divisions)."""
    cfg, N = CASES.config(), 257
    trace = []
    out = CASES.run(N, cfg, rough, trace=trace)
    for s in trace:
        m = s["contact"]
        p, u, w = s["p"].astype(np.float64), s["u"].astype(np.float64), s["omega"].astype(np.float64)[:, None]
        vx = s["vbx"].astype(np.float64)[:, None] - w * p[:, :, 1] + u[:, :, 0]
        vy = s["vby"].astype(np.float64)[:, None] + w * p[:, :, 0] + u[:, :, 1]
        mag_x = np.abs(s["vbx"])[:, None] + np.abs(w * p[:, :, 1]) + np.abs(u[:, :, 0])
        mag_y = np.abs(s["vby"])[:, None] + np.abs(w * p[:, :, 0]) + np.abs(u[:, :, 1])
        assert (np.abs((vx * m).sum(1)) <= 16 * EPS * (mag_x * m).sum(1) + 1e-30).all()
        assert (np.abs((vy * m).sum(1)) <= 16 * EPS * (mag_y * m).sum(1) + 1e-30).all()
    # the same through the public tensors of the last step: world velocities of the feet in contact
    new = out[-1][2]
    feet = new["rigid_body_state"][:, list(cfg.feet)].astype(np.float64)
    m = trace[-1]["contact"]
    tot = np.abs(feet[:, :, 7:9]).sum(2)
    for i in (7, 8):
        assert (np.abs((feet[:, :, i] * m).sum(1)) <= 64 * EPS * ((tot + np.abs(new["root_states"][:, 7:9]).sum(1)[:, None]) * m).sum(1) + 1e-30).all()


def test_a_one_foot_stance_gives_no_yaw_rate_and_some_feet_always_touch():
    cfg, N = CASES.config(), 257
    trace = []
    CASES.run(N, cfg, True, trace=trace)
    ones = 0
    for s in trace:
        assert (s["n_c"] >= 1).all()
        one = s["n_c"] == 1
        ones += int(one.sum())
        assert (s["omega"][one] == 0).all()
        assert (s["omega"][s["n_c"] >= 2] != 0).any()
    assert ones > 0


@pytest.mark.parametrize("N", [1, 3, 257])
@pytest.mark.parametrize("decimation", [1, 4])
def test_fixture_reaches_every_branch(N, decimation):
    """What tests/test_hip_sim.py relies on: over its three steps the seeded inputs resample commands for some envs and not for
    others, zero a small command, clip torques, stop joints at both limits, and clamp a foot's table index at the border."""
    cfg = CASES.config(decimation)
    for rough in (False, True):
        trace = []
        out = CASES.run(N, cfg, rough, trace=trace)
        st0 = CASES.state(N, cfg)
        t = CASES.tables(cfg)
        lens = np.stack([o[2]["episode_length_buf"] for o in out])
        due = lens % cfg.resampling_steps == 0
        assert due[:, 0].any() and not due[:, 0].all()                      # env 0: due once, not due otherwise
        prev = st0["commands"]
        for i, (_, _, new) in enumerate(out):
            changed = (new["commands"] != prev).any(1)
            assert np.array_equal(changed, due[i])
            prev = new["commands"]
        assert any((np.abs(s["tau"][N - 1]) == cfg.torque_limit).any() for s in trace)
        q = np.stack([s["q"][N - 1] for s in trace])
        assert (q == t["dof_pos_limits"][:, 1]).any() and (q == t["dof_pos_limits"][:, 0]).any()
        root0 = st0["root_states"][0]
        assert (root0[0] + cfg.border_size) / cfg.horizontal_scale < -1 and (root0[1] + cfg.border_size) / cfg.horizontal_scale > CASES.COLS + 1
        if N == 257:
            n_c = np.stack([s["n_c"] for s in trace])
            assert ((n_c == 1).any() and (n_c >= 2).any()) if rough else (n_c[:, 1] == 4).all()
            assert any((o[2]["commands"][due[i], :2] == 0).all(1).any() for i, o in enumerate(out))
