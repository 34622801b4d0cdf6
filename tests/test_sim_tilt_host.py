"""The tilt surrogate step without a GPU: the C ABI of dtc_sim_step_tilt as the binding sees it, and the properties of the model on
its numpy float32 restatement (tests/sim_tilt_oracle.py), which the kernel is held to bit for bit in tests/test_hip_sim_tilt.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sim_cases as CASES
import sim_oracle as O
import sim_tilt_oracle as TO

F = np.float32
EPS = float(np.finfo(np.float32).eps)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ host
def test_abi_symbols_version_and_size_tables():
    from dtc_amd import _ffi
    lib = _ffi.lib()
    for name in ("dtc_sim_step_tilt", "dtc_sim_tilt_abi_sizes"):
        assert name in _ffi.exported_symbols() and hasattr(lib, name)
    header = open(os.path.join(ROOT, "include", "dtc_hip.h")).read()
    in_header = int(re.search(r"#define\s+DTC_ABI_VERSION\s+(\d+)", header).group(1))
    assert in_header >= 23 and _ffi.ABI_VERSION == in_header and lib.dtc_version() == in_header
    sizes = (C.c_int64 * 32)()
    assert lib.dtc_sim_tilt_abi_sizes(sizes, 32) == 1 and sizes[0] == C.sizeof(_ffi.DtcSimTilt) == 8
    assert lib.dtc_sim_tilt_abi_sizes(None, 0) == 1
    # the older tables keep their counts
    for table, count in (("dtc_abi_sizes", 18), ("dtc_env_reset_abi_sizes", 3), ("dtc_contain_envs_abi_sizes", 1),
                         ("dtc_act_contain_abi_sizes", 1), ("dtc_sim_abi_sizes", 2)):
        assert getattr(lib, table)(sizes, 32) == count, table


def test_the_default_config_has_no_tilt_and_bad_arguments_are_refused_before_any_launch():
    from dtc_amd import _ffi, sim as SIM
    c = SIM.SimConfig()
    assert c.tilt is False and c.max_slope == 1.0 and 0 < c.min_det < 1e-4
    lib = _ffi.lib()
    st, cfg = _ffi.DtcSimStep(), _ffi.DtcSimCfg()
    assert lib.dtc_sim_step_tilt(st, cfg, None, 4, None) != 0 and b"DtcSimTilt" in lib.dtc_last_error()
    assert lib.dtc_sim_step_tilt(st, cfg, _ffi.DtcSimTilt(1.0, 1e-6), 4, None) != 0              # the zeroed config is refused as ever


# ------------------------------------------------------------------------------------------------ the model, on the oracle
def _rest(N, cfg, yaw=0.0):
    """Default pose at rest, no motor offsets, level, heading `yaw`."""
    st, t = CASES.state(N, cfg), CASES.tables(cfg)
    st["dof_pos"] = np.tile(t["default_dof_pos"], (N, 1))
    st["dof_vel"] = np.zeros((N, 12), dtype=F)
    st["motor_offsets"] = np.zeros((N, 12), dtype=F)
    st["root_states"][:, 3:7] = TO.quaternion(np.full(N, yaw), np.zeros(N), np.zeros(N))
    return st


def test_a_identical_legs_on_flat_ground_are_the_yaw_only_step():
    """(a) Four legs in the same state with the same motor factors and per-leg identical actions on the flat table: all four demand
    the same base height, the fit gives a = b = 0 exactly and every output equals the yaw-only oracle's as numbers (the sign of a zero
    may differ), over 8 chained steps.  The tilt step normalises the yaw pair at load, the yaw-only step does not: the envs start from
    yaw pairs that the fp32 normalisation leaves unchanged (sqrt(qz^2 + qw^2) == 1 in fp32), chosen by that property of the input."""
    cfg, N = CASES.config(4, tilt=True), 7
    g = np.random.default_rng(5)
    yaw = (2 * g.random(400) - 1) * np.pi
    pair = np.stack([np.sin(yaw / 2), np.cos(yaw / 2)], axis=1).astype(F)
    fixed = np.sqrt(pair[:, 0] * pair[:, 0] + pair[:, 1] * pair[:, 1]) == F(1)
    assert fixed.sum() >= N
    pair = pair[fixed][:N]
    st = CASES.state(N, cfg)
    leg = lambda a: np.tile(a[:, :3], (1, 4))                                             # noqa: E731
    for name in ("dof_pos", "dof_vel", "Kp_factors", "Kd_factors", "motor_strengths", "motor_offsets"):
        st[name] = leg(st[name])
    st["root_states"][:, 3:5] = 0
    st["root_states"][:, 5:7] = pair
    actions = lambda i: leg(CASES.actions(N, cfg, i))                                     # noqa: E731
    tilt = TO.run(N, cfg, False, steps=8, st=st, actions=actions)
    t, hs, cur = CASES.tables(cfg), CASES.terrain(False), st
    for i, (a, u, new) in enumerate(tilt):
        ref = O.sim_step(cur, O.config_dict(cfg, CASES.ROWS, CASES.COLS, counter=i), t, a, hs, u)
        for name in O.STATE:
            assert np.array_equal(new[name], ref[name], equal_nan=new[name].dtype == F), f"step {i}: {name}"
        assert np.isfinite(new["root_states"]).all() and (new["projected_gravity"] == [0, 0, -1]).all()
        cur = dict(cur, **ref)
    assert np.abs(new["dof_vel"]).max() > 0.1                                             # the legs did move


@pytest.mark.parametrize("axis", ["x", "y"])
def test_b_the_plane_settles_on_a_ramp(axis):
    """(b) An exact ramp, 2 height units per cell: slope s = 2 * 0.005 / 0.05 = 0.2 along world x (pitch) or y (roll); level start at
    the default pose, heading along x, zero actions, 20 steps.  All four feet are stance legs of every fit, and wherever the plane is
    at rest (a substep that leaves n unchanged) all four are in contact with the ground too.

    The bound.  _get_heights reads the ramp as a staircase: h = s X - e with 0 <= e < step = s * cell = 0.01 m.  The feet pair up on
    equal X (x ramp: front / hind, baseline L = |p.x(front) - p.x(hind)| = 0.34 m; y ramp: left / right, L = 0.2 m), so the fitted
    slope is a = s rho - (e1 - e2) / L, where rho = (r1 - r2) / (p1 - p2) is the foreshortening of the baseline by the tilt the feet
    were rotated with: rho = 1 - n^2 / (1 + nz) = nz for a tilt about one axis, so 1 / sqrt(1 + a_max^2) <= rho <= 1 with
    a_max = s + step / L (by induction from the level start, rho = 1).  Hence |a - s| <= step / L + s (1 - 1 / sqrt(1 + a_max^2)),
    and since |d/da (a / sqrt(1 + a^2))| <= 1 and |d/da (1 / sqrt(1 + a^2))| <= a_max < 1, every component of projected_gravity is
    within that bound of the ramp normal's; 1e-6 covers fp32 rounding.  x: 0.0294 + 0.0051; y: 0.05 + 0.0061."""
    cfg, N = CASES.config(4, tilt=True), 12
    s, step, L = 0.2, 0.2 * cfg.horizontal_scale, dict(x=0.34, y=0.2)[axis]
    a_max = s + step / L
    bound = step / L + s * (1 - 1 / np.sqrt(1 + a_max ** 2)) + 1e-6
    st = _rest(N, cfg)
    g = np.random.default_rng(9)
    st["root_states"][:, 0], st["root_states"][:, 1] = 22 + 6 * g.random(N), 21 + 3 * g.random(N)
    ramp = 2 * np.arange(CASES.ROWS if axis == "x" else CASES.COLS, dtype=np.int16) - 900
    hs = np.ascontiguousarray(np.broadcast_to(ramp[:, None] if axis == "x" else ramp[None, :], (CASES.ROWS, CASES.COLS)))
    trace = []
    out = TO.run(N, cfg, False, steps=20, st=st, actions=lambda i: np.zeros((N, 12), dtype=F), hs=hs, trace=trace)
    pg = out[-1][2]["projected_gravity"].astype(np.float64)
    normal = np.array([-s, 0, 1] if axis == "x" else [0, -s, 1]) / np.sqrt(1 + s * s)    # the ramp rises along +x / +y
    want = np.array([normal[0], normal[1], -normal[2]])                                   # projected_gravity = (n.x, n.y, -n.z) with n the normal
    err = np.abs(pg - want).max()
    print(f"ramp along {axis}: projected_gravity {pg[0]} against {want}, largest error {err:.4f}, bound {bound:.4f}")
    assert err <= bound
    assert (pg[:, 2] > -1).all() and (-pg[:, 2] < 1).all()                                # nz < 1
    rest = 0
    for sub in trace:
        assert sub["stance"].all() and sub["fit"].all()
        still = (sub["n"] == sub["n_new"]).all(axis=1)
        assert (sub["n_c"][still] == 4).all()
        rest += int(still.sum())
    assert rest > N                                                                       # planes do come to rest


def test_c_fewer_than_three_stance_legs_and_a_collinear_stance_hold_the_tilt():
    """(c) Two legs folded by 0.2 rad at the knee (their feet 3 cm up in the body frame): two stance legs.  Three stance feet on a
    line (foot_nominal of a tripod whose third foot lies between the other two): the scatter's determinant is rounding noise.  In
    both the tilt the quaternion came with is held, on a ramp that asks for another, and wx = wy = 0."""
    cfg, N = CASES.config(4, tilt=True), 4
    hs = np.ascontiguousarray(np.broadcast_to((2 * np.arange(CASES.ROWS, dtype=np.int16) - 900)[:, None], (CASES.ROWS, CASES.COLS)))
    k = TO.config_dict(cfg, CASES.ROWS, CASES.COLS)
    for case in ("two legs", "collinear"):
        st, t = _rest(N, cfg), CASES.tables(cfg)
        st["root_states"][:, 3:7] = TO.quaternion(np.linspace(-2, 2, N), np.full(N, 0.1), np.full(N, -0.05))
        goal = np.tile(t["default_dof_pos"], (N, 1))
        if case == "two legs":
            goal[:, [5, 8]] += F(0.2)
        else:
            goal[:, 11] += F(0.2)                                                         # leg 3 folded: legs 0, 1, 2 stand
            t["foot_nominal"][2, :2] = F(0.5) * (t["foot_nominal"][0, :2] + t["foot_nominal"][1, :2])
        st["dof_pos"] = goal.copy()
        actions = ((goal - t["default_dof_pos"]) / F(cfg.action_scale)).astype(F)        # the PD goal is the pose itself
        _, _, n0 = TO.split_quaternion(st["root_states"][:, 3:7])
        trace = []
        new = TO.sim_step(st, k, t, actions, hs, CASES.draws(N, 0), trace=trace)
        for sub in trace:
            assert (sub["n_s"] == (2 if case == "two legs" else 3)).all() and not sub["fit"].any(), case
            assert (sub["wx"] == 0).all() and (sub["wy"] == 0).all()
            assert np.array_equal(sub["n_new"], np.stack(n0, axis=1))
            if case == "collinear":
                assert (np.abs(sub["det"]) < 1e-9).all()
        assert np.array_equal(new["projected_gravity"], np.stack([n0[0], n0[1], -n0[2]], axis=1))
        assert (new["root_states"][:, 10:12] == 0).all()                                 # no tilt rate in the world frame


def test_d_max_slope_clamps_at_a_one_cell_cliff():
    """(d) A cliff of 0.5 m between two rows of the table, under the belly of a level env heading along x: the front feet stand on it,
    the hind feet below, the fit asks for a = 0.5 / 0.34 > 1 and the clamp gives n = (-1, 0, 1) / sqrt(2); a smaller max_slope clamps
    sooner, a cliff of 0.1 m (a = 0.29) is followed unclamped."""
    N = 3
    for height, max_slope, want in ((100, 1.0, 1.0), (100, 0.25, 0.25), (20, 1.0, None)):
        cfg = CASES.config(4, tilt=True, max_slope=max_slope)
        st = _rest(N, cfg)
        st["root_states"][:, 0], st["root_states"][:, 1] = [5.0, 5.01, 4.99], 3.0
        hs = np.zeros((CASES.ROWS, CASES.COLS), dtype=np.int16)
        hs[int((5.0 + cfg.border_size) / cfg.horizontal_scale):] = height
        trace = []
        new = TO.sim_step(st, TO.config_dict(cfg, CASES.ROWS, CASES.COLS), CASES.tables(cfg), np.zeros((N, 12), dtype=F), hs, CASES.draws(N, 0),
                          trace=trace)
        first = trace[0]
        assert first["fit"].all() and np.allclose(first["a"], height * 0.005 / 0.34, rtol=1e-5) and (first["b"] == 0).all()
        a = F(want) if want is not None else first["a"]
        n = np.stack([-a / np.sqrt(a * a + F(1)), 0 * a, F(1) / np.sqrt(a * a + F(1))], axis=-1) * np.ones((N, 1), dtype=F)
        assert np.allclose(first["n_new"], n, atol=2 * EPS), (height, max_slope)
        assert np.isfinite(new["root_states"]).all() and (np.abs(new["projected_gravity"][:, 0]) <= max_slope / np.sqrt(1 + max_slope ** 2) + EPS).all()


def test_e_fifty_random_steps_on_the_rough_table_keep_the_state_consistent():
    """(e) Every env, every step: unit quaternion and unit projected_gravity within 1e-6; Rz Rt base_lin_vel gives root_states[7:10]
    back within 4 ulp of the largest component (float64 from the step's own yaw pair and n); per substep no foot below the terrain
    under it by more than contact_eps and at least one foot in contact.  The tilt is exercised: fits are taken, held and clamped."""
    cfg, N = CASES.config(4, tilt=True), 33
    trace = []
    out = TO.run(N, cfg, True, steps=50, trace=trace)
    worst = 0.0
    for i, (_, _, new) in enumerate(out):
        q, pg = new["base_quat"].astype(np.float64), new["projected_gravity"].astype(np.float64)
        assert np.abs(np.linalg.norm(q, axis=1) - 1).max() <= 1e-6 and np.abs(np.linalg.norm(pg, axis=1) - 1).max() <= 1e-6, f"step {i}"
        assert np.array_equal(new["base_quat"], new["root_states"][:, 3:7])
        n = np.stack([pg[:, 0], pg[:, 1], -pg[:, 2]], axis=1)
        k1 = 1 + n[:, 2]
        Rt = np.zeros((N, 3, 3))
        Rt[:, 0, 0], Rt[:, 0, 1], Rt[:, 1, 1] = 1 - n[:, 0] ** 2 / k1, -n[:, 0] * n[:, 1] / k1, 1 - n[:, 1] ** 2 / k1
        Rt[:, 1, 0], Rt[:, :, 2], Rt[:, 2, 0], Rt[:, 2, 1] = Rt[:, 0, 1], n, -n[:, 0], -n[:, 1]
        zy, wy = q[:, 2] / np.hypot(q[:, 2], q[:, 3]), q[:, 3] / np.hypot(q[:, 2], q[:, 3])
        c, s = 1 - 2 * zy * zy, 2 * zy * wy
        v = np.einsum("nij,nj->ni", Rt, new["base_lin_vel"].astype(np.float64))
        world = np.stack([c * v[:, 0] - s * v[:, 1], s * v[:, 0] + c * v[:, 1], v[:, 2]], axis=1)
        have = new["root_states"][:, 7:10].astype(np.float64)
        ulp = EPS * np.abs(have).max(axis=1, keepdims=True)
        worst = max(worst, float((np.abs(world - have) / ulp).max()))
    print(f"Rz Rt base_lin_vel against root_states[7:10]: at most {worst:.2f} ulp of the largest component")
    assert worst <= 4
    for sub in trace:
        gap = (sub["base_z"][:, None] + sub["p"][:, :, 2]) - sub["h"]
        assert (gap >= -cfg.contact_eps).all() and (sub["n_c"] >= 1).all()
    fit = np.stack([s["fit"] for s in trace])
    clamped = np.stack([(np.abs(s["a"]) > cfg.max_slope) & s["fit"] for s in trace])
    assert 0.02 < fit.mean() < 0.98 and clamped.any()
    moved = np.stack([np.abs(s["wx"]) + np.abs(s["wy"]) for s in trace])
    assert (moved[fit] > 0).any() and (moved[~fit] == 0).all()
