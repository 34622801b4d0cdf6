"""What the balance model of dtc_sim_balance does, on the CPU: properties of tests/sim_balance_oracle.py's float64 run on scenes that
stand still (the step's tensors the same every step, only the lean carried), the scenarios of the GPU test taking every branch,
`BalanceConfig.validate()`, the binding, and the env without the option.  No GPU."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import sim_balance_cases as BC
import sim_balance_oracle as BO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 0.02


def _scene(stance, off=(0.0, 0.0), lean=(0.0, 0.0, 0.0, 0.0), height=BC.HEIGHT, dtype=np.float64):
    """One env at yaw 0 over the default stance, the base `off` from the stance centre; the float tensors in `dtype`."""
    st = dict(root_states=np.zeros((1, 13)), base_pos=np.array([[off[0], off[1], height]]), base_quat=np.array([[0.0, 0.0, 0.0, 1.0]]),
              projected_gravity=np.array([[0.0, 0.0, -1.0]]), base_lin_vel=np.zeros((1, 3)), base_ang_vel=np.zeros((1, 3)),
              rigid_body_state=np.zeros((1, BC.B, 13)), contact_forces=np.zeros((1, BC.B, 3)), lean=np.array([lean], dtype=np.float64),
              contact_filt=np.array([stance], dtype=bool), episode_length_buf=np.array([7], dtype=np.int64))
    st["root_states"][0, :3], st["root_states"][0, 6] = st["base_pos"][0], 1.0
    for l in range(4):
        st["rigid_body_state"][0, BC.FEET[l], 0:2] = BC.CORNERS[l]
    return {k: (v.astype(dtype) if v.dtype == np.float64 else v) for k, v in st.items()}


def _constants():
    return BO.balance_dict(BC.Balance(), 0.005, 4)


def test_the_default_pose_on_four_feet_never_leans():
    for dtype in (np.float64, np.float32):
        st = _scene((1, 1, 1, 1), dtype=dtype)
        lean, fallen = BO.run(st, BC.FEET, _constants(), 200, dtype)
        assert (lean == 0).all() and not fallen.any()
        out = BO.balance(st, BC.FEET, _constants(), dtype)
        for name in ("root_states", "base_pos", "base_quat", "projected_gravity", "base_lin_vel", "base_ang_vel", "contact_forces"):
            assert np.array_equal(out[name], st[name]) and out[name].dtype == dtype, name
        assert np.array_equal(out["rigid_body_state"][0, 0, :7], st["root_states"][0, :7])


def test_a_base_outside_a_two_foot_segment_falls_in_the_linearised_pendulums_time():
    """FL and HL stand (the segment y = 0.1), the base's xy is 5 cm outside it.  With a fixed support the model is the linear
    pendulum p'' = (g h / (h^2 + d^2)) p + g d / (h^2 + d^2): p(t) = (d / h) (cosh(lambda t) - 1), lambda^2 = g h / (h^2 + d^2)."""
    d, h, k = 0.05, BC.HEIGHT, _constants()
    st = _scene((1, 0, 1, 0), off=(0.0, 0.1 - d))
    lean, fallen = BO.run(st, BC.FEET, k, 100)
    lam = math.sqrt(9.81 * h / (h * h + d * d))
    t_fall = math.acosh(1.0 + 0.8 * h / d) / lam
    first = int(np.argmax(fallen[:, 0]))
    assert fallen[:, 0].any() and abs((first + 1) * DT - t_fall) <= 0.1 * t_fall, ((first + 1) * DT, t_fall)
    assert (lean[1:first + 2, 0, 1] < 0).all() and np.abs(lean[:, 0, 0]).max() < 1e-12          # it tips away from the segment: -y
    assert (np.diff(np.abs(lean[:first + 2, 0, 1])) > 0).all()
    out = BO.balance(dict(st, lean=lean[first]), BC.FEET, k, np.float64)
    assert out["fallen"][0] == 1 and out["contact_forces"][0, 0, 2] == 200.0 and out["projected_gravity"][0, 1] < -0.5
    assert out["base_pos"][0, 2] < BC.HEIGHT - 0.05 and out["base_ang_vel"][0, 0] > 1.0       # the base drops; it rolls about +x


def test_a_lean_over_the_support_returns_to_exactly_zero_and_stays():
    """Four feet, the base 2 cm to the left of the centre: 8 cm inside the nearest edge (y = 0.1), a lean of 0.2 rad forward."""
    for dtype in (np.float64, np.float32):
        st = _scene((1, 1, 1, 1), off=(0.0, 0.02), lean=(0.2, 0.0, 0.0, 0.0), dtype=dtype)
        lean, fallen = BO.run(st, BC.FEET, _constants(), 60, dtype)
        zero = np.nonzero((lean[:, 0] == 0).all(axis=1))[0]
        assert zero.size and (lean[zero[0]:] == 0).all() and not fallen.any()
        # a constant deceleration g * 0.08 / (h^2 + 0.08^2) from rest: sqrt(2 * 0.2 / a) seconds, within two steps
        a = 9.81 * 0.08 / (BC.HEIGHT ** 2 + 0.08 ** 2)
        assert abs(zero[0] * DT - math.sqrt(0.4 / a)) <= 2 * DT
        assert (np.diff(lean[:zero[0], 0, 0]) < 0).all()


def test_no_stance_feet_leave_the_rate_unchanged():
    st = _scene((0, 0, 0, 0), lean=(0.05, -0.02, 0.3, 0.1))
    lean, fallen = BO.run(st, BC.FEET, _constants(), 10)
    assert (lean[:, 0, 2] == 0.3).all() and (lean[:, 0, 3] == 0.1).all()
    assert np.allclose(lean[:, 0, 0], 0.05 + 0.3 * DT * np.arange(11), rtol=0, atol=1e-7)


def test_one_foot_and_a_fresh_env():
    st = _scene((0, 1, 0, 0))
    out = BO.balance(st, BC.FEET, _constants(), np.float64)
    assert out["lean"][0, 2] < 0 and out["lean"][0, 3] > 0                         # away from FR (0.17, -0.1): towards -x, +y
    st["episode_length_buf"][:] = 1
    st["lean"][:] = (0.3, 0.1, 1.0, 1.0)
    out = BO.balance(st, BC.FEET, _constants(), np.float64)
    assert (out["lean"] == 0).all() and out["fallen"][0] == 0


@pytest.mark.parametrize("tilted", [False, True], ids=["level", "tilted"])
def test_the_seeded_cases_take_every_branch(tilted):
    """What tests/test_hip_sim_balance.py relies on, with the oracle alone: at every N the rounds take every branch."""
    for N in (1, 3, 5, 257):
        seen = dict.fromkeys(BO.BRANCHES, 0)
        for r in range(BC.rounds(N)):
            _, trace = BC.expected(BC.state(N, tilted, r), tilted)
            for name, v in BO.branches(trace).items():
                seen[name] += v
        assert all(v > 0 for v in seen.values()), (N, seen)


def test_the_lean_rotation_is_a_unit_quaternion_about_the_horizontal_axis():
    """float64: q' is unit, the body's z axis tips towards p by 2 atan(|p| / 2), projected_gravity is the world's down seen from the leaned body (a nose that tips down sees gravity ahead)."""
    st = _scene((0, 0, 0, 0), lean=(0.3, -0.4, 0.0, 0.0))
    out = BO.balance(st, BC.FEET, _constants(), np.float64)
    q = out["base_quat"][0]
    assert abs(np.linalg.norm(q) - 1) < 1e-15 and q[2] == 0
    up = np.array([2 * (q[0] * q[2] + q[3] * q[1]), 2 * (q[1] * q[2] - q[3] * q[0]), 1 - 2 * (q[0] ** 2 + q[1] ** 2)])
    ang = 2 * math.atan(0.25)
    assert np.allclose(up, [math.sin(ang) * 0.6, math.sin(ang) * -0.8, math.cos(ang)], atol=1e-15)
    assert np.allclose(out["projected_gravity"][0], [math.sin(ang) * 0.6, math.sin(ang) * -0.8, -math.cos(ang)], atol=1e-15)
    assert np.array_equal(out["root_states"][0, 3:7], q) and np.array_equal(out["rigid_body_state"][0, 0, 3:7], q)
    assert out["base_pos"][0, 2] == out["root_states"][0, 2] == out["rigid_body_state"][0, 0, 2] == BC.HEIGHT - BC.HEIGHT * 0.25 / 2


def test_balance_config_validate_refuses_each_bad_field():
    from dtc_amd import sim as SIM
    SIM.BalanceConfig().validate()
    for name in ("h_min", "fall_angle", "fall_force"):
        for v in (0.0, -1.0, float("nan")):
            with pytest.raises(ValueError, match=name):
                SIM.BalanceConfig(**{name: v}).validate()
    for v in (SIM.TERMINATION_FORCE, 50.0):
        with pytest.raises(ValueError, match="fall_force"):
            SIM.BalanceConfig(fall_force=v).validate()
    for name in ("gravity", "lean_eps"):
        with pytest.raises(ValueError, match=name):
            SIM.BalanceConfig(**{name: -1.0}).validate()
    with pytest.raises(ValueError, match="com_offset"):
        SIM.BalanceConfig(com_offset=(0.0, float("inf"))).validate()
    with pytest.raises(ValueError, match="fall_angle"):                     # SimStep validates what it is given
        SIM.SimStep(4, "cpu", SIM.SimConfig(balance=SIM.BalanceConfig(fall_angle=0.0)), SIM.flat_table(4, 4))
    d = BO.balance_dict(SIM.BalanceConfig(), 0.005, 4)                      # the oracle's stand-in holds the library's defaults
    assert d == BO.balance_dict(BC.Balance(), 0.005, 4)


def test_the_binding_and_the_abi():
    from dtc_amd import _ffi, sim as SIM
    lib = _ffi.lib()
    header = open(os.path.join(ROOT, "include", "dtc_hip.h")).read()
    assert int(re.search(r"#define\s+DTC_ABI_VERSION\s+(\d+)", header).group(1)) == _ffi.ABI_VERSION == lib.dtc_version()
    for name in ("dtc_sim_balance", "dtc_sim_balance_abi_sizes"):
        assert name in _ffi.exported_symbols() and hasattr(lib, name) and re.search(rf"\bint {name}\(", header)
    sizes = (ctypes.c_int64 * 4)()
    assert lib.dtc_sim_balance_abi_sizes(sizes, 4) == 1 and sizes[0] == ctypes.sizeof(_ffi.DtcSimBalance) == 48
    assert lib.dtc_sim_balance_abi_sizes(None, 0) == 1
    assert lib.dtc_sim_abi_sizes(sizes, 4) == 2 and lib.dtc_sim_contact_abi_sizes(sizes, 4) == 1      # the older tables keep their entries
    fields = [n for n, _ in _ffi.DtcSimBalance._fields_]
    body = re.search(r"typedef struct DtcSimBalance \{(.*?)\} DtcSimBalance;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [n.strip(" *").split("[")[0] for decl in body.split(";") if decl.strip() for n in re.sub(r"^\s*(const\s+)?\w+\s*\*?", "", decl.strip()).split(",")]
    assert declared == fields, (declared, fields)
    assert lib.dtc_sim_balance(None, None, None, 4, None) != 0 and b"null descriptor" in lib.dtc_last_error()
    step = SIM.SimStep(4, "cpu", SIM.SimConfig(balance=SIM.BalanceConfig(com_offset=(0.01, -0.02))), SIM.flat_table(4, 4))
    b = step.balance_struct()
    assert b.dt == np.float32(0.02) and tuple(b.com_offset) == (np.float32(0.01), np.float32(-0.02)) and b.fall_force == 200.0


def test_without_balance_the_env_never_calls_the_new_entry_point(monkeypatch):
    """balance=None: `SimStep.balance` is replaced by a function that raises, the env constructs, owns neither tensor, and hands the
    reset no row more; with the option it owns the two and `lean` is among the rows a reset clears."""
    import torch
    from dtc_amd import _ffi, sim as SIM
    from dtc_amd.env import SurrogateConfig, SurrogateLeggedEnv
    from dtc_amd.env import surrogate

    def refuse(*a, **kw):
        raise AssertionError("SimStep.balance called by an env without balance")
    env = SurrogateLeggedEnv(4, "cpu", SurrogateConfig(), seed=3)
    assert env.config.sim.balance is None and not hasattr(env, "lean") and not hasattr(env, "fallen") and env._balance_rows == ()
    with pytest.raises(_ffi.DtcError, match="needs config.balance"):
        env.sim.balance(env)
    on = SurrogateLeggedEnv(4, "cpu", SurrogateConfig(sim=SIM.SimConfig(balance=SIM.BalanceConfig())), seed=3)
    assert set(vars(on)) - set(vars(env)) == {"lean", "fallen"} and set(vars(env)) <= set(vars(on))
    monkeypatch.setattr(SIM.SimStep, "balance", refuse)
    monkeypatch.setattr(_ffi.lib(), "dtc_sim_balance", refuse, raising=True)
    called = []
    monkeypatch.setattr(SIM.SimStep, "step", lambda self, *a, **kw: called.append("step"))
    with pytest.raises(Exception) as info:                                 # no device: the step ends at the first kernel behind the two
        env.step(torch.zeros(4, 12))
    assert called == ["step"] and "SimStep.balance called" not in str(info.value)
    assert on.lean.shape == (4, 4) and on.lean.dtype == torch.float32 and on.fallen.shape == (4,) and on.fallen.dtype == torch.uint8
    assert on._balance_rows == (on.lean,)
    with pytest.raises(AssertionError, match="SimStep.balance called"):
        on.step(torch.zeros(4, 12))
    assert surrogate.BALANCE_SCALES == dict(orientation=-0.5, termination=-0.1) and not set(surrogate.BALANCE_SCALES) & set(surrogate._SCALES)
