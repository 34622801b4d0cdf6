"""dtc_sim_contacts on the CPU: what the model of tests/sim_contact_oracle.py does, each property checked on its float32 run against
its own float64 run; `ContactConfig.validate`, `knee_tables`, the binding, and the opt-out.  No GPU."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import sim_contact_cases as CC
import sim_contact_oracle as CO
import sim_oracle as O

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# float32 against float64 on values of order 1 m and 200 N: positions within 1e-6 m, forces within stiffness * 1e-6 + 1e-4 N
POS_TOL, FORCE_TOL = 1e-6, 5e-3 + 1e-4


def _flat(cfg, rows=200, cols=200):
    return np.zeros((rows, cols), dtype=np.int16), O.config_dict(cfg, rows, cols)


def _standing(cfg, N=1, z=None, dq=None, yaw=0.0):
    """An env at the default pose (plus `dq` on every leg) over (3, 3) at height `z`: the rows a surrogate step writes."""
    t, B = CC.tables(cfg), cfg.num_bodies
    z = cfg.nominal_height if z is None else z
    dof = np.tile(t["default_dof_pos"], (N, 1)).astype(np.float64)
    if dq is not None:
        dof += np.tile(np.asarray(dq, dtype=np.float64), 4)
    base = np.tile(np.array([3.0, 3.0, z]), (N, 1))
    q = np.tile(np.array([0.0, 0.0, math.sin(yaw / 2), math.cos(yaw / 2)]), (N, 1))
    rb, cf = np.zeros((N, B, 13)), np.zeros((N, B, 3))
    for l in range(4):
        d = dof[0, 3 * l:3 * l + 3] - t["default_dof_pos"][3 * l:3 * l + 3]
        rb[:, cfg.feet[l], 0:3] = base + CC._rot(q[0], t["foot_nominal"][l] + t["leg_jacobian"][l] @ d)
        rb[:, cfg.thighs[l], 0:3] = base + CC._rot(q[0], t["hip_offset"][l])
    return {k: v.astype(F) for k, v in dict(base_pos=base, base_quat=q, dof_pos=dof, rigid_body_state=rb, contact_forces=cf).items()}


def _both(st, cfg, hs, k):
    """The oracle in float32 and in float64 on the same float32 inputs."""
    out = []
    for T in (F, np.float64):
        trace = {}
        out.append((CO.contacts(st, k, CO.contact_dict(cfg.contacts), CC.tables(cfg), CO.knee_tables(cfg, T), hs, dtype=T, trace=trace), trace))
    (o32, t32), (o64, t64) = out
    assert np.array_equal(o32["leg_contact"], o64["leg_contact"]) and np.array_equal(o32["stumbled"], o64["stumbled"])
    assert np.abs(o32["contact_forces"] - o64["contact_forces"]).max() <= FORCE_TOL
    assert np.abs(o32["rigid_body_state"] - o64["rigid_body_state"]).max() <= POS_TOL
    return o32, t32, t64


def test_the_lookup_is_the_surrogate_steps_own():
    cfg = CC.config()
    hs, k = CC.terrain(), O.config_dict(cfg, CC.ROWS, CC.COLS)
    g = np.random.default_rng(3)
    x, y = (8 * g.random(4000) - 2).astype(F), (7 * g.random(4000) - 2).astype(F)          # past every border as well
    assert np.array_equal(CO.terrain_height(k, hs, x, y), O.terrain_height(k, hs, x, y))
    assert CO.terrain_height(k, hs, np.array([np.nan], dtype=F), np.array([0.5], dtype=F))[0] == O.terrain_height(k, hs, F([-50]), F([0.5]))[0]


def test_flat_ground_default_pose_gives_nothing():
    cfg = CC.config()
    hs, k = _flat(cfg)
    for yaw in (0.0, 0.7):
        o, t, _ = _both(_standing(cfg, yaw=yaw), cfg, hs, k)
        assert not o["contact_forces"].any() and not o["leg_contact"].any() and not o["stumbled"].any()
        assert (t["d_thigh"] == 0).all() and (t["d_shank"] == 0).all()
        knee = o["rigid_body_state"][0, list(cfg.contacts.shanks), 0:3]
        assert np.abs(knee[:, 2] - (cfg.nominal_height - 0.2 * math.cos(0.8))).max() < 1e-6   # the knee stands l1 cos(t1) under the hip


def test_a_crouched_leg_gets_the_spring_force_and_a_deep_one_the_cap():
    cfg = CC.config()
    hs, k = _flat(cfg)
    c = cfg.contacts
    # a crouch: the feet on the ground, the knees (l1 cos(t1) = 0.139 m under the hip) 0.05 m above it.  The shank's lowest sample,
    # three quarters of the way to the foot, stands a quarter of that high: 0.0125 m, inside body_radius
    zk = 0.05
    st = _standing(cfg, z=0.2 * math.cos(0.8) + zk)
    st["rigid_body_state"][:, list(cfg.feet), 2] = 0.0
    o, t, t64 = _both(st, cfg, hs, k)
    d = t64["d_shank"][0]
    assert (np.abs(d - (c.body_radius - 0.25 * zk)) < 1e-6).all() and (t["d_thigh"] == 0).all()
    want = c.stiffness * d
    got = o["contact_forces"][0, list(c.shanks), 2]
    assert (want < c.max_force).all() and np.abs(got - want).max() <= FORCE_TOL and (got > 0.1).all()      # above the collision threshold
    assert (o["leg_contact"][0] == [0, 1] * 4).all() and not o["contact_forces"][0, list(cfg.thighs)].any()
    assert not o["contact_forces"][0, list(c.shanks), :2].any()
    # deeper: the knee 0.1 m under the ground.  Exactly max_force, for the thigh's lowest sample too
    st = _standing(cfg, z=0.2 * math.cos(0.8) - 0.1)
    st["rigid_body_state"][:, list(cfg.feet), 2] = 0.0
    o, t, _ = _both(st, cfg, hs, k)
    assert (o["contact_forces"][0, list(c.shanks), 2] == F(c.max_force)).all() and (o["contact_forces"][0, list(cfg.thighs), 2] == F(c.max_force)).all()
    assert o["leg_contact"].all()


def _ledge(cfg):
    """Flat ground with a ledge of 0.1 m from world x = 3.2 on (the front feet of _standing stand at x = 3.17)."""
    hs, k = _flat(cfg)
    hs[int(round((3.2 + cfg.border_size) / cfg.horizontal_scale)):, :] = 20
    return hs, k


def test_a_foot_moving_toward_a_ledge_stumbles_and_the_force_opposes_its_velocity():
    cfg = CC.config()
    hs, k = _ledge(cfg)
    c = cfg.contacts
    st = _standing(cfg, N=5)
    front = cfg.feet[0]
    vel = [(0.4, 0.0), (0.4, 0.3), (3.0, 0.0), (-0.4, 0.0), (0.04, 0.0)]          # toward, obliquely toward, fast, away, under min_speed
    for n, v in enumerate(vel):
        st["rigid_body_state"][n, front, 7:9] = v
    o, t, t64 = _both(st, cfg, hs, k)
    assert o["stumbled"][:, 0].tolist() == [1, 1, 1, 0, 0] and not o["stumbled"][:, 1:].any()
    assert abs(float(t["rise"][0, 0]) - 0.1) < 1e-6 and c.probe >= 3.2 - 3.17
    for n in range(3):
        v = np.array(vel[n])
        speed = np.linalg.norm(v)
        want = -min(c.wall_damping * speed, c.max_force) * v / speed
        assert np.abs(o["contact_forces"][n, front, :2] - want).max() <= FORCE_TOL
        assert o["contact_forces"][n, front, :2] @ v < 0
    assert np.hypot(*o["contact_forces"][2, front, :2]) == pytest.approx(c.max_force, abs=FORCE_TOL)       # 600 N asked, capped
    assert not o["contact_forces"][3:, front, :2].any()                  # moving away; slower than min_speed
    assert t["speed"][4, 0] < F(c.min_speed) < t["speed"][3, 0] and t["rise"][4, 0] > F(c.stumble_height)
    assert not o["contact_forces"][:, front, 2].any()                    # foot z is the step's, not written here


def test_a_nan_row_raises_nothing_and_flags_nothing():
    cfg = CC.config()
    st = CC.state(4, cfg, True, nan_rows=(1, 3))
    with np.errstate(all="raise"):                                        # the oracle silences its own arithmetic and nothing else
        out, trace = CC.expected(st, cfg)
    clean, _ = CC.expected(CC.state(4, cfg, True), cfg)
    rows = list(cfg.thighs) + list(cfg.contacts.shanks)
    for n in (1, 3):
        assert not out["leg_contact"][n].any() and not out["stumbled"][n].any()
        assert (out["contact_forces"][n, rows] == 0).all() and (out["contact_forces"][n, list(cfg.feet), :2] == 0).all()
        assert np.array_equal(out["contact_forces"][n, 0], st["contact_forces"][n, 0])
    for n in (0, 2):
        for name in out:
            assert np.array_equal(out[name][n].view(np.uint8), clean[name][n].view(np.uint8)), name
    # one NaN alone, a foot's z: its shank's four samples are NaN (the knee's too: 0 * NaN) and drop out, its thigh's are not, and
    # the rise ahead of it compares false
    st = CC.state(2, cfg, False)
    st["rigid_body_state"][0, cfg.feet[2], 2] = np.nan
    out, trace = CC.expected(st, cfg)
    assert np.isnan(trace["pens"][0, 2, 3:]).all() and not np.isnan(trace["pens"][0, 2, :3]).any() and np.isnan(trace["rise"][0, 2])
    assert trace["d_shank"][0, 2] == 0 and out["leg_contact"][0, 5] == 0 and out["stumbled"][0, 2] == 0
    assert not out["contact_forces"][0, cfg.contacts.shanks[2]].any() and not out["contact_forces"][0, cfg.feet[2], :2].any()


@pytest.mark.parametrize("tilted", [False, True], ids=["level", "tilted"])
def test_the_seeded_cases_take_every_branch(tilted):
    """What tests/test_hip_sim_contacts.py asserts before it compares, checked here without a GPU: env 0 alone (N = 1) takes every
    branch, so every N does; with NaN rows the finite ones still do."""
    cfg = CC.config()
    ck = CO.contact_dict(cfg.contacts)
    for N in (1, 3, 5, 257):
        _, trace = CC.expected(CC.state(N, cfg, tilted), cfg)
        seen = CC.branches(trace, ck)
        assert set(seen) == set(CC.BRANCHES) and all(v > 0 for v in seen.values()), (N, seen)
    _, trace = CC.expected(CC.state(9, cfg, True, nan_rows=(1, 4, 8)), cfg)
    seen = CC.branches(trace, ck, rows=[0, 2, 3, 5, 6, 7])
    assert all(v > 0 for v in seen.values()), seen


def test_contact_config_validate_refuses_each_bad_field():
    from dtc_amd import sim as SIM
    SIM.ContactConfig().validate()
    SIM.ContactConfig().validate(SIM.SimConfig())
    SIM.ContactConfig(body_radius=0.0, stumble_height=0.0, min_speed=0.0).validate(SIM.SimConfig())
    for name in ("stiffness", "max_force", "probe", "wall_damping"):
        for v in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match=name):
                SIM.ContactConfig(**{name: v}).validate()
    for name in ("body_radius", "stumble_height", "min_speed"):
        for v in (-1e-3, float("nan"), float("inf"), -float("inf")):
            with pytest.raises(ValueError, match=name):
                SIM.ContactConfig(**{name: v}).validate()
    for shanks in ((0, 7, 11, 15), (4, 7, 11, 15), (2, 7, 11, 15), (3, 7, 11, 17), (-1, 7, 11, 15)):       # base, foot, thigh, outside
        with pytest.raises(ValueError, match="shank"):
            SIM.ContactConfig(shanks=shanks).validate(SIM.SimConfig())
    with pytest.raises(ValueError, match="shanks"):
        SIM.ContactConfig(shanks=(3, 3, 11, 15)).validate()
    with pytest.raises(ValueError):                                      # SimStep validates against its own layout
        SIM.SimStep(4, "cpu", SIM.SimConfig(contacts=SIM.ContactConfig(shanks=(4, 7, 11, 15))), SIM.flat_table(4, 4))
    assert SIM.SimConfig().contacts is None


def test_knee_tables_agree_with_a_finite_difference_of_the_closed_form_knee():
    from dtc_amd import sim as SIM
    cfg = SIM.SimConfig(default_dof_pos=(0.1, -0.8, 1.6, -0.2, -0.7, 1.5, 0.0, -0.9, 1.7, 0.05, -0.8, 1.6))
    l1 = cfg.link_lengths[0]
    hip = np.asarray(cfg.hip_offset)

    def knee(l, q):
        a, t1, _ = q
        return hip[l] + np.array([-l1 * math.sin(t1), l1 * math.cos(t1) * math.sin(a), -l1 * math.cos(t1) * math.cos(a)])
    t = SIM.knee_tables(cfg)
    assert t["knee_nominal"].dtype == t["knee_jacobian"].dtype == np.float64 and t["knee_nominal"].shape == (4, 3) and t["knee_jacobian"].shape == (4, 3, 3)
    q0 = np.asarray(cfg.default_dof_pos).reshape(4, 3)
    h = 1e-6
    for l in range(4):
        assert np.abs(t["knee_nominal"][l] - knee(l, q0[l])).max() < 1e-15
        for j in range(3):
            e = np.zeros(3)
            e[j] = h
            fd = (knee(l, q0[l] + e) - knee(l, q0[l] - e)) / (2 * h)
            assert np.abs(t["knee_jacobian"][l, :, j] - fd).max() < 1e-9, (l, j)
        assert not t["knee_jacobian"][l, :, 2].any()                      # the knee does not move with the knee joint
    # the knee lies on the leg of leg_tables: l1 from the hip, l2 from the foot
    lt = SIM.leg_tables(cfg)
    assert np.abs(np.linalg.norm(t["knee_nominal"] - hip, axis=1) - l1).max() < 1e-15
    assert np.abs(np.linalg.norm(lt["foot_nominal"] - t["knee_nominal"], axis=1) - cfg.link_lengths[1]).max() < 1e-15


def test_the_binding_and_the_abi():
    from dtc_amd import _ffi
    lib = _ffi.lib()
    header = open(os.path.join(ROOT, "include", "dtc_hip.h")).read()
    assert int(re.search(r"#define\s+DTC_ABI_VERSION\s+(\d+)", header).group(1)) == 25 == _ffi.ABI_VERSION == lib.dtc_version()
    for name in ("dtc_sim_contacts", "dtc_sim_contact_abi_sizes"):
        assert name in _ffi.exported_symbols() and hasattr(lib, name) and re.search(rf"\bint {name}\(", header)
    sizes = (ctypes.c_int64 * 4)()
    assert lib.dtc_sim_contact_abi_sizes(sizes, 4) == 1 and sizes[0] == ctypes.sizeof(_ffi.DtcSimContacts) == 80
    assert lib.dtc_sim_contact_abi_sizes(None, 0) == 1
    assert lib.dtc_sim_abi_sizes(sizes, 4) == 2 and lib.dtc_sim_fly_abi_sizes(sizes, 4) == 1          # the older tables keep their entries
    fields = [n for n, _ in _ffi.DtcSimContacts._fields_]
    body = re.search(r"typedef struct DtcSimContacts \{(.*?)\} DtcSimContacts;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [n.strip(" *").split("[")[0] for decl in body.split(";") if decl.strip() for n in re.sub(r"^\s*(const\s+)?\w+\s*\*?", "", decl.strip()).split(",")]
    assert declared == fields, (declared, fields)
    # null descriptors are an error code, not a fault, with no device behind the call
    assert lib.dtc_sim_contacts(None, None, None, 4, None) != 0 and b"null descriptor" in lib.dtc_last_error()


def test_without_contacts_the_env_never_calls_the_new_entry_point(monkeypatch):
    """contacts=None: the env constructs with the binding's dtc_sim_contacts replaced by a function that raises, and owns neither
    flag tensor nor knee table."""
    import torch
    from dtc_amd import _ffi, sim as SIM
    from dtc_amd.env import SurrogateConfig, SurrogateLeggedEnv
    from dtc_amd.env import surrogate

    def refuse(*a, **kw):
        raise AssertionError("dtc_sim_contacts called by an env without contacts")
    monkeypatch.setattr(_ffi.lib(), "dtc_sim_contacts", refuse, raising=True)
    env = SurrogateLeggedEnv(4, "cpu", SurrogateConfig(), seed=3)
    assert env.config.sim.contacts is None and not hasattr(env, "leg_contact") and not hasattr(env, "stumbled") and not hasattr(env.sim, "knee")
    assert env._contact_flags == ()
    with pytest.raises(_ffi.DtcError, match="needs config.contacts"):
        env.sim.contacts(env)
    on = SurrogateLeggedEnv(4, "cpu", SurrogateConfig(sim=SIM.SimConfig(contacts=SIM.ContactConfig())), seed=3)
    assert set(vars(on)) - set(vars(env)) == {"leg_contact", "stumbled"} and set(vars(env)) <= set(vars(on))
    assert on.leg_contact.shape == (4, 8) and on.stumbled.shape == (4, 4) and on.leg_contact.dtype == on.stumbled.dtype == torch.uint8
    assert surrogate.CONTACT_SCALES == dict(collision=-1.5, stumble=-0.5) and not set(surrogate.CONTACT_SCALES) & set(surrogate._SCALES)
    assert list(env.penalised_contact_indices) == [b for l in range(4) for b in (SIM.SimConfig().thighs[l], SIM.ContactConfig().shanks[l])]
