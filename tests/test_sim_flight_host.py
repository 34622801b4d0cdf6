"""The flight model of dtc_sim_step_fly on the CPU: properties of its specification, tests/sim_flight_oracle.py, on scenarios small
enough to reason about -- a ledge, a step up, a wall, a take-off at the joint limit, a flat table -- plus FlightConfig.validate() and
the ABI version.  No GPU, no kernel: tests/test_hip_sim_flight.py holds the kernel to the same oracle bit for bit.

Every continuous comparison below is held to four times the largest deviation of the float32 oracle from its own float64 run
(dtype=np.float64: the same recurrence from the same float32 constants) on the same scenario, measured in the test itself."""
import os
import re

import numpy as np
import pytest

import sim_actuator_oracle as AO
import sim_cases as CASES
import sim_flight_oracle as FO
import sim_oracle as O
import sim_tilt_oracle as TO

F = np.float32
EDGE = 25.0                     # world x of every scenario's feature; the base stands at y = 22 m
BASES = [(False, False), (True, False), (False, True), (True, True)]
IDS = ["yaw", "tilt", "yaw-act", "tilt-act"]


def _table(dz, lo=EDGE, hi=None):
    """A flat table whose ground lies dz metres higher for lo <= x (< hi)."""
    hs = np.zeros((CASES.ROWS, CASES.COLS), dtype=np.int16)
    hs[FO.cell(lo):(None if hi is None else FO.cell(hi))] = int(round(dz / 0.005))
    return hs


def _rest(cfg, x, z, vel=(0.0, 0.0, 0.0), elen=1, N=1):
    """N envs alike at rest in the default pose: level, heading along x, nominal gains, no commands."""
    st = CASES.state(N, cfg)
    t = CASES.tables(cfg)
    st["dof_pos"][:], st["dof_vel"][:], st["motor_offsets"][:] = t["default_dof_pos"], 0, 0
    st["Kp_factors"][:] = st["Kd_factors"][:] = st["motor_strengths"][:] = 1
    st["root_states"][:] = 0
    st["root_states"][:, 0], st["root_states"][:, 1], st["root_states"][:, 2], st["root_states"][:, 6] = x, 22.0, z, 1
    st["root_states"][:, 7:10] = vel
    st["base_ang_vel"][:], st["commands"][:], st["episode_length_buf"][:], st["last_contacts"][:] = 0, 0, elen, True
    if cfg.actuator is not None:
        st["lag_state"], st["push_vel"] = np.zeros((N, 6, 12), dtype=F), np.zeros((N, 2), dtype=F)
    st["airborne"], st["crashed"] = np.zeros(N, dtype=np.uint8), np.zeros(N, dtype=np.uint8)
    return st


def _stand(cfg):
    return F(-CASES.tables(cfg)["foot_nominal"][0, 2])


def _zero(N):
    return lambda i: np.zeros((N, 12), dtype=F)


def _pair(cfg, st, hs, steps, actions=None):
    """The float32 and the float64 run of one scenario: ((steps, trace) float32, (steps, trace) float64)."""
    out = []
    for dtype in (F, np.float64):
        tr = []
        ref = FO.run(st["root_states"].shape[0], cfg, steps=steps, trace=tr, st={k: np.array(v, copy=True) for k, v in st.items()}, hs=hs,
                     actions=actions or _zero(st["root_states"].shape[0]), dtype=dtype, push_steps=())
        out.append((ref, tr))
    return out


def _dev(tr32, tr64, key):
    return max(float(np.abs(a[key].astype(np.float64) - b[key]).max()) for a, b in zip(tr32, tr64))


def test_ledge_drop_is_a_parabola_that_lands_where_float64_says():
    """A 1.0 m step down, all four feet past the edge, entry velocity (0.3, 0, 0).  Airborne from the first substep; z follows
    z0 - g dt^2 k (k + 1) / 2 and x advances 0.3 dt per substep, each within 4 x the float32 run's largest deviation from its float64
    run (measured: z 2.13e-7 m -> bound 8.5e-7 m; x 7.33e-5 m -> bound 2.9e-4 m over the 89 substeps of the fall); no foot in contact,
    contact_filt clear from the second step; the env lands in substep k = 90 (index 89), the first k with g dt^2 k (k + 1) / 2 >=
    1 m - contact_eps = 0.995 m: k = 89 gives 0.9822 m, k = 90 1.0043 m, either side three orders of magnitude beyond the float32
    deviation, so the float32 and the float64 run land on the same substep; after it z is on the lower support."""
    cfg = FO.config(4)
    z0 = _stand(cfg)
    st = _rest(cfg, EDGE + 0.5, z0, vel=(0.3, 0.0, 0.0))
    (r32, t32), (r64, t64) = _pair(cfg, st, _table(-1.0), 25)
    air32, air64 = (np.array([s["air"][0] for s in t]) for t in (t32, t64))
    land = int(np.argmin(air32))
    assert air32[0] and land == int(np.argmin(air64)) == 89 and air32[:land].all() and not air32[land:].any()
    assert np.array_equal(air32, air64)
    g, dt = float(F(9.81)), float(F(0.005))
    k = np.arange(1, land + 1)
    z32, z64 = (np.array([s["z"][0] for s in t[:land]], dtype=np.float64) for t in (t32, t64))
    x32, x64 = (np.array([s["x"][0] for s in t[:land]], dtype=np.float64) for t in (t32, t64))
    dev_z, dev_x = _dev(t32[:land], t64[:land], "z"), _dev(t32[:land], t64[:land], "x")
    print(f"ledge drop: float32 - float64 deviation z {dev_z:.3e} m, x {dev_x:.3e} m over {land} substeps")
    assert 0 < dev_z < 1e-3 and 0 < dev_x < 1e-3
    want_z = float(z0) - g * dt * dt * k * (k + 1) / 2
    want_x = float(F(EDGE + 0.5)) + float(F(0.3)) * dt * k
    assert np.abs(z64 - want_z).max() < 1e-12 and np.abs(x64 - want_x).max() < 1e-12
    assert np.abs(z32 - want_z).max() <= 4 * dev_z and np.abs(x32 - want_x).max() <= 4 * dev_x
    for i, (*_, new) in enumerate(r32[:land // 4]):
        assert new["airborne"][0] == 1 and new["crashed"][0] == 0 and not new["last_contacts"].any() and not new["contact_forces"].any()
        assert new["contact_filt"].all() if i == 0 else not new["contact_filt"].any()
        assert new["root_states"][0, 7] == F(0.3) and new["root_states"][0, 8] == 0 and new["root_states"][0, 12] == 0
    done = r32[-1][5]
    assert done["airborne"][0] == 0 and done["crashed"][0] == 0                          # 1 m down is a landing, not a crash
    assert done["root_states"][0, 2] == F(-1.0) + z0 and done["last_contacts"].all()
    assert t32[land]["z"][0] == t32[land]["base_z"][0] and abs(float(t32[land]["z"][0]) - (float(z0) - 1.0)) < 1e-6


@pytest.mark.parametrize("tilt,act", BASES, ids=IDS)
def test_step_up_wall_and_reset_exemption(tilt, act):
    """Three envs alike whose front feet stand past the edge of a step up.  0.15 m: no crash, and z equals the flight-off oracle's
    bit for bit.  0.5 m: crashed, contact_forces[n, 0] = (0, 0, crash_force), and the existing check_termination oracle resets the
    crashed env and no other (env 1 of three enters with episode_length_buf == 0: the reset exemption; env 2 stands clear of the
    wall)."""
    from oracle.observations import check_termination
    cfg = FO.config(4, tilt, act)
    off = CASES.config(4, tilt=tilt, actuator=cfg.actuator)
    z0, N = _stand(cfg), 3
    x = np.array([EDGE - 0.1, EDGE - 0.1, EDGE - 1.0], dtype=F)                          # feet at x +- 0.17
    for dz, crash in ((0.15, False), (0.5, True)):
        hs = _table(dz)
        st = _rest(cfg, x, z0, N=N)
        st["episode_length_buf"][1] = 0
        k = FO.config_dict(cfg, hs.shape[0], hs.shape[1])
        ch = AO.choices(4, 0) if act else None
        tr = []
        new = FO.sim_step(st, k, CASES.tables(cfg), np.zeros((N, 12), dtype=F), hs, CASES.draws(N, 0), trace=tr, tilt=tilt, act=act, lag_choice=ch)
        assert not tr[0]["air"].any() and (tilt or not np.array([s["air"] for s in tr]).any())      # (a tilting base may lose its support)
        assert list(tr[0]["crashed"]) == ([True, False, False] if crash else [False] * 3)
        assert list(new["crashed"]) == ([1, 0, 0] if crash else [0, 0, 0])
        force = np.zeros((N, 3), dtype=F)
        force[0, 2] = cfg.flight.crash_force if crash else 0
        assert np.array_equal(new["contact_forces"][:, 0], force)
        ko, otr = (AO if act else TO).config_dict(off, hs.shape[0], hs.shape[1]), []
        if act:
            old = AO.sim_step(st, ko, CASES.tables(off), np.zeros((N, 12), dtype=F), hs, CASES.draws(N, 0), trace=otr, tilt=tilt, lag_choice=ch)
        else:
            old = (TO if tilt else O).sim_step(st, ko, CASES.tables(off), np.zeros((N, 12), dtype=F), hs, CASES.draws(N, 0), trace=otr)
        assert np.array_equal(tr[0]["z"].view(np.uint32), otr[0]["base_z"].view(np.uint32))
        assert tr[0]["z"][0] > z0 + F(dz) - F(0.05) and tr[0]["z"][2] == z0
        if not tilt:
            assert np.array_equal(new["root_states"][:, 2].view(np.uint32), old["root_states"][:, 2].view(np.uint32))
        # a terrain discontinuity moves the base but gives it no momentum: (base_z - z) / dt is 30 m/s and more in the first substep
        assert (tr[0]["base_z"][0] - z0) / F(0.005) > 25 and abs(tr[0]["vz"]).max() == 0
        assert tilt or abs(new["root_states"][:, 9]).max() == 0
        s = dict(contact_forces=new["contact_forces"], termination_contact_indices=np.array([0]), episode_length_buf=new["episode_length_buf"],
                 projected_gravity=new["projected_gravity"], root_states=new["root_states"],
                 measured_heights=np.tile(new["root_states"][:, 2:3] - z0, (1, 693)).astype(F))
        reset, time_out, _ = check_termination(s, 1000)
        assert list(reset) == ([True, False, False] if crash else [False] * 3) and not time_out.any()


def test_take_off_at_the_joint_limit():
    """All four knees extend at 20 rad/s and reach their limit in the second substep: the stance legs leave the base 0.143 m/rad x
    ~20 rad/s of upward velocity, the support stops rising, and the base flies.  Airborne for at least one substep (here: 120);
    the apex (0.80 m) lies within 4 x the float32 run's largest z deviation from its float64 run of that run's apex (measured:
    deviation 4.69e-7 m over the flight -> bound 1.9e-6 m), and both runs land on the same substep."""
    cfg = FO.config(4)
    st = _rest(cfg, 21.0, _stand(cfg))
    t = CASES.tables(cfg)
    knee = np.arange(12) % 3 == 2
    st["dof_pos"][0, knee] = t["dof_pos_limits"][knee, 0] + F(0.1)
    st["dof_vel"][0, knee] = -20.0
    st["root_states"][0, 2] = 0.32                                                       # the support of the extended legs, about
    (r32, t32), (r64, t64) = _pair(cfg, st, _table(0.0), 40)
    air32, air64 = (np.array([s["air"][0] for s in tr]) for tr in (t32, t64))
    assert np.array_equal(air32, air64) and not air32[0] and air32.sum() >= 1 and not air32[-1]
    first, last = int(np.argmax(air32)), len(air32) - 1 - int(np.argmax(air32[::-1]))
    assert air32[first:last + 1].all()                                                   # one flight
    assert t32[first - 1]["vz"][0] > 1.5                                                 # the take-off velocity of the stance legs
    dev = _dev(t32[:last + 1], t64[:last + 1], "z")
    apex32, apex64 = (max(float(s["z"][0]) for s in tr) for tr in (t32, t64))
    print(f"take-off: {air32.sum()} airborne substeps, apex {apex64:.4f} m, float32 - float64 z deviation {dev:.3e} m")
    assert apex64 - float(t64[first - 1]["z"][0]) > 0.1 and 0 < dev < 1e-3
    assert abs(apex32 - apex64) <= 4 * dev
    assert r32[-1][5]["crashed"][0] == 0


@pytest.mark.parametrize("tilt,act", BASES, ids=IDS)
def test_flat_table_from_rest_is_the_flight_off_step(tilt, act):
    """Flat table, zero actions, from rest at the standing height: never airborne, never crashed, and every output that does not
    carry the vertical velocity equals the flight-off oracle's (numerically: a zero's sign may differ)."""
    cfg = FO.config(4, tilt, act)
    off = CASES.config(4, tilt=tilt, actuator=cfg.actuator)
    N, hs = 3, _table(0.0)
    st = _rest(cfg, np.array([21.0, 22.5, 24.0], dtype=F), _stand(cfg), N=N)
    old_st = {k: v for k, v in st.items() if k not in FO.FLAGS}
    zero = np.zeros((N, 12), dtype=F)
    for i in range(3):
        tr = []
        ch = AO.choices(4, i) if act else None
        new = FO.sim_step(st, FO.config_dict(cfg, hs.shape[0], hs.shape[1]), CASES.tables(cfg), zero, hs, CASES.draws(N, i), trace=tr, tilt=tilt,
                          act=act, lag_choice=ch)
        ko = (AO if act else TO).config_dict(off, hs.shape[0], hs.shape[1])
        if act:
            old = AO.sim_step(old_st, ko, CASES.tables(off), zero, hs, CASES.draws(N, i), tilt=tilt, lag_choice=ch)
        else:
            old = (TO if tilt else O).sim_step(old_st, ko, CASES.tables(off), zero, hs, CASES.draws(N, i))
        assert not np.array([s["air"] for s in tr]).any() and not new["airborne"].any() and not new["crashed"].any()
        for name, want in old.items():
            got, want = np.array(new[name], copy=True), np.array(want, copy=True)
            if name == "root_states":
                got[:, 9] = want[:, 9] = 0
            elif name == "base_lin_vel":
                got[:, 2] = want[:, 2] = 0
            elif name == "rigid_body_state":
                got[:, cfg.feet, 9] = want[:, cfg.feet, 9] = 0
            assert got.dtype == want.dtype and np.array_equal(got, want, equal_nan=True), (i, name)
        st, old_st = dict(st, **new), dict(old_st, **old)


def test_validate_rejects_each_bad_constant():
    from dtc_amd import sim as SIM
    SIM.FlightConfig().validate()
    SIM.FlightConfig(gravity=0.0, max_step_up=1e-3, crash_force=100.5).validate()
    for bad in (dict(gravity=-1.0), dict(gravity=float("nan")), dict(max_step_up=0.0), dict(max_step_up=-0.3), dict(max_step_up=float("inf")),
                dict(crash_force=100.0), dict(crash_force=50.0), dict(crash_force=float("nan"))):
        with pytest.raises(ValueError):
            SIM.FlightConfig(**bad).validate()
    d = SIM.FlightConfig()
    assert (d.gravity, d.max_step_up, d.crash_force) == (9.81, 0.3, 200.0) and SIM.SimConfig().flight is None


def test_the_abi_version_is_still_25_and_the_binding_declares_the_entry_point():
    import ctypes as C
    from dtc_amd import _ffi
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dtc_hip.h")).read()
    assert int(re.search(r"#define DTC_ABI_VERSION (\d+)", header).group(1)) == _ffi.ABI_VERSION == 25
    assert "dtc_sim_step_fly" in _ffi.exported_symbols() and "dtc_sim_fly_abi_sizes" in _ffi.exported_symbols()
    assert re.search(r"int dtc_sim_step_fly\(const DtcSimStep\* st, const DtcSimCfg\* cfg, const DtcSimTilt\* tilt_or_null", header)
    assert C.sizeof(_ffi.DtcSimFlight) == 32 and _ffi.DtcSimFlight.airborne.offset == 16 and _ffi.DtcSimFlight.crashed.offset == 24
