"""CPU: the float64 reward oracle (tests/golden/reward_oracle.py) reproduces the reference's compute_reward, captured in
tests/golden/rewards.npz by tests/golden/make_reward_golden.py, step by step; RewardConfig.from_cfg resolves the scales as the
reference's _prepare_reward_function does; and the per-term measure of tests/reward_cases.py, which holds csrc/rewards.hip to the
oracle in tests/test_hip_rewards.py, is a usable yardstick: the oracle's own fp32 run stays inside the cap on every case, the
measure sees a spoiled term that the earlier max(1, |ref|) measure let through, and no case checks a term that is zero.

test_oracle_reproduces_reference: the fixture is the reference's own fp32 run, so the oracle is held to it per term in the measure
of reward_cases, against max(2^-20, 8 * e32) with e32 from the oracle's fp32 run on the fixture's inputs; 29.8 * e32 for the plane-fit
quantities (_plane_fit_factor below).  The step with the largest error of the 6, per config, on one CPU (air / pitch = the carried
feet_air_time / pitch_est); the episode sums per term are held the same way, the closest being sums:pos_acc (lite3) at
2.3/1.4/11.6:

error / e32 / bound (1e-7)                       lite3                     x30                     all
rew                                       7.3/7.8/62.0            3.3/2.7/21.3      117.6/140.9/1127.1
action_rate                               3.0/2.0/15.7            2.1/2.2/17.6            2.5/2.3/18.3
ang_vel_xy                                1.2/1.2/10.0            1.3/1.3/10.6            1.3/1.3/10.3
base_height                            25.5/25.5/204.2            2.2/2.2/17.9         30.5/23.1/184.5
dof_acc                                   1.9/2.5/19.9            2.1/2.2/17.5            2.4/2.5/19.7
dof_pos_limits                             0.9/1.0/9.5             0.7/0.7/9.5             0.7/0.6/9.5
feet_air_time                          12.9/18.4/147.1         24.7/26.7/213.7         33.9/27.6/221.2
feet_slip                                 2.2/1.4/11.5                       -            1.8/2.0/16.0
foot_acc                                  2.2/4.0/31.9                       -            7.6/7.6/61.2
hip_pos                                   1.5/1.5/12.2                       -            1.6/1.7/13.7
lin_vel_z                                  0.9/0.9/9.5             0.9/1.0/9.5             0.9/0.9/9.5
orientation                             51.9/7.5/223.0          50.9/9.7/288.7          64.6/7.5/224.3
pos_acc                                   2.3/1.4/11.6            1.7/1.6/13.1            1.7/1.6/12.5
power                                     1.5/1.6/12.5                       -            1.6/1.6/13.0
powerchange                               3.8/4.3/34.4            5.4/4.3/34.6            4.0/4.4/35.5
smooth                                    2.9/2.7/21.8                       -            2.5/2.5/20.4
soft_tracking_ang_vel                      0.9/0.9/9.5                       -             0.7/0.7/9.5
soft_tracking_lin_vel                     3.4/5.0/40.2                       -            3.8/5.9/47.4
stand_still                               1.3/1.4/11.6                       -            1.7/1.5/12.2
torques                                   1.8/1.8/14.7                       -            2.0/2.0/15.8
tracking_optimal_footholds          174.4/157.7/1261.4      328.3/343.2/2745.6      249.5/249.1/1993.0
air                                       1.4/1.9/14.8            1.6/1.8/14.1            1.9/1.9/15.3
pitch                                  72.4/22.6/675.2         41.9/18.4/549.3          21.9/3.6/106.3
dof_vel                                              -            1.9/2.5/19.8            2.1/2.1/16.6
feet_contact_forces                                  -            7.8/7.2/57.8            9.0/9.1/73.0
tracking_ang_vel                                     -            0.8/1.6/13.0            0.8/1.4/10.9
tracking_lin_vel                                     -            8.4/8.5/68.1            6.8/7.6/60.9
dof_vel_limits                                       -                       -             1.0/1.0/9.5
orientation_roll                                     -                       -       115.6/39.9/1188.6
torque_limits                                        -                       -             1.0/1.0/9.5
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import reward_cases as K  # noqa: E402
import reward_oracle as O  # noqa: E402
from dtc_amd import synthetic as S  # noqa: E402
from dtc_amd.rewards import EnvRewards, RewardConfig, TERMS  # noqa: E402
from reward_cases import cfg_from_fixture, oracle_cfg  # noqa: E402,F401  (tests/test_hip_rewards.py takes them from here)

TAGS = K.TAGS


def _plane_fit_factor():
    """The multiple of e32 for the fixture's plane-fit quantities.  The reference fits the height plane per env through the normal
    equations in fp32 (legged_robot.py:1535-1557): A1 = A^T A, A2 = inv(A1), A3 = A2 A^T, X = A3 h.  The oracle (and the kernel)
    take the constant float64 rows of (A^T A)^-1 A^T, so the oracle's fp32 run shows the rounding of the last product only.  The
    rounding of A1 and that of its inverse reach the slopes amplified by up to cond(A^T A) each (10.9 on the 33 x 21 grid), which
    e32 does not see: the fixture's orientation, orientation_roll and pitch_est are held to (8 + 2 cond) e32 = 29.8 e32 instead
    of 8 e32, the cap unchanged.  From the grid alone; no measured error enters."""
    x = np.asarray(S.MEASURED_POINTS_X, dtype=np.float32).astype(np.float64)
    y = np.asarray(S.MEASURED_POINTS_Y, dtype=np.float32).astype(np.float64)
    gx, gy = np.meshgrid(x, y, indexing="ij")
    A = np.stack([gx.ravel(), gy.ravel(), np.ones(gx.size)], axis=1)
    return K.FACTOR + 2.0 * float(np.linalg.cond(A.T @ A))


PLANE_FIT_FACTOR = {k: _plane_fit_factor() for k in ("orientation", "orientation_roll", "pitch", "sums:orientation",
                                                     "sums:orientation_roll")}


def fixture_bound(key, e32):
    """The bound of a quantity compared with the fixture (the oracle on the CPU, the kernel on the GPU): max(2^-20, 8 * e32), the
    plane-fit quantities with their own multiple; the cap holds for the bound as it is used."""
    b = max(K.FLOOR, PLANE_FIT_FACTOR.get(key, K.FACTOR) * e32)
    assert b <= K.CAP, (key, e32, b)
    return b


@pytest.fixture(scope="module")
def fx(golden):
    return golden("rewards")


def run_oracle_sequence(cfg, N, steps, seed, wp=np.float64, fresh=S.reward_state):
    """Yields (rew, per_term dict, episode sums before the reset, env) per step of the fixture's sequence, in working precision
    `wp` (the carried float state included)."""
    F = list(cfg["feet_indices"])
    env = O.seq_begin(fresh(N, seed=seed), F)
    env.update({k: env[k].astype(wp) for k in ("feet_air_time", "pitch_est")})
    sums = {n: np.zeros(N, dtype=wp) for n in cfg["scales"]}
    for t in range(steps):
        rew, per = O.compute_reward(env, cfg, env, sums, wp)
        yield rew, per, {k: v.copy() for k, v in sums.items()}, env
        O.seq_reset(env, sums)
        if t + 1 < steps:
            O.seq_next(env, fresh(N, seed=seed + t + 1), F)


def sequence_e32(cfg, N, steps, seed):
    """-> (the float64 steps, e32 per step: {term / "rew" / "air" / "pitch" / "sums:<term>": e32}); the yielded env is copied where
    it is needed later."""
    keep = lambda rew, per, sums, env: dict(rew=rew, per=per, sums=sums, st={k: env[k].copy() for k in O.STATE})   # noqa: E731
    r64 = [keep(*s) for s in run_oracle_sequence(cfg, N, steps, seed)]
    r32 = [keep(*s) for s in run_oracle_sequence(cfg, N, steps, seed, np.float32)]
    e32 = []
    for a, b in zip(r64, r32):
        e = K.e32_of(b, a)
        e.update({"sums:" + n: K.term_err(b["sums"][n], a["sums"][n]) for n in a["sums"] if n not in O.DISCRETE})
        e32.append(e)
    return r64, e32


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
    names = rc.names
    r64, e32 = sequence_e32(oracle_cfg(rc), N, steps, seed)
    worst, over = {}, {}

    def hold(key, t, got, ref, e):
        err, b = K.term_err(got, ref), fixture_bound(key, e)
        if err >= worst.get(key, (-1.0,))[0]:
            worst[key] = (err, e, b)
        if not err <= b:
            over[key, t] = (err, e, b)

    for t, (r, e) in enumerate(zip(r64, e32)):
        hold("rew", t, r["rew"], fx[f"{tag}_rew_{t}"], e["rew"])
        ref_per, ref_sums = fx[f"{tag}_per_{t}"], fx[f"{tag}_sums_{t}"]
        for i, n in enumerate(names):
            got = r["per"][n][::stride]
            if n in O.DISCRETE:
                sc = rc.scales[n]
                np.testing.assert_array_equal(got / sc, np.round(ref_per[i].astype(np.float64) / sc), err_msg=f"{tag} step {t} {n}")
                np.testing.assert_array_equal(np.round(r["sums"][n][::stride] / sc), np.round(ref_sums[i].astype(np.float64) / sc),
                                              err_msg=f"{tag} step {t} sums of {n}")
            else:
                hold(n, t, got, ref_per[i], e[n])
                hold("sums:" + n, t, r["sums"][n][::stride], ref_sums[i], e["sums:" + n])
        np.testing.assert_array_equal(np.packbits(r["st"]["last_contacts"]), fx[f"{tag}_contacts_{t}"])
        np.testing.assert_array_equal(r["st"]["stumble"], fx[f"{tag}_stumble_{t}"])
        hold("air", t, r["st"]["feet_air_time"][::4], fx[f"{tag}_air_{t}"], e["air"])
        hold("pitch", t, r["st"]["pitch_est"][::2], fx[f"{tag}_pitch_{t}"], e["pitch"])
    print(f"\n{tag} oracle against the fixture, error / e32 / bound (1e-7):\n" +
          "\n".join(f"  {k:36s} {v[0] * 1e7:8.1f} /{v[1] * 1e7:8.1f} /{v[2] * 1e7:8.1f}" for k, v in worst.items()))
    assert not over, over
    assert all(K.FACTOR * max(e.values()) <= K.CAP for e in e32)


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


# ------------------------------------------------------------------------------------------- the oracle's working precision
def _all_terms_env(N=256, seed=5):
    rc = RewardConfig(scales={n: K.SCALE for n in TERMS}, max_acc=100.0, only_positive_rewards=True)
    return rc, K.lite3_state(N, seed)


RECORDED_TOL = 1e-11


def test_float64_results_are_the_recorded_ones(fx, golden):
    """The float64 oracle is the one from before it took a working precision: tests/golden/reward_oracle_f64.npz holds what that
    version returned for the `all` config on reward_state(64, seed=5) from linspace sums -- rew, per_term, the sums and the float
    state, once with the env's own fp32 state arrays (`env`: the way the tests called it then) and once with float64 state
    (`f64`).  Compared in the per-term measure at 1e-11: numpy's exp / log / arctan and the BLAS product of the plane fit may
    differ in the last bits from one CPU to the next, a step done in fp32 would show at 1e-8.  The default and wp=float64 are the
    same call, bit for bit, and everything that comes back is float64 (feet_air_time on fp32 state excepted, as recorded)."""
    rec = golden("reward_oracle_f64")
    rc, N = K.fixture_rc(fx, "all"), 64
    cfg, env = oracle_cfg(rc), K.lite3_state(N, 5)
    for tag, st0 in (("env", {k: env[k].copy() for k in O.STATE}), ("f64", O.state(env))):
        runs = []
        for kw in ({}, dict(wp=np.float64)):
            st = {k: v.copy() for k, v in st0.items()}
            sums = {n: K.linspace_sums(len(rc.names), N)[i].astype(np.float64) for i, n in enumerate(rc.names)}
            rew, per = O.compute_reward(env, cfg, st, sums, **kw)
            runs.append(dict(rew=rew, per=per, sums=sums, air=st["feet_air_time"], pitch=st["pitch_est"]))
        a, b = runs
        assert a["rew"].tobytes() == b["rew"].tobytes() and a["rew"].dtype == np.float64 and a["pitch"].dtype == np.float64
        assert a["air"].dtype == (np.float32 if tag == "env" else np.float64)
        assert K.term_err(a["rew"], rec[tag + "_rew"]) <= RECORDED_TOL
        assert K.term_err(a["air"], rec[tag + "_air"]) <= RECORDED_TOL and K.term_err(a["pitch"], rec[tag + "_pitch"]) <= RECORDED_TOL
        for i, n in enumerate(rc.names):
            assert a["per"][n].tobytes() == b["per"][n].tobytes() and a["sums"][n].tobytes() == b["sums"][n].tobytes(), (tag, n)
            assert a["sums"][n].dtype == np.float64 and (a["per"][n].dtype == np.float64 or (tag, n) == ("env", "feet_air_time"))
            assert K.term_err(a["per"][n], rec[tag + "_per"][i]) <= RECORDED_TOL, (tag, n)
            assert K.term_err(a["sums"][n], rec[tag + "_sums"][i]) <= RECORDED_TOL, (tag, n)


@pytest.mark.parametrize("numpy_config", [False, True])
def test_float32_mode_is_float32_throughout(numpy_config):
    """Every per-term output, rew, the sums and the float state of the fp32 run have dtype float32 -- also when the config holds
    numpy float64 scalars (which would otherwise promote an fp32 array)."""
    rc, env = _all_terms_env()
    cfg = oracle_cfg(rc)
    if numpy_config:
        cfg = {k: (np.float64(v) if isinstance(v, float) else v) for k, v in cfg.items()}
        cfg["scales"] = {n: np.float64(v) for n, v in cfg["scales"].items()}
    st, sums = O.state(env, np.float32), {n: np.zeros(256, dtype=np.float32) for n in rc.names}
    rew, per = O.compute_reward(env, cfg, st, sums, np.float32)
    assert rew.dtype == np.float32 and st["feet_air_time"].dtype == np.float32 and st["pitch_est"].dtype == np.float32
    assert {n: v.dtype for n, v in per.items() if v.dtype != np.float32} == {} and sorted(per) == sorted(TERMS)
    assert {n: v.dtype for n, v in sums.items() if v.dtype != np.float32} == {}
    for n in TERMS:
        assert O.term(n, env, cfg, O.state(env, np.float32), np.float32).dtype == np.float32, n
    # and it is the same computation: within fp32 rounding of the float64 run, discrete terms equal
    r64 = K.run_oracle(env, oracle_cfg(rc), np.zeros((len(rc.names), 256)), np.float64)
    for n in TERMS:
        if n in O.DISCRETE:
            np.testing.assert_array_equal(per[n], r64["per"][n].astype(np.float32), err_msg=n)
        else:
            assert K.term_err(per[n], r64["per"][n]) <= K.CAP / K.FACTOR, n


# ------------------------------------------------------------------------------------------------------- the measure itself
def test_measure_edges():
    assert K.term_err(np.zeros(4), np.zeros(4)) == 0.0 and K.term_err([0.0, 1e-30], np.zeros(2)) == float("inf")
    assert K.term_err([1.0, 1e-4 + 1e-6], [1.0, 1e-4]) == pytest.approx(1e-6 / 1e-2)          # small rows: 1 % of the largest
    assert K.term_err([2.0 + 2e-3, 1.0], [2.0, 1.0]) == pytest.approx(1e-3)
    assert np.isnan(K.term_err([np.nan, 1.0], [1.0, 1.0])) and not np.nan <= K.bound(0.0)
    assert K.bound(0.0) == 2.0 ** -20 and K.bound(1e-6) == 8e-6


@pytest.fixture(scope="module")
def single_steps(fx):
    """(label, config, float64 run, e32) of every one-launch case of the GPU tests."""
    out = []
    for label, rc, layout, env, sums0 in K.single_step_cases(fx):
        r64, e32 = K.reference(env, oracle_cfg(rc, layout), sums0)
        out.append((label, rc, r64, e32, len(sums0[0])))
    return out


def test_reference_alone_stays_inside_the_cap(fx, single_steps):
    """8 * e32 <= CAP for every continuous term, rew and the float state of every case: the inputs are ones on which the float64
    oracle is a yardstick to a few 1e-5 at worst."""
    over, worst = {}, {}
    for label, rc, r64, e32, N in single_steps:
        for k, e in e32.items():
            worst[k] = max(worst.get(k, 0.0), e)
            if not K.FACTOR * e <= K.CAP:
                over[label, k] = e
    for tag in K.TWENTY["tags"]:
        _, seq = sequence_e32(oracle_cfg(K.fixture_rc(fx, tag)), K.TWENTY["N"], K.TWENTY["steps"], K.TWENTY["seed"])
        for t, e32 in enumerate(seq):
            for k, e in e32.items():
                worst[k] = max(worst.get(k, 0.0), e)
                if not K.FACTOR * e <= K.CAP:
                    over[f"{tag} step {t}", k] = e
    print("\nworst e32 over all cases: " + " ".join(f"{k}={v:.1e}" for k, v in sorted(worst.items(), key=lambda kv: -kv[1])[:8]))
    assert not over, over


def test_no_case_is_vacuous(fx, single_steps):
    """At N >= 1024 every continuous term is nonzero in at least 10 % of the rows and every discrete term takes at least two
    counts; the small cases (one term alone, the term sets, the other shapes: N = 67) still have a nonzero row per term."""
    # a shape with no penalised body / no hip has a collision / hip_pos term that is zero by construction, and only that shape
    empty = {key: [t for t, count in (("collision", v[4]), ("hip_pos", len(v[5]))) if count == 0] for key, v in K.SHAPES.items()}
    assert sorted(k for k, v in empty.items() if v) == ["dof1-body5-cmd3-grid2x2", "dof13-body5-cmd5-grid13x5"]
    for label, rc, r64, e32, N in single_steps:
        for n in rc.names:
            v = r64["per"][n]
            if N >= 1024:
                if n in O.DISCRETE:
                    assert len(np.unique(v)) >= 2, (label, n)
                else:
                    assert np.count_nonzero(v) >= 0.1 * N, (label, n, np.count_nonzero(v) / N)
            elif N == K.ALONE_N and not (n in empty.get(label.split(" N=")[0], ())):
                assert np.count_nonzero(v) >= 1, (label, n)


def test_new_measure_sees_what_the_old_one_did_not(fx):
    """Every continuous term of every fixture config, spoiled (a) by a factor 1 + 2e-3 and (b) by one dof / foot / component taken
    out of its sum: the per-term measure exceeds the cap; the earlier measure, max |got - ref| / max(1, |ref|) <= 4e-6, passes
    both for power (lite3, all) and dof_vel (x30) -- it also passes power replaced by 0."""
    N = 4099
    blind = set()
    for tag in TAGS:
        rc = K.fixture_rc(fx, tag)
        cfg = oracle_cfg(rc)
        env = K.lite3_state(N, 11 + N)
        for n in rc.names:
            if n in O.DISCRETE:
                continue
            sc = rc.scales[n]
            ref = O.term(n, env, cfg, O.state(env)) * sc
            spoiled = {"scaled": ref * (1.0 + 2e-3)}
            env2, st2 = {k: v.copy() for k, v in env.items()}, O.state(env)
            if K.drop_one(n, env2, st2):
                spoiled["dropped"] = O.term(n, env2, cfg, st2) * sc
            for how, got in spoiled.items():
                assert K.term_err(got, ref) > K.CAP, (tag, n, how, K.term_err(got, ref))
            if all(K.old_err(got, ref) <= K.OLD_BOUND for got in spoiled.values()) and len(spoiled) == 2:
                blind.add((tag, n))
            if n == "power":
                assert K.old_err(np.zeros(N), ref) <= K.OLD_BOUND and K.term_err(np.zeros(N), ref) > K.CAP
    assert {("lite3", "power"), ("all", "power"), ("x30", "dof_vel")} <= blind, blind


# -------------------------------------------------------------------------------------------------- refusals, no device needed
@pytest.mark.parametrize("kw", [dict(num_dof=65), dict(num_dof=0), dict(penalised_contact_indices=tuple(range(33)), num_dof=64),
                                dict(hip_indices=tuple(range(17)), num_dof=64), dict(feet_indices=(4, 8, 12))],
                         ids=["65 dofs", "0 dofs", "33 penalised bodies", "17 hips", "3 feet"])
def test_env_rewards_refuses_unsupported_shapes(kw):
    """One limit over at a time (EnvRewards names all of them in one message); the neighbour inside the limit is accepted."""
    args = dict(feet_indices=S.REWARD_FEET, penalised_contact_indices=S.REWARD_PENALISED, hip_indices=S.REWARD_HIPS)
    rc = RewardConfig(scales={"torques": K.SCALE})
    with pytest.raises(ValueError, match="4 feet, <= 32 penalised bodies, <= 16 hip dofs and 1..64 dofs"):
        EnvRewards(8, "cpu", rc, **{**args, **kw})
    inside = dict(num_dof=64, penalised_contact_indices=tuple(range(32)), hip_indices=tuple(range(16)))
    assert EnvRewards(8, "cpu", rc, **{**args, **inside}).num_dof == 64


@pytest.mark.parametrize("field, value, needle", [("num_dof", 65, b"num_dof 65 outside"), ("num_dof", 0, b"num_dof 0 outside"),
                                                  ("n_penalised", 33, b"index lists too long"), ("n_hip", 17, b"index lists too long")])
def test_dtc_env_rewards_refuses_before_any_launch(field, value, needle):
    """The entry point checks the descriptor before it looks at a pointer: with every buffer NULL and N > 0 the answer is the
    shape error, not `null pointer` -- nothing was read and nothing launched."""
    from dtc_amd import _ffi
    lib = _ffi.lib()
    c, st = _ffi.DtcRewardCfg(), _ffi.DtcRewardStep()
    for i in range(_ffi.REWARD_TERMS):
        c.row[i] = -1
    c.scale[TERMS.index("torques")], c.row[TERMS.index("torques")] = K.SCALE, 0
    c.num_dof, c.n_penalised, c.n_hip, c.num_points = 12, 9, 4, 693
    st.num_bodies, st.num_commands = 17, 4
    assert lib.dtc_env_rewards(st, c, 64, None) == -1 and b"null pointer" in lib.dtc_last_error()       # the descriptor is sound
    setattr(c, field, value)
    assert lib.dtc_env_rewards(st, c, 64, None) == -1
    assert needle in lib.dtc_last_error(), lib.dtc_last_error()
