"""The any-grid oracle (oracle/foothold.py) against an independent float64 restatement of the reference block, against
the fixture recorded from the reference on two other grids (tests/golden/scorer_grids.npz), and the host-side path
decision of the planner (dtc_foothold_grid_info).  CPU only.

`f64_plan` below is written from legged_gym/envs/base/legged_robot_dtc.py:98-201 with torch's own operators
(torch.gradient(spacing=0.05), torch.mean, torch.var, topk(k=1, largest=False)) in float64; it shares no code with
oracle/foothold.py.  Knife-edge policy: the two may pick different indices only where the float64
runner-up gap is <= 1e-5."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import cases as C  # noqa: E402


# ------------------------------------------------------------------------------------------------ float64 restatement
def _quat_rotate_inverse(q, v):
    q_w, q_vec = q[:, -1], q[:, :3]
    a = v * (2.0 * q_w ** 2 - 1.0).unsqueeze(-1)
    b = torch.cross(q_vec, v, dim=-1) * q_w.unsqueeze(-1) * 2.0
    c = q_vec * (q_vec * v).sum(-1, keepdim=True) * 2.0
    return a - b + c


def _quat_apply_yaw(q, vec):
    qy = q.clone()
    qy[:, :2] = 0.0
    qy = qy / qy.norm(p=2, dim=-1, keepdim=True).clamp(min=1e-9)
    xyz = qy[:, :3]
    t = torch.cross(xyz, vec, dim=-1) * 2
    return vec + qy[:, 3:] * t + torch.cross(xyz, t, dim=-1)


def f64_plan(inp, X, Y, t_stance=0.005 * 4):
    d = torch.float64
    mh, root = inp["measured_heights"].to(d), inp["root_states"].to(d)
    hip, cmd = inp["thigh_pos"].to(d), inp["commands"].to(d)
    X, Y = torch.as_tensor(np.asarray(X, dtype=np.float32)).to(d), torch.as_tensor(np.asarray(Y, dtype=np.float32)).to(d)
    N, nx, ny = mh.shape[0], len(X), len(Y)
    base_pos, base_quat = root[:, :3], root[:, 3:7]
    base_lin_vel = _quat_rotate_inverse(base_quat, root[:, 7:10])
    # :100-120
    hip_to_base = hip - base_pos.unsqueeze(1)
    th = cmd[:, 2]
    zeros, ones = torch.zeros_like(th), torch.ones_like(th)
    Rz = torch.stack([torch.cos(th), -torch.sin(th), zeros, torch.sin(th), torch.cos(th), zeros, zeros, zeros, ones], dim=1).reshape(-1, 3, 3)
    p_shoulder = base_pos.unsqueeze(1) + torch.bmm(Rz, hip_to_base.transpose(1, 2)).transpose(1, 2)
    cmd_lin = torch.cat((cmd[:, :2], torch.zeros(N, 1, dtype=d)), dim=1)
    p_sym = t_stance / 2 * base_lin_vel.unsqueeze(1) + 0.03 * (base_lin_vel.unsqueeze(1) - cmd_lin.unsqueeze(1))
    pred = p_shoulder + p_sym
    # :127-148
    grid = (mh - base_pos[:, 2:3]).view(N, nx, ny)
    exception = (grid > 1) | (grid < -1)
    grid = grid.clamp(min=-0.5, max=0.5)
    d_x, d_y = torch.gradient(grid, dim=[1, 2], spacing=0.05)
    slope = torch.sqrt(d_x ** 2 + d_y ** 2)
    rough = torch.abs(grid - torch.mean(grid, dim=(1, 2)).view(N, 1, 1))
    edge = torch.sqrt(torch.var(grid, dim=(1, 2))).view(N, 1, 1).clamp(min=0.0, max=0.3)
    score = (0.2 * edge + 1 * slope + 0.3 * rough).view(N, -1)
    score = torch.where(score < 0.1, score, torch.tensor(10.0, dtype=d))
    # :152-175
    gx, gy = torch.meshgrid(X, Y, indexing="ij")
    pts = torch.stack([gx.flatten(), gy.flatten(), torch.zeros(nx * ny, dtype=d)], dim=1)
    hw = _quat_apply_yaw(base_quat.repeat(1, nx * ny).view(-1, 4), pts.repeat(N, 1)).view(N, -1, 3) + base_pos.unsqueeze(1)
    hw[:, :, 2] = mh
    dis = torch.norm(pred.unsqueeze(1)[:, :, :, :-1] - hw.unsqueeze(2)[:, :, :, :-1], dim=-1)
    dis = torch.where(dis < 0.16, dis, torch.tensor(10.0, dtype=d))
    total = score.unsqueeze(2) * 0.2 + dis * 0.8
    total = torch.where(exception.view(N, -1).unsqueeze(2), torch.tensor(10.0, dtype=d), total)
    # :180-201
    idx = torch.topk(total, k=1, dim=1, largest=False, sorted=True)[1]
    x_i, y_i = torch.remainder(idx, ny), torch.div(idx, ny, rounding_mode="trunc")
    obs = torch.cat((torch.gather(X.view(1, 1, -1).repeat(N, 1, 4), -1, x_i), torch.gather(Y.view(1, 1, -1).repeat(N, 1, 4), -1, y_i)),
                    dim=-2).view(N, -1)
    idx = idx.squeeze(1)
    world = hw[torch.arange(N).unsqueeze(-1).expand_as(idx), idx]
    srt = torch.sort(total, dim=1)[0]
    return dict(idx=idx.numpy(), obs=obs.numpy(), world=world.numpy(), gap=(srt[:, 1] - srt[:, 0]).numpy(), total=total.numpy())


def _oracle(inp, X, Y, debug=False):
    from oracle import foothold as OF
    return OF.plan(inp["measured_heights"].numpy(), inp["root_states"].numpy(), inp["thigh_pos"].numpy(),
                   inp["commands"].numpy(), X, Y, want_debug=debug)


# (env, leg) pairs per grid on which the oracle and the float64 restatement may pick different indices (all of them knife
# edges, gap <= 1e-5): what the seeds of cases.planner_cases give, measured on the CPU.  The rule is <= 4 per 1000 pairs
# (5320 pairs per grid -> at most 21; 120 pairs on the two largest grids -> 0).
F64_KNIFE_EDGES = {"17x11@0.05": 0, "17x11@0.1": 1, "9x8@0.05": 1, "9x7@0.05": 0, "13x9@0.047": 0, "13x9@0.046": 0, "2x2": 0,
                   "8x16@0.05": 0, "63x32@0.025": 0, "64x32@0.025": 0, "33x21": 0, "33x21-cubic": 0, "33x21-reversed": 0}


# Left out of the float64 comparison (the GPU tests run it against the oracle like every other case): the 2 x 2 grid on the
# `exceptions` kind.  With four points, 40 % of them exceptional and any height step making a point invalid, most of its
# totals are EXACT ties at the sentinel 10.0, in float64 as in float32.  The oracle and the kernels resolve a tie to the
# lowest index, which is what torch.topk does on the CPU for P >= 64; below that its CPU path picks an unspecified element
# (measured: an all-tied column gives index 2 at P = 4 and 41 at P = 63), so there the two differ on 76 of 1064 pairs by
# the tie rule alone -- nothing the 4-per-1000 cap is meant to let through or to catch.
TOPK_TIE_CASES = {("2x2", "exceptions")}


@pytest.mark.parametrize("name", C.PLANNER_GRIDS)
def test_oracle_matches_float64_restatement(name):
    """Measured knife-edge counts (oracle index != float64 index, float64 gap <= 1e-5), per grid over all its cases:
    17x11@0.1: 1, 9x8@0.05: 1, every other grid 0 (F64_KNIFE_EDGES above; the test asserts exactly those caps)."""
    X, Y = C.planner_grid(name)
    n_mism = n_pairs = 0
    for N, kind, seed in C.planner_cases(name):
        if (name, kind) in TOPK_TIE_CASES:
            continue
        inp = C.planner_inputs(N, X, Y, seed, kind)
        o, r = _oracle(inp, X, Y), f64_plan(inp, X, Y)
        mism = np.argwhere(o["idx"] != r["idx"])
        for e, l in mism:
            assert r["gap"][e, l] <= 1e-5, (name, N, kind, e, l, o["idx"][e, l], r["idx"][e, l], r["gap"][e, l])
        n_mism += len(mism)
        n_pairs += 4 * N
        ok = np.ones((N, 4), bool)
        ok[mism[:, 0], mism[:, 1]] = False
        ok8 = np.concatenate([ok, ok], axis=1)
        np.testing.assert_array_equal(o["foothold_obs"].astype(np.float64)[ok8], r["obs"][ok8])         # table values
        np.testing.assert_array_equal(o["optimal_footholds_world"][:, :, 2].astype(np.float64)[ok], r["world"][:, :, 2][ok])
        np.testing.assert_allclose(o["optimal_footholds_world"][:, :, :2][ok], r["world"][:, :, :2][ok], rtol=0, atol=4e-6)
    print(f"{name}: {n_mism} knife-edge index differences on {n_pairs} (env, leg) pairs")
    assert n_mism <= F64_KNIFE_EDGES[name] <= 4 * n_pairs / 1000


# ------------------------------------------------------------------------------------------------ reference fixture
@pytest.mark.parametrize("tag", [t for t, _, _ in C.SCORER_GRID_CASES])
def test_oracle_matches_reference_on_other_grids(golden, tag):
    """The oracle against the imported reference run on 17 x 11 at 0.1 m and 8 x 16 at 0.05 m (512 envs each).  Index
    mismatches only where the recorded runner-up gap is <= 1e-5, at most 4 per case (measured when recording: 0 and 0)."""
    g = golden("scorer_grids")
    X, Y, inp = C.scorer_grid_inputs(tag)
    o = _oracle(inp, X, Y, debug=True)
    ref = g[tag + "_idx"].astype(np.int64)
    mism = np.argwhere(ref != o["idx"])
    for e, l in mism:
        assert g[tag + "_gap"][e, l] <= 1e-5, (e, l, ref[e, l], o["idx"][e, l])
    print(f"{tag}: {len(mism)} knife-edge index differences")
    assert len(mism) <= 4
    np.testing.assert_array_equal(o["nominal_idx"], g[tag + "_nominal_idx"].astype(np.int64))
    ok = np.ones(len(ref), bool)
    ok[mism[:, 0]] = False
    sub = ok[::4]
    np.testing.assert_array_equal(o["foothold_obs"][::4][sub], g[tag + "_foothold_obs"][sub])
    np.testing.assert_allclose(o["optimal_footholds_world"][::4][sub], g[tag + "_world"][sub], rtol=0, atol=4e-6)
    np.testing.assert_allclose(o["pred_footholds"][::4], g[tag + "_pred"], rtol=0, atol=4e-6)
    np.testing.assert_allclose(o["pred_footholds_to_robot"][::4], g[tag + "_pred_to_robot"], rtol=0, atol=4e-6)
    # slopes reach 20 (a clamped 1 m step over 0.05 m), where one float32 ulp is 1.9e-6: two ulp relative on top of the
    # absolute 1e-6 of the 33 x 21 test (the quotients and the square root are each correctly rounded on either side;
    # torch.gradient may scale by a reciprocal where the oracle divides)
    np.testing.assert_allclose(o["slope"][::64], g[tag + "_slope_sample"], rtol=2.4e-7, atol=1e-6)
    np.testing.assert_allclose(o["foothold_score"][::64], g[tag + "_score_sample"], rtol=0, atol=1e-5)


# ------------------------------------------------------------------------------------------------ host-side path decision
def _info(X, Y):
    from dtc_amd import foothold
    return foothold.grid_info(foothold.GridConfig(tuple(float(v) for v in X), tuple(float(v) for v in Y)))


def patch_start(X, Y, lx, ly):
    """First cell (sx, sy) of the 8 x 8 candidate patch as make_params / the kernels place it for a nominal foothold
    (lx, ly) in the grid's frame -- the float32 formulas of csrc/foothold.hip, assuming a uniform increasing table."""
    f = np.float32
    X, Y = np.asarray(X, dtype=f), np.asarray(Y, dtype=f)
    inv_dx, inv_dy = f(len(X) - 1) / (X[-1] - X[0]), f(len(Y) - 1) / (Y[-1] - Y[0])
    rad_x, rad_y = f(0.16) * inv_dx + f(0.05), f(0.16) * inv_dy + f(0.05)
    u, v = (np.asarray(lx, dtype=f) - X[0]) * inv_dx, (np.asarray(ly, dtype=f) - Y[0]) * inv_dy
    return (np.floor(u - rad_x) + 1).astype(np.int64), (np.floor(v - rad_y) + 1).astype(np.int64)


def test_grid_info_path_decision():
    """Uniform float32 linspace tables stay patch-eligible; the cubic and the reversed tables, and 13 x 9 at 0.046 m
    (2 * rad = 7.06 cells), are not; LDS bytes and the fast-kernel flag as documented."""
    eligible = {"17x11@0.05": True, "17x11@0.1": True, "9x8@0.05": True, "13x9@0.047": True, "13x9@0.046": False, "2x2": True,
                "8x16@0.05": True, "63x32@0.025": False, "64x32@0.025": False, "33x21": True, "33x21-cubic": False,
                "33x21-reversed": False,
                "9x7@0.05": True}       # eligible by placement, but ny < 8: the generic kernel never uses the patch there
    assert set(eligible) == set(C.PLANNER_GRIDS)
    for name, want in eligible.items():
        X, Y = C.planner_grid(name)
        i = _info(X, Y)
        assert i["patch_ok"] == want, (name, i)
        assert i["num_points"] == len(X) * len(Y)
        assert i["lds_bytes"] == (2 * ((4 * len(X) * len(Y) + 3) & ~3) + 96) * 4
        assert i["fast"] == (len(X) == 33 and len(Y) == 21 and not os.environ.get("DTC_PLANNER_GENERIC"))
    assert _info(*C.planner_grid("63x32@0.025"))["lds_bytes"] == 64896
    assert _info(*C.planner_grid("64x32@0.025"))["lds_bytes"] == 65920
    from dtc_amd import synthetic as S
    assert _info(S.MEASURED_POINTS_X, S.MEASURED_POINTS_Y)["patch_ok"]          # the reference's own (rounded decimal) tables
    # the uniformity bound: a single entry 0.02 cells off keeps the patch, 0.04 cells off loses it
    X, Y = C.planner_grid("17x11@0.05")
    for dev, want in ((0.02, True), (0.04, False)):
        Xd = X.copy()
        Xd[5] += np.float32(dev * 0.05)
        assert _info(Xd, Y)["patch_ok"] == want, dev
        Yd = Y.copy()
        Yd[3] -= np.float32(dev * 0.05)
        assert _info(X, Yd)["patch_ok"] == want, dev
    # monotonic but not strictly: two equal entries
    Xd = X.copy()
    Xd[4] = Xd[5]
    assert not _info(Xd, Y)["patch_ok"]
    from dtc_amd import _ffi
    assert _ffi.lib().dtc_foothold_grid_info(None, None) == -1


def test_uniform_placement_misses_in_radius_points_only_on_nonuniform_tables():
    """The defect the uniformity rule closes, on the CPU: place the patch by the uniform-table formulas for random nominal
    footholds and count those with an in-radius grid point (|x - lx| < 0.16 and |y - ly| < 0.16 bound the disc) outside it."""
    rng = np.random.default_rng(5)
    for name in C.PLANNER_GRIDS:
        X, Y = C.planner_grid(name)
        if not (name in ("33x21-cubic", "33x21-reversed") or _info(X, Y)["patch_ok"]):
            continue
        lo_x, hi_x, lo_y, hi_y = X.min(), X.max(), Y.min(), Y.max()
        lx = rng.uniform(lo_x - 0.2, hi_x + 0.2, 20000).astype(np.float32)
        ly = rng.uniform(lo_y - 0.2, hi_y + 0.2, 20000).astype(np.float32)
        sx, sy = patch_start(X, Y, lx, ly)
        ix, iy = np.arange(len(X))[None, :], np.arange(len(Y))[None, :]
        miss_x = ((np.abs(X[None, :] - lx[:, None]) < 0.16) & ((ix < sx[:, None]) | (ix > sx[:, None] + 7))).any(axis=1)
        miss_y = ((np.abs(Y[None, :] - ly[:, None]) < 0.16) & ((iy < sy[:, None]) | (iy > sy[:, None] + 7))).any(axis=1)
        missed = int((miss_x | miss_y).sum())
        if name in ("33x21-cubic", "33x21-reversed"):
            assert missed > 1000, (name, missed)
        else:
            assert missed == 0, (name, missed)
