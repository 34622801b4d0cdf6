"""The generic foothold kernel (`foothold_plan_kernel`: every grid other than 33 x 21, and the debug outputs) against the
any-grid oracle, bit for bit, at the grids where its paths change.  GPU only.

    grid               what it exercises
    17x11@0.05         P = 187, P % 4 = 3 (zero tail of the canonical two-sum order); candidate patch
    17x11@0.1          stock legged_gym grid: search radius 1.65 cells, gradient divisors still 0.05 / 0.1
    9x8@0.05           ny == 8: the patch at its boundary; P = 72
    9x7@0.05           ny < 8: always the full scan; P = 63 < 64 lanes
    13x9@0.047         2 * rad = 6.91 cells: the patch near its limit
    13x9@0.046         2 * rad = 7.06 cells: patch_ok = 0, full scan
    2x2                the smallest grid accepted; variance over P - 1 = 3
    8x16@0.05          ny > nx: the decode's wrap of the x table (the reference gathers from tables repeated four times)
    63x32@0.025        P = 2016, 64 896 B of dynamic LDS: the largest request below 64 KiB
    64x32@0.025        the size limit: 65 920 B of dynamic LDS (the device grants 160 KiB per workgroup)
    33x21+generic      the generic kernel's patch path (DTC_PLANNER_GENERIC=1) on the stress kinds
    33x21-cubic        non-uniform tables: the uniform patch placement would miss in-radius points -> full scan
    33x21-reversed     decreasing tables: likewise

Each grid runs N in {1, 3, 5, 257} (a partial workgroup of 4 envs, a full one plus a tail, many) x the five input kinds of
cases.planner_inputs, with and without debug outputs, on a 16-byte aligned and a misaligned heights view (float4 / scalar
loads).  Inputs and oracle results are computed once per grid and shared.

Measured on an MI355X before `patch_ok` asked for uniform tables: on the cubic tables the call without debug outputs
differed from the oracle on 177 of 5320 (env, leg) pairs through the fast kernel and on 158 through the generic kernel
(the debug call's full scan on none); on the reversed tables and on the uniform 33 x 21 grid on none.  With the rule every
output of every case equals the oracle bit for bit."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import cases as C  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OUT = ("optimal_foothold_indice", "foothold_obs", "optimal_footholds_world", "pred_footholds", "pred_footholds_to_robot")
PATCH_GRIDS = ("17x11@0.05", "17x11@0.1", "9x8@0.05", "13x9@0.047", "8x16@0.05", "33x21")       # patch_ok and ny >= 8
VARIANTS = tuple(n if n != "33x21" else "33x21+generic" for n in C.PLANNER_GRIDS) + ("33x21-cubic+generic", "33x21-reversed+generic")


def _np(t):
    return t.detach().cpu().numpy()


def _grid(X, Y):
    from dtc_amd import foothold
    return foothold.GridConfig(tuple(float(v) for v in X), tuple(float(v) for v in Y))


@functools.lru_cache(maxsize=None)
def oracle_cases(name):
    """[(N, kind, inputs, oracle outputs incl. the debug ones)] of one grid; never modified by a test."""
    from oracle import foothold as OF
    X, Y = C.planner_grid(name)
    out = []
    for N, kind, seed in C.planner_cases(name):
        inp = C.planner_inputs(N, X, Y, seed, kind)
        o = OF.plan(_np(inp["measured_heights"]), _np(inp["root_states"]), _np(inp["thigh_pos"]), _np(inp["commands"]), X, Y,
                    want_debug=True)
        out.append((N, kind, inp, o))
    return X, Y, out


def _assert_equal(o, h, debug, what):
    np.testing.assert_array_equal(_np(h["optimal_foothold_indice"]).squeeze(1), o["idx"], err_msg=str(what))
    np.testing.assert_array_equal(_np(h["foothold_obs"]), o["foothold_obs"], err_msg=str(what))
    np.testing.assert_array_equal(_np(h["optimal_footholds_world"]), o["optimal_footholds_world"], err_msg=str(what))
    np.testing.assert_array_equal(_np(h["pred_footholds"]), o["pred_footholds"], err_msg=str(what))
    np.testing.assert_array_equal(_np(h["pred_footholds_to_robot"]), o["pred_footholds_to_robot"], err_msg=str(what))
    if debug:
        np.testing.assert_array_equal(_np(h["foothold_score"]), o["foothold_score"], err_msg=str(what))
        np.testing.assert_array_equal(_np(h["nominal_footholds_indice"]), o["nominal_idx"], err_msg=str(what))
        np.testing.assert_array_equal(_np(h["slope"]), o["slope"], err_msg=str(what))
        np.testing.assert_array_equal(_np(h["heights_world"])[:, :, :2], o["heights_world_xy"], err_msg=str(what))
        np.testing.assert_array_equal(_np(h["heights_world"])[:, :, 2], _np(h["_mh"]), err_msg=str(what))


def winner_totals(o):
    """Oracle total of the oracle's winner, [N, 4]."""
    return np.take_along_axis(o["foothold_score"], o["idx"][:, None, :], axis=1)[:, 0, :]


def nominal_in_grid_frame(inp, o):
    """R(-yaw) * (pred - base): the nominal footholds in the frame of the coordinate tables (float64; coverage only)."""
    rs = _np(inp["root_states"]).astype(np.float64)
    n = np.maximum(np.sqrt(rs[:, 5] ** 2 + rs[:, 6] ** 2), 1e-9)
    zq, wq = (rs[:, 5] / n)[:, None], (rs[:, 6] / n)[:, None]
    cy, sy = wq * wq - zq * zq, 2.0 * wq * zq
    rx, ry = o["pred_footholds"][:, :, 0] - rs[:, 0:1], o["pred_footholds"][:, :, 1] - rs[:, 1:2]
    return cy * rx + sy * ry, -sy * rx + cy * ry


def outside_uniform_patch(X, Y, inp, o):
    """[N, 4] bool: the oracle's winner is valid, lies outside the 8 x 8 patch the uniform-table formulas of make_params
    place, AND that patch holds a valid candidate of its own -- the kernel would accept the patch minimum and lose the winner."""
    from test_planner_grid_oracle import patch_start
    lx, ly = nominal_in_grid_frame(inp, o)
    sx, sy = patch_start(X, Y, lx, ly)
    ny = len(Y)
    wix, wiy = o["idx"] // ny, o["idx"] % ny
    out = (wix < sx) | (wix > sx + 7) | (wiy < sy) | (wiy > sy + 7)
    tot = o["foothold_score"].reshape(len(lx), len(X), ny, 4)
    ix, iy = np.arange(len(X))[None, :, None, None], np.arange(ny)[None, None, :, None]
    inside = (ix >= sx[:, None, None, :]) & (ix <= sx[:, None, None, :] + 7) & (iy >= sy[:, None, None, :]) & (iy <= sy[:, None, None, :] + 7)
    patch_min = np.where(inside, tot, np.inf).min(axis=(1, 2))
    return out & (winner_totals(o) < 1.0) & (patch_min < 1.0)


def _plan(inp, grid, debug, misaligned):
    from dtc_amd import foothold
    N, P = inp["measured_heights"].shape
    if misaligned:
        buf = torch.empty(N * P + 1, device=DEV)
        mh = buf[1:].view(N, P)
        mh.copy_(inp["measured_heights"])
        assert mh.data_ptr() % 16 != 0
    else:
        mh = inp["measured_heights"].to(DEV)
        assert mh.data_ptr() % 16 == 0
    h = foothold.plan(mh, inp["root_states"].to(DEV), inp["thigh_pos"].to(DEV), inp["commands"].to(DEV), grid=grid, want_debug=debug)
    h["_mh"] = mh
    return h


@pytest.mark.parametrize("variant", VARIANTS)
def test_generic_planner_bit_exact_vs_oracle(variant, monkeypatch):
    name, _, generic = variant.partition("+")
    if generic:
        monkeypatch.setenv("DTC_PLANNER_GENERIC", "1")
    X, Y, cases = oracle_cases(name)
    grid = _grid(X, Y)
    for N, kind, inp, o in cases:
        dbg = None
        for misaligned in (False, True):
            for debug in (True, False):
                h = _plan(inp, grid, debug, misaligned)
                _assert_equal(o, h, debug, (variant, N, kind, "debug" if debug else "plain", "misaligned" if misaligned else "aligned"))
                if debug:
                    dbg = h
                else:                       # the call without debug outputs equals the debug call's full scan
                    for k in OUT:
                        assert torch.equal(h[k], dbg[k]), (variant, N, kind, k)


@pytest.mark.parametrize("name", PATCH_GRIDS)
def test_patch_and_fallback_are_both_reached(name):
    """Branch coverage proved from the oracle's own totals: some (env, leg) has a valid winner (total < 1: the patch result
    is accepted) and some env of the `rough` / `border` kinds has a leg without one (the wave falls back to the full scan)."""
    from dtc_amd import foothold
    X, Y, cases = oracle_cases(name)
    i = foothold.grid_info(_grid(X, Y))
    assert i["patch_ok"] and len(Y) >= 8
    valid = sum(int((winner_totals(o) < 1.0).sum()) for _, _, _, o in cases)
    fallback = sum(int((winner_totals(o) >= 1.0).any(axis=1).sum()) for _, kind, _, o in cases if kind in ("rough", "border"))
    assert valid > 0 and fallback > 0, (valid, fallback)


def test_nonuniform_cases_can_expose_a_uniform_placement():
    """The inputs of the non-uniform grid hold (env, leg) pairs whose oracle winner lies outside the patch that uniform
    placement would choose while that patch holds a valid candidate (177 of 5320): a kernel that placed the patch there
    returns another index, so the bit-exact test above sees it.  (On the reversed tables the misplaced patch starts 3.15
    cells beyond the nominal foothold and so holds no in-radius point but for a sliver 0.05 cells wide: the kernel falls
    back to the full scan; these inputs hold no such pair, and none on the uniform grid.)"""
    from dtc_amd import foothold
    X, Y, cases = oracle_cases("33x21-cubic")
    assert not foothold.grid_info(_grid(X, Y))["patch_ok"]
    assert sum(int(outside_uniform_patch(X, Y, inp, o).sum()) for _, _, inp, o in cases) > 0
    Xu, Yu, cu = oracle_cases("33x21")
    assert sum(int(outside_uniform_patch(Xu, Yu, inp, o).sum()) for _, _, inp, o in cu) == 0


def test_lds_limit_covers_the_largest_grid():
    """64 x 32 asks for 65 920 B of dynamic LDS per workgroup; the device's limit (163 840 B on the MI355X) covers it, and
    dtc_foothold_plan compares the two before it launches."""
    from dtc_amd import foothold
    need = foothold.grid_info(_grid(*C.planner_grid("64x32@0.025")))["lds_bytes"]
    assert need == 65920 <= torch.cuda.get_device_properties(0).shared_memory_per_block


@pytest.mark.parametrize("tag", [t for t, _, _ in C.SCORER_GRID_CASES])
def test_planner_matches_reference_on_other_grids(golden, tag):
    """The kernel against the fixture recorded from the reference on 17 x 11 at 0.1 m and 8 x 16 at 0.05 m.  Knife-edge
    policy: an index may differ only where the recorded runner-up gap is <= 1e-5, on at most 4 (env, leg) pairs, and the
    kernel's choice must then be a near-minimum of the oracle's own score table."""
    from oracle import foothold as OF
    g = golden("scorer_grids")
    X, Y, inp = C.scorer_grid_inputs(tag)
    h = _plan(inp, _grid(X, Y), False, False)
    idx = _np(h["optimal_foothold_indice"]).squeeze(1)
    ref = g[tag + "_idx"].astype(np.int64)
    mism = np.argwhere(idx != ref)
    assert len(mism) <= 4
    if len(mism):
        rows = np.unique(mism[:, 0])
        o = OF.plan(*(_np(inp[k])[rows] for k in ("measured_heights", "root_states", "thigh_pos", "commands")), X, Y, want_debug=True)
        for e, l in mism:
            r = int(np.searchsorted(rows, e))
            assert g[tag + "_gap"][e, l] <= 1e-5, (e, l)
            assert o["foothold_score"][r, ref[e, l], l] - o["foothold_score"][r, idx[e, l], l] <= 1e-5, (e, l)
    ok = np.ones(len(ref), bool)
    ok[mism[:, 0]] = False
    sub = ok[::4]
    np.testing.assert_array_equal(_np(h["foothold_obs"])[::4][sub], g[tag + "_foothold_obs"][sub])
    np.testing.assert_allclose(_np(h["optimal_footholds_world"])[::4][sub], g[tag + "_world"][sub], rtol=0, atol=4e-6)
    np.testing.assert_allclose(_np(h["pred_footholds"])[::4], g[tag + "_pred"], rtol=0, atol=4e-6)
    np.testing.assert_allclose(_np(h["pred_footholds_to_robot"])[::4], g[tag + "_pred_to_robot"], rtol=0, atol=4e-6)


@pytest.mark.parametrize("name", ["17x11@0.1", "8x16@0.05"])
def test_get_heights_other_grids_bit_exact(name):
    """`get_heights` on two other grids, including root positions on and past the terrain table's border."""
    from dtc_amd import foothold
    from oracle import heights as OH
    from test_hip_kernels import _terrain_table
    X, Y = C.planner_grid(name)
    tab = _terrain_table()
    root = C.planner_inputs(261, X, Y, 77, "random")["root_states"]
    root[:8, 0] = torch.tensor([-30., -19.99, 0., 67.9, 68.0, 100., 20., 20.])
    root[:8, 1] = torch.tensor([-30., 0., -19.99, 35.9, 36.0, 100., -25., 40.])
    ref = OH.get_heights(tab.numpy(), root.numpy(), X, Y)
    got = foothold.get_heights(tab.to(DEV), root.to(DEV), grid=_grid(X, Y))
    np.testing.assert_array_equal(_np(got), ref)
