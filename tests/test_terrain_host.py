"""The terrain specification (tests/terrain_oracle.py) on the host: against what the reference decides (tests/golden/terrain.npz, made
by tests/golden/make_terrain_golden.py: family and parameters per sub-terrain, origins, gap and pit cell for cell), its own
properties at 80-cell sub-terrains, seeds, and the validation of the configs.  No GPU."""
import dataclasses
import math

import numpy as np
import pytest

import terrain_oracle as O

S = 80                                                     # cells per side at terrain_length 4


def _one_hot(f):
    return [float(q == f) for q in range(9)]


def _single(fam, seed=5, difficulty_row=2, rows=3, **kw):
    """A rows x 1 curriculum grid of family `fam` (difficulty i / rows); returns (config, the sub-terrain of row `difficulty_row`)."""
    k = O.config(terrain_length=4., terrain_width=4., border_size=1., num_rows=rows, num_cols=1, terrain_proportions=_one_hot(fam),
                 seed=seed, **kw)
    r = O.generate(k)
    b = r["border"]
    assert (r["family"] == fam).all()
    return k, r, r["table"][b + difficulty_row * S:b + (difficulty_row + 1) * S, b:b + S].astype(np.int64)


# ------------------------------------------------------------------------------------------------ against the reference's decisions
@pytest.mark.parametrize("grid", ["grid3x9", "lite3"])
def test_layout_family_parameters_and_origins_are_the_references(golden, grid):
    g = golden("terrain")
    hs, vs, border_size, length = g[grid + "_cfg"].tolist()
    rows, cols, border, R, C = g[grid + "_shape"].tolist()
    k = O.config(horizontal_scale=hs, vertical_scale=vs, border_size=border_size, terrain_length=length, terrain_width=length,
                 num_rows=R, num_cols=C, terrain_proportions=g[grid + "_proportions"].tolist(), seed=1)
    r = O.generate(k)
    assert (r["tot_rows"], r["tot_cols"], r["border"]) == (rows, cols, border) and r["table"].shape == (rows, cols)
    assert np.array_equal(r["family"], g[grid + "_family"])
    assert np.array_equal(r["params"], g[grid + "_params"], equal_nan=True)                # every argument, to the bit
    ref = g[grid + "_env_origins"]
    assert np.array_equal(r["origins"][..., :2], ref[..., :2].astype(np.float32))
    own = np.isin(r["family"], (6, 7))                                                     # z: where the cells are the reference's
    assert np.array_equal(r["origins"][..., 2][own], ref[..., 2][own].astype(np.float32))
    if grid == "grid3x9":
        assert sorted(set(r["family"].ravel().tolist())) == list(range(9)) and own.sum() == 6
    else:
        assert np.array_equal(r["family"], np.tile([2, 4], (6, 1)))                        # Lite3's two columns: stairs down, discrete


def test_gap_and_pit_cell_for_cell(golden):
    g = golden("terrain")
    k = O.config(terrain_length=4., terrain_width=4.)
    for n, d in enumerate(g["difficulties"].tolist()):
        for fam, name in ((6, "gap"), (7, "pit")):
            f, par = O.make_terrain(0.5, d, O.cumulative(_one_hot(fam)))
            assert f == fam
            assert np.array_equal(O.sub_terrain(k, fam, par, 0), g[name][n]), (name, d)
    assert (g["gap"][1] == O.GAP_UNITS).any() and (g["pit"][2] < 0).any()


def test_gap_slice_wraps_as_python_does():
    """At high difficulty the reference's outer slice starts below zero and names only the last rows: kept, cell for cell."""
    k = O.config(terrain_length=4., terrain_width=4.)
    f, par = O.make_terrain(0.5, 0.9, O.cumulative(_one_hot(6)))
    want = np.zeros((S, S), dtype=np.int16)
    gap, P = int(par[0] / 0.05), int(1. / 0.05)
    x1 = (S - P) // 2
    x2 = x1 + gap
    assert S // 2 - x2 < 0
    want[S // 2 - x2:S // 2 + x2, S // 2 - x2:S // 2 + x2] = -1000
    want[S // 2 - x1:S // 2 + x1, S // 2 - x1:S // 2 + x1] = 0
    assert np.array_equal(O.sub_terrain(k, 6, par, 0), want)


# ------------------------------------------------------------------------------------------------ properties of the definitions
@pytest.mark.parametrize("fam", range(9))
def test_border_is_zero_and_values_fit(fam):
    k, r, z = _single(fam)
    b = r["border"]
    t = r["table"]
    assert b == 20 and t.shape == (3 * S + 2 * b, S + 2 * b)
    assert not t[:b].any() and not t[-b:].any() and not t[:, :b].any() and not t[:, -b:].any()
    assert z.any()


@pytest.mark.parametrize("fam,size", [(4, 3.), (5, 1.), (8, 1.3)])
def test_platform_cells_are_zero(fam, size):
    _, r, z = _single(fam)
    P = int(size / 0.05)
    x1, x2 = (S - P) // 2, (S + P) // 2
    assert not z[x1:x2, x1:x2].any()
    assert fam == 8 or r["origins"][2, 0, 2] == 0                                          # 8: its stones stand above the platform


@pytest.mark.parametrize("fam", [0, 1, 2, 3])
def test_pyramids_have_a_flat_three_metre_top(fam):
    _, r, z = _single(fam)
    top = z[10:70, 10:70]
    if fam == 1:
        assert np.abs(top - np.median(top)).max() <= 10                                    # the noise: at most 0.05 m
    else:
        assert (top == top[0, 0]).all() and top[0, 0] != 0
        assert r["origins"][2, 0, 2] == np.float32(int(top[0, 0]) * 0.005)


@pytest.mark.parametrize("fam", [5, 8])
def test_hole_depth(fam):
    _, _, z = _single(fam)
    assert z.min() == int(-2 / 0.005) == -400 and (z == -400).any()
    max_height = O.make_terrain(0.5, 2 / 3, O.cumulative(_one_hot(8)))[1][2]
    assert z.max() == (0 if fam == 5 else 2 * int(max_height / 0.005))                     # the reference's height_range ends there


def test_stepping_stone_share_is_the_lattices():
    """Above the platform, over whole periods in both directions, the stones of family 5 cover exactly (s / p)^2: every stone row has
    s of its p columns on stones, and a row shift only rotates which s of every p rows are."""
    for row in (1, 2):
        k, _, z = _single(5, difficulty_row=row)
        par = O.make_terrain(0.001, row / 3, O.cumulative(_one_hot(5)))[1]
        s, d = int(par[0] / 0.05), int(par[1] / 0.05)
        p = s + d
        assert d == 1 and 1 <= s < S
        x1 = (S - int(1. / 0.05)) // 2
        nb = x1 // p                                                                      # stone rows that end above the platform
        na = S // p
        band = z[:na * p, :nb * p]
        assert nb >= 1 and int((band == 0).sum()) * p * p == band.size * s * s


def test_stones_everywhere_share_within_the_size_draws_spread():
    """Family 8 over whole stones above the platform: a stone covers sa * sb of its p^2 cells, sa and sb each m - 1 or m with equal
    chance, so the share of n stones has mean (m - 1/2)^2 / p^2 and variance (E[sa^2]^2 - (m - 1/2)^4) / (n p^4); 4 sigma."""
    for row in (0, 1, 2):
        info = {}
        k = O.config(terrain_length=4., terrain_width=4., border_size=1., num_rows=3, num_cols=1, terrain_proportions=_one_hot(8), seed=21)
        par = O.make_terrain(0.5, row / 3, O.cumulative(_one_hot(8)))[1]
        z = O.sub_terrain(k, 8, par, row, info)
        m, p, shift = info["size"], info["period"], info["shift"]
        x1 = (S - int(1.3 / 0.05)) // 2
        stone, n = 0, 0
        for rb in range(x1 // p):
            a0 = (p - int(shift[rb])) % p                                                 # the first whole stone of this row
            na = (S - a0) // p
            stone += int((z[a0:a0 + na * p, rb * p:(rb + 1) * p] > 0).sum())
            n += na
        mean = (m - 0.5) ** 2
        var = (((m - 1) ** 2 + m ** 2) / 2) ** 2 - mean ** 2
        assert n > 50 and abs(stone / n - mean) <= 4 * math.sqrt(var / n), (row, stone / n, mean)


@pytest.mark.parametrize("fam", [2, 3])
def test_stairs_are_monotone_in_the_edge_distance(fam):
    _, _, z = _single(fam)
    a, b = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    e = np.minimum(np.minimum(a, S - 1 - a), np.minimum(b, S - 1 - b))
    level = np.array([z[e == d][0] for d in range(S // 2)])
    assert all((z[e == d] == level[d]).all() for d in range(S // 2))                       # a function of e alone
    steps = np.diff(level) * (1 if fam == 3 else -1)
    assert (steps >= 0).all() and steps.max() == int((0.05 + 0.13 * (2 / 3)) / 0.005) and (steps > 0).sum() == 10 // 6


def test_slope_sign_flips_in_the_lower_half_of_its_band():
    k = O.config(terrain_length=4., terrain_width=4., border_size=1., num_rows=3, num_cols=4, terrain_proportions=_one_hot(0), seed=1)
    r = O.generate(k)
    assert (r["family"] == 0).all()
    assert (r["params"][1:, :2, 0] < 0).all() and (r["params"][1:, 2:, 0] > 0).all()       # choice < 0.5: columns 0 and 1
    b = r["border"]
    down, up = r["table"][b + 2 * S:b + 3 * S, b:b + S], r["table"][b + 2 * S:b + 3 * S, b + 2 * S:b + 3 * S]
    assert np.array_equal(down, -up) and up.max() > 0 and r["origins"][2, 0, 2] == -r["origins"][2, 2, 2] < 0


# ------------------------------------------------------------------------------------------------ seeds
def test_seeds():
    base = dict(terrain_length=4., terrain_width=4., border_size=1., num_rows=3, num_cols=9, terrain_proportions=[1 / 9] * 9)
    a, a2, c = O.generate(O.config(seed=1, **base)), O.generate(O.config(seed=1, **base)), O.generate(O.config(seed=2, **base))
    assert np.array_equal(a["table"], a2["table"]) and np.array_equal(a["origins"], a2["origins"])
    b = a["border"]
    col = lambda r, j: r["table"][b:-b, b + j * S:b + (j + 1) * S]                        # noqa: E731
    for j in (0, 2, 3, 6, 7):                                                              # no draw: slope, stairs, gap, pit
        assert np.array_equal(col(a, j), col(c, j)), j
    for j in (1, 4, 5, 8):                                                                 # drawn: noise, rectangles, stones
        assert not np.array_equal(col(a, j), col(c, j)), j
    r1 = O.generate(O.config(seed=1, curriculum=False, **base))
    r2 = O.generate(O.config(seed=2, curriculum=False, **base))
    assert not np.array_equal(r1["family"], r2["family"])
    k = O.config(seed=1, curriculum=False, **base)
    drawn = [O.choice_and_difficulty(k, i, j) for i in range(3) for j in range(9)]
    assert all(0 <= c < 1 and d in O.RANDOM_DIFFICULTIES for c, d in drawn) and len({d for _, d in drawn}) == 4


# ------------------------------------------------------------------------------------------------ configs
def test_config_validation():
    from dtc_amd import sim as SIM
    from dtc_amd.env import SurrogateConfig, SurrogateLeggedEnv
    from dtc_amd.terrain import Terrain, TerrainConfig
    import torch
    assert SurrogateConfig().terrain is None
    t = TerrainConfig()
    assert (t.num_rows, t.num_cols, t.terrain_length, t.border_size, tuple(t.terrain_proportions)) == (6, 2, 8.0, 20.0, O.LITE3_PROPORTIONS)
    assert (t.tot_rows, t.tot_cols, t.border, t.cells_per_side) == (1760, 1120, 400, 160)
    assert t.cumulative_proportions() == O.cumulative(O.LITE3_PROPORTIONS)
    with pytest.raises(ValueError, match="terrain_width"):
        Terrain(dataclasses.replace(t, terrain_width=4.0), "cpu")
    with pytest.raises(NotImplementedError):
        Terrain(dataclasses.replace(t, selected=True), "cpu")
    with pytest.raises(ValueError, match="sum to 1"):
        Terrain(dataclasses.replace(t, terrain_proportions=(0.1, 0.1, 0.1, 0.1)), "cpu")
    with pytest.raises(ValueError, match="horizontal_scale"):
        SurrogateLeggedEnv(4, "cpu", SurrogateConfig(terrain=dataclasses.replace(t, horizontal_scale=0.1)))
    with pytest.raises(ValueError, match="border_size"):
        SurrogateLeggedEnv(4, "cpu", SurrogateConfig(sim=SIM.SimConfig(border_size=5.0), terrain=t))
    with pytest.raises(ValueError, match="height_samples"):
        SurrogateLeggedEnv(4, "cpu", SurrogateConfig(terrain=t), torch.zeros(8, 8, dtype=torch.int16))
    with pytest.raises(ValueError, match="max_init_terrain_level"):
        SurrogateLeggedEnv(4, "cpu", SurrogateConfig(terrain=dataclasses.replace(t, max_init_terrain_level=6)))
    rc = SurrogateConfig(terrain=t).reset_config()
    assert rc.terrain_curriculum and rc.custom_origins and rc.max_terrain_level == 6 and rc.env_length == 8.0
    rc = SurrogateConfig().reset_config()
    assert not rc.terrain_curriculum and not rc.custom_origins


def test_from_cfg_reads_the_reference_style_config():
    from dtc_amd.terrain import TerrainConfig

    class cfg:
        class terrain:
            mesh_type, horizontal_scale, vertical_scale, border_size, curriculum, selected = "trimesh", 0.05, 0.005, 20, True, False
            max_init_terrain_level, terrain_length, terrain_width, num_rows, num_cols = 5, 8., 8., 6, 2
            terrain_proportions = [0., 0., .2, .2, .2, .4]
    assert TerrainConfig.from_cfg(cfg, seed=3) == dataclasses.replace(TerrainConfig(), seed=3)
