"""Generate tests/golden/terrain.npz by RUNNING THE REFERENCE's Terrain (legged_gym/utils/terrain.py) with a stand-in
isaacgym.terrain_utils: `SubTerrain` is a plain holder and the five family functions record their name and arguments and do nothing
else, so the fixture pins what the reference decides -- layout, family and parameters per sub-terrain, origins -- and the three
sub-terrains it builds itself (gap, pit cell for cell; stones everywhere only as a hole share, for the documents).

    python tests/golden/make_terrain_golden.py

Runs only where the reference exists (the build container).  Arrays, names and numbers only.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _ref_harness as H  # noqa: E402
import terrain_oracle as O  # noqa: E402

H.install()
TU = sys.modules["isaacgym.terrain_utils"]
CALLS = []                                                 # (name, positional and keyword arguments) since the last clear


class SubTerrain:
    def __init__(self, terrain_name="terrain", width=256, length=256, vertical_scale=1.0, horizontal_scale=1.0):
        self.terrain_name, self.width, self.length = terrain_name, width, length
        self.vertical_scale, self.horizontal_scale = vertical_scale, horizontal_scale
        self.height_field_raw = np.zeros((width, length), dtype=np.int16)


def _recorder(name):
    def record(terrain, *args, **kwargs):
        CALLS.append((name, [float(a) for a in args] + [float(v) for v in kwargs.values()]))
        return terrain
    return record


TU.SubTerrain = SubTerrain
for _name in ("pyramid_sloped_terrain", "random_uniform_terrain", "pyramid_stairs_terrain", "discrete_obstacles_terrain",
              "stepping_stones_terrain"):
    setattr(TU, _name, _recorder(_name))

# terrain.py alone, by path: its only project import is the config class its annotation names
import importlib.util  # noqa: E402
import types  # noqa: E402

for _name in ("legged_gym", "legged_gym.envs", "legged_gym.envs.base", "legged_gym.envs.base.legged_robot_config"):
    sys.modules.setdefault(_name, types.ModuleType(_name))
sys.modules["legged_gym.envs.base.legged_robot_config"].LeggedRobotCfg = type("LeggedRobotCfg", (), {"terrain": object})
_spec = importlib.util.spec_from_file_location("reference_terrain", os.path.join(H.REF_ROOT, "legged_gym", "utils", "terrain.py"))
T = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(T)

for _name in ("gap_terrain", "pit_terrain", "stones_everywhere_terrain"):           # the reference's own: run them, and record the call

    def _wrap(fn, name):
        def run(terrain, *args, **kwargs):
            CALLS.append((name, [float(a) for a in args] + [float(v) for v in kwargs.values()]))
            return fn(terrain, *args, **kwargs)
        return run
    setattr(T, _name, _wrap(getattr(T, _name), _name))


def _family(calls):
    """The recorded calls of one make_terrain as (family index of tests/terrain_oracle.py, arguments NaN-padded to six)."""
    names = [c[0] for c in calls]
    args = [v for c in calls for v in c[1]]
    if names == ["pyramid_sloped_terrain"]:
        fam = 0
    elif names == ["pyramid_sloped_terrain", "random_uniform_terrain"]:
        fam = 1
    elif names == ["pyramid_stairs_terrain"]:
        fam = 2 if args[1] < 0 else 3
    else:
        fam = {"discrete_obstacles_terrain": 4, "stepping_stones_terrain": 5, "gap_terrain": 6, "pit_terrain": 7,
               "stones_everywhere_terrain": 8}[names[0]]
        assert len(names) == 1
    return fam, np.array(args + [np.nan] * (6 - len(args)))


def _terrain_cfg(**kw):
    class cfg:
        mesh_type, horizontal_scale, vertical_scale, border_size, curriculum, selected = "heightfield", 0.05, 0.005, 20, True, False
        terrain_length, terrain_width, num_rows, num_cols, slope_treshold = 8., 8., 6, 2, 0.75
        terrain_proportions = list(O.LITE3_PROPORTIONS)
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def layout(prefix, out, **kw):
    """curiculum() of the reference, make_terrain by make_terrain."""
    cfg = _terrain_cfg(**kw)
    R, C = cfg.num_rows, cfg.num_cols
    family, params = np.zeros((R, C), dtype=np.int64), np.zeros((R, C, 6))
    made = {}
    real = T.Terrain.make_terrain

    def make_terrain(self, choice, difficulty):
        del CALLS[:]
        t = real(self, choice, difficulty)
        made[id(t)] = _family(CALLS)
        return t

    real_add = T.Terrain.add_terrain_to_map

    def add_terrain_to_map(self, terrain, row, col):
        family[row, col], params[row, col] = made[id(terrain)]
        return real_add(self, terrain, row, col)

    T.Terrain.make_terrain, T.Terrain.add_terrain_to_map = make_terrain, add_terrain_to_map
    try:
        t = T.Terrain(cfg, 16)
    finally:
        T.Terrain.make_terrain, T.Terrain.add_terrain_to_map = real, real_add
    out[prefix + "_family"], out[prefix + "_params"], out[prefix + "_env_origins"] = family, params, t.env_origins
    out[prefix + "_shape"] = np.array([t.tot_rows, t.tot_cols, t.border, R, C])
    out[prefix + "_cfg"] = np.array([cfg.horizontal_scale, cfg.vertical_scale, cfg.border_size, cfg.terrain_length])
    out[prefix + "_proportions"] = np.array(cfg.terrain_proportions, dtype=np.float64)
    # only the gap and pit cells of the table are the reference's (the stand-in families leave zeros)
    return t


def main():
    out = {"family_names": np.array(O.FAMILIES)}
    layout("grid3x9", out, terrain_length=4., terrain_width=4., border_size=1, num_rows=3, num_cols=9, terrain_proportions=[1 / 9] * 9)
    layout("lite3", out)
    difficulties = np.array([0.0, 1 / 3, 2 / 3])
    out["difficulties"] = difficulties
    S = int(4. / 0.05)
    gaps, pits, share = [], [], np.zeros((3, 16))
    for n, d in enumerate(difficulties):
        one_hot = lambda f: O.cumulative([float(q == f) for q in range(9)])       # noqa: E731
        gap_size, pit_depth, stones = (O.make_terrain(0.5, float(d), one_hot(f))[1] for f in (6, 7, 8))
        t = SubTerrain(width=S, length=S, vertical_scale=0.005, horizontal_scale=0.05)
        T.gap_terrain(t, gap_size=gap_size[0], platform_size=1.)
        gaps.append(t.height_field_raw.copy())
        t = SubTerrain(width=S, length=S, vertical_scale=0.005, horizontal_scale=0.05)
        T.pit_terrain(t, depth=pit_depth[0], platform_size=1.)
        pits.append(t.height_field_raw.copy())
        for seed in range(16):                                                       # the hole share of the reference's stones everywhere
            np.random.seed(seed)
            t = SubTerrain(width=S, length=S, vertical_scale=0.005, horizontal_scale=0.05)
            T.stones_everywhere_terrain(t, stone_size=stones[0], stone_distance=stones[1], max_height=stones[2], platform_size=stones[3],
                                        depth=stones[4])
            share[n, seed] = float((t.height_field_raw == int(-2 / 0.005)).mean())
    out["gap"], out["pit"], out["stones_everywhere_hole_share"] = np.stack(gaps), np.stack(pits), share
    path = os.path.join(HERE, "terrain.npz")
    np.savez_compressed(path, **out)
    # this project's stones everywhere (tests/terrain_oracle.py) under the same 16 seeds, for the documents: not part of the fixture
    own = np.zeros((3, 16))
    for n, d in enumerate(difficulties):
        par = O.make_terrain(0.5, float(d), O.cumulative([float(q == 8) for q in range(9)]))[1]
        for seed in range(16):
            z = O.sub_terrain(O.config(terrain_length=4., terrain_width=4., seed=seed), 8, par, 0)
            own[n, seed] = float((z == int(-2 / 0.005)).mean())
    print(f"wrote {path}: {os.path.getsize(path)} bytes; stones-everywhere hole share per difficulty: the reference's "
          f"{share.mean(axis=1).round(4).tolist()}, this project's {own.mean(axis=1).round(4).tolist()}")


if __name__ == "__main__":
    main()
