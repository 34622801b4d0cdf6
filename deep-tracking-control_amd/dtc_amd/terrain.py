"""Host side of the DTC curriculum terrain (csrc/terrain.hip, `dtc_terrain_generate`): the int16 height table and the sub-terrain
origins of legged_gym/utils/terrain.py, generated in device memory from one seed in one launch, with no host dependency (the
reference's generator needs isaacgym.terrain_utils, scipy and Python loops per stone).

The reference's: the layout, the choice of a family from `terrain_proportions`, the parameters of make_terrain (its "lite3" values),
the origins, and the gap and pit sub-terrains cell for cell.  This project's definitions, with the reference's parameters but neither
its numpy random sequence nor isaacgym's code: the cells of the slopes, stairs, discrete obstacles, stepping stones and stones
everywhere.  include/dtc_hip.h states every formula; tests/terrain_oracle.py restates them in numpy.

`TerrainConfig` holds the fields of LeggedRobotCfg.terrain that matter (defaults: the Lite3 DTC values) plus `seed`;
`Terrain(cfg, device)` carries the attribute names the reference's class has.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import _ffi

LITE3_PROPORTIONS = (0.0, 0.0, 0.2, 0.2, 0.2, 0.4)
FAMILIES = ("smooth_slope", "rough_slope", "stairs_down", "stairs_up", "discrete_obstacles", "stepping_stones", "gap", "pit",
            "stones_everywhere")


@dataclass
class TerrainConfig:
    """Names as in LeggedRobotCfg.terrain (lite3_dtc_config.py:20-51)."""
    horizontal_scale: float = 0.05
    vertical_scale: float = 0.005
    border_size: float = 20.0
    curriculum: bool = True
    selected: bool = False
    max_init_terrain_level: int = 5
    terrain_length: float = 8.0
    terrain_width: float = 8.0
    num_rows: int = 6
    num_cols: int = 2
    terrain_proportions: tuple = LITE3_PROPORTIONS
    seed: int = 0

    @classmethod
    def from_cfg(cls, env_cfg, *, seed: int = 0) -> "TerrainConfig":
        """From a LeggedRobotCfg-style config class or instance (its `terrain` member)."""
        t = env_cfg.terrain
        return cls(horizontal_scale=float(t.horizontal_scale), vertical_scale=float(t.vertical_scale), border_size=float(t.border_size),
                   curriculum=bool(t.curriculum), selected=bool(getattr(t, "selected", False)),
                   max_init_terrain_level=int(t.max_init_terrain_level), terrain_length=float(t.terrain_length),
                   terrain_width=float(t.terrain_width), num_rows=int(t.num_rows), num_cols=int(t.num_cols),
                   terrain_proportions=tuple(float(p) for p in t.terrain_proportions), seed=int(seed))

    def validate(self):
        if self.selected:
            raise NotImplementedError("TerrainConfig.selected: the reference eval()s a function name there; not supported")
        if self.terrain_length != self.terrain_width:
            raise ValueError(f"terrain_length {self.terrain_length} != terrain_width {self.terrain_width}: the reference builds square "
                             "sub-terrains from the width")
        if not (self.horizontal_scale > 0 and self.vertical_scale > 0 and self.border_size >= 0 and self.terrain_length >= 2.0):
            raise ValueError("TerrainConfig: positive scales, border_size >= 0 and sub-terrains of at least 2 m")
        if self.num_rows < 1 or self.num_cols < 1:
            raise ValueError("TerrainConfig: at least one row and one column")
        if not 4 <= len(self.terrain_proportions) <= 9:
            raise ValueError("TerrainConfig: terrain_proportions has 4 to 9 entries")
        if len(self.terrain_proportions) < 9 and self.cumulative_proportions()[len(self.terrain_proportions) - 1] < 1.0:
            raise ValueError("TerrainConfig: a terrain_proportions list shorter than nine entries must sum to 1 (the reference indexes "
                             "past its end otherwise)")

    def cumulative_proportions(self) -> list:
        """Terrain.__init__'s cumulative sums (terrain.py:18), padded to nine entries with 2.0: no choice reaches the padding."""
        p = [float(np.sum(list(self.terrain_proportions)[:i + 1])) for i in range(len(self.terrain_proportions))]
        return p + [2.0] * (9 - len(p))

    @property
    def cells_per_side(self) -> int:
        return int(self.terrain_length / self.horizontal_scale)

    @property
    def border(self) -> int:
        return int(self.border_size / self.horizontal_scale)

    @property
    def tot_rows(self) -> int:
        return self.num_rows * self.cells_per_side + 2 * self.border

    @property
    def tot_cols(self) -> int:
        return self.num_cols * self.cells_per_side + 2 * self.border


class Terrain:
    """The reference's Terrain on the device: `height_field_raw` / `heightsamples` (ONE int16 tensor [tot_rows, tot_cols]),
    `env_origins` [num_rows, num_cols, 3] fp32, `tot_rows`, `tot_cols`, `border`, `env_length`, `env_width`.  `generate(seed=None)`
    refills both tensors in place (one launch, nothing read back), so every holder of the table sees the new layout.  `out`, an int16
    tensor of the table's shape on the device, is used as the table instead of a fresh one."""

    def __init__(self, cfg: TerrainConfig | None = None, device="cuda", *, out: torch.Tensor | None = None):
        cfg = self.cfg = cfg or TerrainConfig()
        cfg.validate()
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device, self.seed = dev, int(cfg.seed)
        self.env_length, self.env_width = cfg.terrain_length, cfg.terrain_width
        self.border, self.tot_rows, self.tot_cols = cfg.border, cfg.tot_rows, cfg.tot_cols
        self.width_per_env_pixels = self.length_per_env_pixels = cfg.cells_per_side
        if self.tot_rows * self.tot_cols >= 1 << 31:
            raise ValueError(f"Terrain: a table of {self.tot_rows} x {self.tot_cols} cells has 2^31 cells or more")
        if out is None:
            out = torch.zeros(self.tot_rows, self.tot_cols, dtype=torch.int16, device=dev)
        elif out.dtype != torch.int16 or tuple(out.shape) != (self.tot_rows, self.tot_cols) or out.device != dev or not out.is_contiguous():
            raise ValueError(f"Terrain: out must be a contiguous int16 tensor of shape {(self.tot_rows, self.tot_cols)} on {dev}")
        self.height_field_raw = self.heightsamples = out
        self.env_origins = torch.zeros(cfg.num_rows, cfg.num_cols, 3, dtype=torch.float32, device=dev)
        self.generate()

    def cfg_struct(self) -> "_ffi.DtcTerrainCfg":
        k, c = self.cfg, _ffi.DtcTerrainCfg()
        c.horizontal_scale, c.vertical_scale, c.border_size = k.horizontal_scale, k.vertical_scale, k.border_size
        c.terrain_length, c.terrain_width = k.terrain_length, k.terrain_width
        for i, p in enumerate(k.cumulative_proportions()):
            c.proportions[i] = p
        c.num_rows, c.num_cols, c.curriculum = int(k.num_rows), int(k.num_cols), int(bool(k.curriculum))
        c.tot_rows, c.tot_cols, c.seed = self.tot_rows, self.tot_cols, self.seed & 0xFFFFFFFFFFFFFFFF
        return c

    def generate(self, seed: int | None = None) -> "Terrain":
        if seed is not None:
            self.seed = int(seed)
        _ffi.check(_ffi.lib().dtc_terrain_generate(self.cfg_struct(), _ffi.ptr(self.height_field_raw), _ffi.ptr(self.env_origins),
                                                   _ffi.stream()), "dtc_terrain_generate")
        return self
