"""TEST INFRASTRUCTURE and SPECIFICATION: numpy restatement of dtc_terrain_generate (csrc/terrain.hip; include/dtc_hip.h states the
formulas).  The layout (Terrain.__init__, curiculum, randomized_terrain, add_terrain_to_map), the family choice and the parameters
(make_terrain, the "lite3" values) and the gap and pit sub-terrains are the reference's (legged_gym/utils/terrain.py); the cells of the
other seven families are this project's definitions with the reference's parameters: pure functions of (config, seed, i, j, cell), with
Philox4x32-10 draws instead of numpy's sequential stream, and not isaacgym's code.

Arithmetic: parameters are IEEE doubles in the order written (Python floats here, `double` under -ffp-contract=off in the kernel), so
that every int(x / scale) is the reference's; cells are integers.  Nothing here imports the package's kernels; Philox4x32-10 is
oracle/rng.py's numpy restatement (put on the path below), the one tests/sim_oracle.py draws from."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
from rng import philox4x32_10  # noqa: E402

FAMILIES = ("smooth_slope", "rough_slope", "stairs_down", "stairs_up", "discrete_obstacles", "stepping_stones", "gap", "pit",
            "stones_everywhere")
LITE3_PROPORTIONS = (0.0, 0.0, 0.2, 0.2, 0.2, 0.4)
TAG = 0x74657272                                   # "terr": word 3 of every counter
# purposes (word 2 of the counter)
P_LAYOUT, P_NODE, P_RECT, P_STEP_SHIFT, P_STONE_SHIFT, P_STONE = 0, 1, 2, 3, 4, 5
GAP_UNITS = -1000                                  # the reference's literal, whatever the vertical scale
NUM_RECTANGLES = 20
RANDOM_DIFFICULTIES = (0.25, 0.5, 0.75, 0.9)


def config(*, horizontal_scale=0.05, vertical_scale=0.005, border_size=20.0, curriculum=True, terrain_length=8.0, terrain_width=8.0,
           num_rows=6, num_cols=2, terrain_proportions=LITE3_PROPORTIONS, seed=0) -> dict:
    return dict(locals())


def cumulative(proportions):
    """Terrain.__init__'s cumulative sums, padded to nine entries with 2.0 (no choice reaches them)."""
    p = [float(np.sum(list(proportions)[:i + 1])) for i in range(len(proportions))]
    return p + [2.0] * (9 - len(p))


def geometry(k: dict) -> dict:
    hs = k["horizontal_scale"]
    S = int(k["terrain_length"] / hs)
    border = int(k["border_size"] / hs)
    R, C = k["num_rows"], k["num_cols"]
    x1 = int((k["terrain_length"] / 2. - 1) / hs)
    x2 = min(int((k["terrain_length"] / 2. + 1) / hs), S)
    return dict(S=S, border=border, tot_rows=R * S + 2 * border, tot_cols=C * S + 2 * border, x1=x1, x2=x2)


def draws(seed, sub, purpose, items):
    """Philox4x32-10: key = (seed low, seed high), counter = (item, sub-terrain index i * C + j, purpose, TAG).  Returns the four
    32-bit words of every item as uint64 [len(items), 4]."""
    items = np.asarray(items, dtype=np.uint64).reshape(-1)
    ctr = np.zeros((items.size, 4), dtype=np.uint64)
    ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3] = items, sub, purpose, TAG
    return philox4x32_10(ctr, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)


def below(word, n):
    """A 32-bit word to an integer in [0, n): (word * n) >> 32."""
    return ((word.astype(np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def choice_and_difficulty(k: dict, i: int, j: int):
    R, C = k["num_rows"], k["num_cols"]
    if k["curriculum"]:
        return j / C + 0.001, i / R
    w = draws(k["seed"], i * C + j, P_LAYOUT, [0])[0]
    return float(w[0]) * 2.0 ** -32, RANDOM_DIFFICULTIES[int(w[1]) >> 30]


def make_terrain(choice: float, difficulty: float, cum) -> tuple:
    """(family index, the arguments the reference passes to that family's generator, NaN-padded to six)."""
    slope = difficulty * 0.4
    stepping_stones_size = 1 * (1.05 - difficulty)
    step_height = 0.05 + 0.13 * difficulty
    discrete_obstacles_height = 0.05 + difficulty * 0.15
    stone_distance = 0.03 if difficulty == 0 else 0.06
    max_height = 0.02 + 0.03 * difficulty
    stone_size = -0.1 * difficulty + 0.3
    gap_size = .8 * difficulty
    pit_depth = .8 * difficulty
    if choice < cum[0]:
        if choice < cum[0] / 2:
            slope *= -1
        fam, par = 0, (slope, 3.)
    elif choice < cum[1]:
        fam, par = 1, (slope, 3., -0.05, 0.05, 0.005, 0.2)
    elif choice < cum[3]:
        if choice < cum[2]:
            step_height *= -1
            fam = 2
        else:
            fam = 3
        par = (0.31, step_height, 3.)
    elif choice < cum[4]:
        fam, par = 4, (discrete_obstacles_height, 1., 2., float(NUM_RECTANGLES), 3.)
    elif choice < cum[5]:
        fam, par = 5, (stepping_stones_size, stone_distance, 0., 1., -2.)
    elif choice < cum[6]:
        fam, par = 6, (gap_size, 1.)
    elif choice < cum[7]:
        fam, par = 7, (pit_depth, 1.)
    else:
        fam, par = 8, (stone_size, stone_distance, max_height, 1.3, -2.)
    return fam, np.array(list(par) + [np.nan] * (6 - len(par)))


def _slice(start, stop, S):
    """The cells a Python slice [start:stop] of a length-S axis names (a negative start counts from the end, as the reference's
    gap_terrain meets at high difficulty)."""
    lo = max(start + S, 0) if start < 0 else min(start, S)
    hi = max(stop + S, 0) if stop < 0 else min(stop, S)
    return lo, hi


def sub_terrain(k: dict, fam: int, par, sub: int, info: dict | None = None) -> np.ndarray:
    """One sub-terrain [S, S] in int64 units of the vertical scale (before the int16 clamp)."""
    hs, vs, seed = k["horizontal_scale"], k["vertical_scale"], k["seed"]
    S = int(k["terrain_length"] / hs)
    a, b = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    z = np.zeros((S, S), dtype=np.int64)

    def platform(size):
        P = int(size / hs)
        return ((S - P) // 2, (S + P) // 2) if P < S else (0, S)                         # a platform wider than the sub-terrain is all of it

    def pyramid(platform_size):
        e = np.minimum(np.minimum(a, S - 1 - a), np.minimum(b, S - 1 - b))
        return np.minimum(e, max((S - int(platform_size / hs)) // 2, 0))

    if fam in (0, 1):
        z = np.rint(((par[0] * hs) * pyramid(par[1]).astype(np.float64)) / vs).astype(np.int64)
        if fam == 1:
            g = max(int(par[5] / hs), 1)
            W = S // g + 2
            k21 = below(draws(seed, sub, P_NODE, np.arange(W * W))[:, 0], 21).reshape(W, W)
            node = ((k21 - 10).astype(np.float64) * par[4]) / vs                         # a multiple of 0.005 m, in units
            na, nb, fa, fb = a // g, b // g, a % g, b % g
            t = ((((g - fa) * (g - fb)).astype(np.float64) * node[na, nb] + (fa * (g - fb)).astype(np.float64) * node[na + 1, nb]) +
                 (((g - fa) * fb).astype(np.float64) * node[na, nb + 1] + (fa * fb).astype(np.float64) * node[na + 1, nb + 1]))
            z = z + np.rint(t / float(g * g)).astype(np.int64)
    elif fam in (2, 3):
        w = max(int(par[0] / hs), 1)
        z = (pyramid(par[2]) // w) * int(par[1] / vs)
    elif fam == 4:
        full = int(par[0] / vs)
        m0, m1 = int(par[1] / hs), int(par[2] / hs)
        x = draws(seed, sub, P_RECT, np.arange(NUM_RECTANGLES))
        for r in range(NUM_RECTANGLES):                                                  # later rectangles overwrite earlier ones
            la = min(m0 + int(below(x[r, 0], m1 - m0 + 1)), S)
            lb = min(m0 + int(below(x[r, 1], m1 - m0 + 1)), S)
            pa, pb = int(below(x[r, 2], S - la + 1)), int(below(x[r, 3], S - lb + 1))
            mag = full if int(x[r, 1]) & 1 else full // 2
            z[pa:pa + la, pb:pb + lb] = -mag if int(x[r, 0]) & 1 else mag
        x1, x2 = platform(par[4])
        z[x1:x2, x1:x2] = 0
    elif fam in (5, 8):
        m, d, depth = int(par[0] / hs), int(par[1] / hs), int(par[4] / vs)
        p = max(m + d, 1)
        rb = b // p
        rows = S // p + 1
        shift = below(draws(seed, sub, P_STEP_SHIFT if fam == 5 else P_STONE_SHIFT, np.arange(rows))[:, 0], p)
        if info is not None:
            info.update(period=p, size=m, shift=shift)
        t = a + shift[rb]
        if fam == 5:
            stone = np.full((S, S), True) if m >= S else (m >= 1) & (b % p < m) & (t % p < m)
            z = np.where(stone, 0, depth)
        else:
            mh = int(par[2] / vs)
            ca = t // p
            x = draws(seed, sub, P_STONE, (rb * 65536 + ca).reshape(-1)).reshape(S, S, 4)
            sa, sb = m - 1 + below(x[..., 0], 2), m - 1 + below(x[..., 1], 2)
            height = 1 + below(x[..., 2], 2 * mh) if mh >= 1 else np.zeros((S, S), dtype=np.int64)
            z = np.where((b % p < sb) & (t % p < sa), height, depth)
        x1, x2 = platform(par[3])
        z[x1:x2, x1:x2] = 0
    elif fam == 6:
        g, P = int(par[0] / hs), int(par[1] / hs)
        c = S // 2
        x1 = (S - P) // 2
        x2 = x1 + g
        lo, hi = _slice(c - x2, c + x2, S)
        z[lo:hi, lo:hi] = GAP_UNITS
        lo, hi = _slice(c - x1, c + x1, S)
        z[lo:hi, lo:hi] = 0
    elif fam == 7:
        depth, P = int(par[0] / vs), int(par[1] / hs / 2)
        lo, hi = _slice(S // 2 - P, S // 2 + P, S)
        z[lo:hi, lo:hi] = -depth
    else:
        raise ValueError(fam)
    return z


def generate(k: dict) -> dict:
    """The whole table [tot_rows, tot_cols] int16 (border zero), terrain_origins [R, C, 3] float32, and per sub-terrain the family
    index and the generator's arguments."""
    g = geometry(k)
    S, border, R, C = g["S"], g["border"], k["num_rows"], k["num_cols"]
    if k["terrain_length"] != k["terrain_width"]:
        raise ValueError("square sub-terrains only")
    cum = cumulative(k["terrain_proportions"])
    table = np.zeros((g["tot_rows"], g["tot_cols"]), dtype=np.int16)
    origins = np.zeros((R, C, 3), dtype=np.float32)
    family, params = np.zeros((R, C), dtype=np.int64), np.zeros((R, C, 6))
    for i in range(R):
        for j in range(C):
            choice, difficulty = choice_and_difficulty(k, i, j)
            fam, par = make_terrain(choice, difficulty, cum)
            z = np.clip(sub_terrain(k, fam, par, i * C + j), -32768, 32767).astype(np.int16)
            table[border + i * S:border + (i + 1) * S, border + j * S:border + (j + 1) * S] = z
            top = int(z[g["x1"]:g["x2"], g["x1"]:g["x2"]].max())
            origins[i, j] = ((i + 0.5) * k["terrain_length"], (j + 0.5) * k["terrain_width"], top * k["vertical_scale"])
            family[i, j], params[i, j] = fam, par
    return dict(table=table, origins=origins, family=family, params=params, **g)
