"""dtc_terrain_generate on the GPU against tests/terrain_oracle.py, bit for bit on the table and the origins: every family alone, all
of them in one grid, borders that leave the rows off the 16-byte grid, Lite3's table at full size, the random layout, a table inside a
sentinel-filled buffer at every 2-byte offset, regeneration in place, and the arguments rejected before any launch."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

import terrain_oracle as O

pytestmark = pytest.mark.gpu
NINE = tuple([1 / 9] * 9)


def _cfg(**kw):
    from dtc_amd.terrain import TerrainConfig
    base = dict(terrain_length=4.0, terrain_width=4.0, border_size=1.0, num_rows=3, num_cols=9, terrain_proportions=NINE, seed=7)
    base.update(kw)
    return TerrainConfig(**base)


def _oracle(c):
    return O.generate(O.config(horizontal_scale=c.horizontal_scale, vertical_scale=c.vertical_scale, border_size=c.border_size,
                               curriculum=c.curriculum, terrain_length=c.terrain_length, terrain_width=c.terrain_width, num_rows=c.num_rows,
                               num_cols=c.num_cols, terrain_proportions=c.terrain_proportions, seed=c.seed))


def _check(c, want=None):
    from dtc_amd.terrain import Terrain
    t = Terrain(c, "cuda")
    want = want or _oracle(c)
    assert t.heightsamples is t.height_field_raw and t.height_field_raw.dtype == torch.int16
    assert (t.tot_rows, t.tot_cols, t.border) == (want["tot_rows"], want["tot_cols"], want["border"])
    assert (t.env_length, t.env_width) == (c.terrain_length, c.terrain_width)
    got = t.height_field_raw.cpu().numpy()
    assert got.shape == want["table"].shape and np.array_equal(got, want["table"])
    org = t.env_origins.cpu().numpy()
    assert org.shape == (c.num_rows, c.num_cols, 3) and np.array_equal(org.view(np.int32), want["origins"].view(np.int32))
    return t, want


@pytest.mark.parametrize("fam", range(9), ids=O.FAMILIES)
def test_each_family_alone(fam):
    c = _cfg(num_rows=1, num_cols=1, curriculum=False, terrain_proportions=tuple(float(q == fam) for q in range(9)), seed=5)
    _, want = _check(c)
    assert want["family"][0, 0] == fam and want["table"].any()


def test_all_families_in_one_grid():
    _, want = _check(_cfg())
    assert sorted(set(want["family"].ravel().tolist())) == list(range(9))


@pytest.mark.parametrize("border_size,cells", [(0.35, 6), (0.37, 7), (0.0, 0)])
def test_rows_off_the_16_byte_grid(border_size, cells):
    """border_size 0.35 is int(0.35 / 0.05) = 6 cells in double arithmetic (0.35 / 0.05 = 6.999...), as the reference computes it: rows
    of 732 cells, 1464 bytes, not a multiple of 16.  0.37 gives the 7 cells and an odd pitch of 734 cells."""
    c = _cfg(border_size=border_size)
    t, _ = _check(c)
    assert t.border == cells and t.tot_cols == 720 + 2 * cells
    assert cells == 0 or (t.tot_cols * 2) % 16 != 0


def test_lite3_table_at_full_size():
    from dtc_amd.terrain import TerrainConfig
    t, want = _check(TerrainConfig(seed=3))
    assert (t.tot_rows, t.tot_cols) == (1760, 1120) and np.array_equal(want["family"], np.tile([2, 4], (6, 1)))


def test_random_layout():
    c = _cfg(num_rows=4, num_cols=4, curriculum=False, seed=9)
    _, want = _check(c)
    assert len(set(want["family"].ravel().tolist())) >= 4


def test_other_scales():
    _check(_cfg(horizontal_scale=0.1, vertical_scale=0.01, terrain_length=8.0, terrain_width=8.0, border_size=2.0, num_rows=4, seed=11))


@pytest.mark.parametrize("offset", range(8))
def test_nothing_outside_the_table_is_written(offset):
    """The table at every 2-byte offset from a 16-byte boundary inside a sentinel-filled buffer: the table equals the oracle, every
    other element keeps the sentinel."""
    from dtc_amd.terrain import Terrain
    c = _cfg(num_rows=1, num_cols=2, border_size=0.35, terrain_proportions=(0, 0, 0, 0, 0, .5, 0, 0, .5))
    want = _oracle(c)
    n = want["table"].size
    buf = torch.full((n + 64,), 0x5A5A, dtype=torch.int16, device="cuda")
    org = torch.full((1 * 2 * 3 + 16,), 7.5, device="cuda")
    assert buf.data_ptr() % 16 == 0
    table = buf[24 + offset:24 + offset + n].view(want["table"].shape)
    t = Terrain(c, "cuda", out=table)
    t.env_origins = org[8:14].view(1, 2, 3)
    buf[24 + offset:24 + offset + n] = 0x5A5A
    t.generate()
    got = buf.cpu().numpy()
    assert np.array_equal(got[24 + offset:24 + offset + n].reshape(want["table"].shape), want["table"])
    assert (got[:24 + offset] == 0x5A5A).all() and (got[24 + offset + n:] == 0x5A5A).all()
    o = org.cpu().numpy()
    assert np.array_equal(o[8:14].reshape(1, 2, 3).view(np.int32), want["origins"].view(np.int32)) and (o[:8] == 7.5).all() and (o[14:] == 7.5).all()


def test_generate_again_replaces_the_layout_in_place():
    c = _cfg(seed=1)
    t, first = _check(c)
    ptr, optr = t.height_field_raw.data_ptr(), t.env_origins.data_ptr()
    holder = t.heightsamples
    t.generate(seed=2)
    second = _oracle(dataclasses.replace(c, seed=2))
    assert t.height_field_raw.data_ptr() == ptr and t.env_origins.data_ptr() == optr and t.seed == 2
    assert np.array_equal(holder.cpu().numpy(), second["table"]) and not np.array_equal(first["table"], second["table"])
    assert np.array_equal(t.env_origins.cpu().numpy().view(np.int32), second["origins"].view(np.int32))
    t.generate(seed=1)
    assert np.array_equal(holder.cpu().numpy(), first["table"])


def test_bad_arguments_are_rejected_before_any_launch():
    from dtc_amd import _ffi
    from dtc_amd.terrain import Terrain
    t = Terrain(_cfg(num_rows=1, num_cols=1), "cuda")
    before = t.height_field_raw.clone()
    lib = _ffi.lib()

    def call(**kw):
        c = t.cfg_struct()
        for k, v in kw.items():
            setattr(c, k, v)
        return lib.dtc_terrain_generate(c, _ffi.ptr(t.height_field_raw), _ffi.ptr(t.env_origins), _ffi.stream())

    assert call() == 0
    assert call(terrain_width=8.0) == -1 and b"terrain_width" in lib.dtc_last_error()
    # 40 x 40 sub-terrains of 8 m at 0.05 m: 6400 x 6400 cells per side of the grid = 2^31 + ... cells
    assert call(num_rows=290, num_cols=290, terrain_length=8.0, terrain_width=8.0, tot_rows=46440, tot_cols=46440) == -1
    assert b"2^31" in lib.dtc_last_error()
    assert call(tot_rows=t.tot_rows + 1) == -1                                            # a table of another shape than the geometry's
    assert call(horizontal_scale=0.0) == -1 and call(terrain_length=1.0, terrain_width=1.0) == -1
    assert lib.dtc_terrain_generate(None, _ffi.ptr(t.height_field_raw), _ffi.ptr(t.env_origins), _ffi.stream()) == -1
    assert lib.dtc_terrain_generate(t.cfg_struct(), None, _ffi.ptr(t.env_origins), _ffi.stream()) == -1
    torch.cuda.synchronize()
    assert torch.equal(t.height_field_raw, before)
    sizes = (C.c_int64 * 4)()
    assert lib.dtc_terrain_abi_sizes(sizes, 4) == 1 and sizes[0] == C.sizeof(_ffi.DtcTerrainCfg) == 144
