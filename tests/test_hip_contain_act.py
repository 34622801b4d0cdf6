"""dtc_act_contain (csrc/contain_act.hip) against a numpy restatement kept here (the reference project has no such function), byte for
byte over the WHOLE allocation behind every item: what must be zeroed is zero, and nothing else moved -- NaN payloads of scan-only
items, the gaps of a strided matrix, the element in front of a [1:] view and the rows of act_valid next to the one written included.

The items are those of one rollout step: row tensors of width 1 (1-D and [N, 1]), 3, 12, 53, 265 (row stride 272) and 1389 (odd, and
longer than one pass of a wave), a [1, N, 128] state, and the four [2, N, 50] states of an LSTM pair, whose 200-byte rows start at
8 mod 16 in every other env."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
QNAN, PINF, NINF, NEG_NAN = 0x7fc12345, 0x7f800000, 0xff800000, 0xffc00001       # (a quiet NaN with a payload; a negative one)
POISONS = (QNAN, PINF, NINF, NEG_NAN)
# finite patterns that sit next to the rule's edge: FLT_MAX, -FLT_MAX, the smallest denormal, -0.0, +0.0, the largest denormal
NOT_BAD = (0x7f7fffff, 0xff7fffff, 0x00000001, 0x80000000, 0x00000000, 0x007fffff)

# name, shape, mode (0 scan / 1 scan and zero), elements in front of the view, row stride (None: contiguous)
ITEMS = (("obs", (53,), 0, 0, None), ("privileged_obs", (1389,), 0, 0, None), ("obs_history", (265,), 0, 0, 272), ("base_vel", (3,), 0, 0, None),
         ("action_mean", (12,), 0, 0, None), ("values", (1,), 0, 0, None), ("log_prob", (), 0, 0, None),
         ("actions", (12,), 1, 1, None),                                           # a [1:] view: 4-byte, not 16-byte aligned
         ("gru_h", (1, 128), 1, 0, None),
         ("h_a", (2, 50), 1, 0, None), ("c_a", (2, 50), 1, 0, None), ("h_c", (2, 50), 1, 0, None), ("c_c", (2, 50), 1, 0, None))


class Item:
    """One tensor of the step: `back` is the whole allocation as uint32 on the host, `host` its [outer, N, width] view, `dev_back` /
    `dev` the same on the device (dev in the tensor's natural shape: [N], [N, w] or [L, N, H])."""

    def __init__(self, name, shape, mode, offset, row_stride, N, g):
        self.name, self.mode = name, mode
        outer = shape[0] if len(shape) == 2 else 1
        width = shape[-1] if shape else 1
        rs = width if row_stride is None else row_stride
        size = offset + outer * N * rs + 3
        self.back = g.integers(0x30000000, 0x40000000, size=size, dtype=np.uint32)          # finite, all of them
        self.back[g.integers(0, size, size=max(1, size // 9))] ^= np.uint32(0x80000000)       # ... of both signs
        where = g.integers(0, size, size=2 * len(NOT_BAD))
        self.back[where] = np.array(NOT_BAD, dtype=np.uint32)[np.arange(where.size) % len(NOT_BAD)]
        self.geom = (outer, N, width), (N * rs, rs, 1), offset
        self.host = self._view(self.back)
        self.dev_back = torch.from_numpy(self.back.view(np.int32)).to(DEV).view(torch.float32)
        nat_shape = (N,) if shape == () else (N, width) if len(shape) == 1 else (outer, N, width)
        nat_stride = (rs,) if shape == () else (rs, 1) if len(shape) == 1 else (N * rs, rs, 1)
        self.dev = torch.as_strided(self.dev_back, nat_shape, nat_stride, offset)
        assert self.dev.data_ptr() % 16 == (4 * offset) % 16

    def _view(self, back):
        shape, strides, offset = self.geom
        return np.lib.stride_tricks.as_strided(back[offset:], shape, tuple(4 * s for s in strides))

    def upload(self):
        self.dev_back.copy_(torch.from_numpy(self.back.view(np.int32)).view(torch.float32))

    def device_bits(self):
        return self.dev_back.cpu().view(torch.int32).numpy().view(np.uint32)


def _step(N, seed=0, names=None):
    g = np.random.default_rng(seed)
    return [Item(*spec, N, g) for spec in ITEMS if names is None or spec[0] in names]


def _reference(items, N):
    """the rule, in numpy, applied to the host copies in place -> bad [N] (bool)"""
    bad = np.zeros(N, dtype=bool)
    for it in items:
        bad |= ((it.host & np.uint32(0x7f800000)) == np.uint32(0x7f800000)).any(axis=(0, 2))
    for it in items:
        if it.mode == 1:
            it.host[:, bad, :] = 0
    return bad


def _run_and_compare(items, N, what, outputs=(True, True)):
    from dtc_amd import ops
    record = torch.full((3, N), 7, dtype=torch.uint8, device=DEV)          # act() writes row `step` of the [T, N] record
    env_bad = torch.full((N,), 7, dtype=torch.uint8, device=DEV)
    ops.act_contain(scan=[it.dev for it in items if it.mode == 0], repair=[it.dev for it in items if it.mode == 1],
                    act_valid_row=record[1] if outputs[0] else None, env_bad=env_bad if outputs[1] else None)
    bad = _reference(items, N)
    for it in items:
        got = it.device_bits()
        assert np.array_equal(got, it.back), (what, it.name, np.nonzero(got != it.back)[0][:8])
    rec = record.cpu().numpy()
    assert (rec[0] == 7).all() and (rec[2] == 7).all(), what
    assert np.array_equal(rec[1], (~bad).astype(np.uint8) if outputs[0] else np.full(N, 7, dtype=np.uint8)), what
    assert np.array_equal(env_bad.cpu().numpy(), bad.astype(np.uint8) if outputs[1] else np.full(N, 7, dtype=np.uint8)), what
    return bad


def _env_groups(N):
    """env 0, env N - 1, and two neighbours inside one workgroup (four envs each)"""
    pair = (N // 2 // 4 * 4 + 1, N // 2 // 4 * 4 + 2)
    groups = [(0,), (N - 1,)] + ([pair] if pair[1] < N else [])
    return sorted(set(groups))


def _columns(width):
    """element 0, the last one, the first and last few (an unaligned head is at most 3 long), the tail behind the last whole 16-byte
    group counted from the row's start, and one in the middle"""
    cols = {0, 1, 2, 3, width // 2, 4 * ((width - 1) // 4), width - 4, width - 3, width - 2, width - 1}
    return sorted(c for c in cols if 0 <= c < width)


@pytest.mark.parametrize("N", [1, 3, 257])
def test_a_clean_step_is_left_bit_identical_and_every_env_is_reported_valid(N):
    items = _step(N)
    for it in items:                                          # the finite patterns next to the rule's edge, in every item
        for k, v in enumerate(NOT_BAD):
            it.host[-1, (k * 5) % N, (k * 7) % it.host.shape[2]] = v
        it.upload()
    bad = _run_and_compare(items, N, "clean")
    assert not bad.any()


@pytest.mark.parametrize("N", [1, 3, 257])
def test_one_poison_anywhere_flags_its_env_and_zeroes_that_env_alone(N):
    items = _step(N)
    k = 0
    for it in items:
        outer, _, width = it.host.shape
        for col in _columns(width):
            for envs in _env_groups(N):
                o = outer - 1                                 # a stacked state: the LAST layer only
                keep = {i.name: i.back.copy() for i in items}
                for n in envs:
                    it.host[o, n, col] = POISONS[k % len(POISONS)]
                    k += 1
                for i in items:
                    i.upload()
                bad = _run_and_compare(items, N, (it.name, col, envs))
                assert sorted(np.nonzero(bad)[0].tolist()) == sorted(envs)
                # (the restatement zeroed every repair item at these envs, over all layers -- and a scan item keeps its poison)
                for i in items:
                    if i.mode == 1:
                        assert not i.host[:, list(envs), :].any()
                assert it.mode == 1 or it.host[o, envs[0], col] in POISONS
                for i in items:
                    i.back[:] = keep[i.name]
    assert k >= len(items) * 3


def test_many_poisons_at_once_neighbours_and_whole_groups():
    """several bad envs per workgroup, several hits per 16-byte group and per env, hits in scan and repair items of the same env"""
    N = 257
    items = {it.name: it for it in _step(N, seed=3)}
    g = np.random.default_rng(5)
    for _ in range(60):
        it = list(items.values())[int(g.integers(0, len(items)))]
        pos = tuple(int(g.integers(0, d)) for d in it.host.shape)
        it.host[pos] = POISONS[int(g.integers(0, len(POISONS)))]
    items["privileged_obs"].host[0, 8:12, 1385:1389] = QNAN
    items["h_c"].host[1, 100:104, 44:50] = NINF
    items["c_a"].host[0, 256, :] = PINF
    for it in items.values():
        it.upload()
    bad = _run_and_compare(list(items.values()), N, "many")
    assert bad[8:12].all() and bad[100:104].all() and bad[256] and 10 < int(bad.sum()) < 80


@pytest.mark.parametrize("outputs", [(True, False), (False, True), (False, False)])
def test_each_output_is_optional(outputs):
    N = 7
    items = _step(N, seed=1, names=("obs", "log_prob", "actions", "h_a", "c_a"))
    items[0].host[0, 2, 52] = PINF
    items[3].host[1, 5, 0] = QNAN
    for it in items:
        it.upload()
    bad = _run_and_compare(items, N, outputs, outputs)
    assert np.nonzero(bad)[0].tolist() == [2, 5]


def test_scan_only_call_and_strided_views_of_larger_tensors():
    """only scan items and one mask (a monitor's use); a column of a matrix as a 1-D item; a column block with row stride > width"""
    from dtc_amd import ops
    N = 9
    big = torch.randn(N, 40, device=DEV)
    big[4, 17] = float("nan")                                 # outside both views below: not seen
    big[6, 5] = float("inf")                                  # the 1-D view big[:, 5]
    big[1, 29] = float("-inf")                                # the last column of the block big[:, 20:30]
    keep = big.clone()
    env_bad = torch.full((N,), 7, dtype=torch.uint8, device=DEV)
    ops.act_contain(scan=[big[:, 5], big[:, 20:30]], env_bad=env_bad)
    assert env_bad.cpu().tolist() == [0, 1, 0, 0, 0, 0, 1, 0, 0]
    assert torch.equal(big.view(torch.int32), keep.view(torch.int32))
    # the same block as a repair item: rows 1 and 6 of the block are zeroed, the columns around it stay
    ops.act_contain(scan=[big[:, 5]], repair=[big[:, 20:30]], env_bad=env_bad)
    want = keep.clone()
    want[1, 20:30] = 0
    want[6, 20:30] = 0
    assert env_bad.cpu().tolist() == [0, 1, 0, 0, 0, 0, 1, 0, 0]
    assert torch.equal(big.view(torch.int32), want.view(torch.int32))
    with pytest.raises(ValueError, match="element stride"):
        ops.act_contain(repair=[big.t()[20:30]], env_bad=env_bad)          # [10, N] with element stride 40: never copied
    with pytest.raises(ValueError, match="envs"):
        ops.act_contain(scan=[big, torch.zeros(N + 1, 3, device=DEV)], env_bad=env_bad)
