"""Trajectory batching helpers for the recurrent (GRU) policy path.

Same contracts as rsl_rl/rsl_rl/utils/utils.py:33-70, implemented as index maps (one scatter /
one masked gather, no per-trajectory Python loop) so they run as a handful of device ops:

    split_and_pad_trajectories(tensor [T,N,...], dones [T,N,1]) -> (padded [T, n_traj, ...], masks [T, n_traj])
    unpad_trajectories(padded [T, n_traj, D], masks [T, n_traj]) -> [T, N, D]

A trajectory ends at every `done` and at the last stored step.  The padded time dimension is
always T (the reference pads to the longest trajectory, which equals T whenever at least one env
ran a full rollout without a reset -- the only case in which its own `unpad` works).
"""
import contextlib
import itertools

import torch

from .export import export_policy_as_jit  # noqa: F401  (legged_gym/utils/helpers.py:150)


def trajectory_index_map(dones):
    """dones [T,N,1] or [T,N] -> (traj_id [N*T], pos [N*T], lengths [n_traj]) in env-major order."""
    d = dones.reshape(dones.shape[0], dones.shape[1]).clone().to(torch.int64)
    d[-1] = 1
    flat = d.transpose(1, 0).reshape(-1)                     # env-major: index = n*T + t
    ends = flat.cumsum(0)
    traj_id = ends - flat                                     # number of trajectory ends strictly before
    n_traj = int(ends[-1])
    end_idx = flat.nonzero()[:, 0]
    start_idx = torch.cat((end_idx.new_zeros(1), end_idx[:-1] + 1))
    lengths = end_idx - start_idx + 1
    pos = torch.arange(flat.numel(), device=flat.device) - start_idx[traj_id]
    return traj_id, pos, lengths, n_traj


def split_and_pad_trajectories(tensor, dones):
    T = tensor.shape[0]
    traj_id, pos, lengths, n_traj = trajectory_index_map(dones)
    src = tensor.transpose(1, 0).reshape(-1, *tensor.shape[2:])
    padded = tensor.new_zeros(T, n_traj, *tensor.shape[2:])
    padded[pos, traj_id] = src
    masks = lengths > torch.arange(0, T, device=tensor.device).unsqueeze(1)
    return padded, masks


def unpad_trajectories(trajectories, masks):
    T = trajectories.shape[0]
    return trajectories.transpose(1, 0)[masks.transpose(1, 0)].view(-1, T, trajectories.shape[-1]).transpose(1, 0)


def true_indices(mask, count):
    """Flat indices of the True entries of `mask` in ascending order WITHOUT a host synchronisation: `count` = their number,
    known to the caller (torch.nonzero / boolean indexing must read it back from the device first).  A stable sort of the negated
    mask puts the True entries first, in their original order."""
    flat = mask.reshape(-1)
    return torch.argsort((~flat).to(torch.uint8), stable=True)[:count]


class UpdateSlots:
    """What a trainer computes once per update and mini-batch slot.  The mini-batches of an update are the same index sets in every
    epoch (rollout_storage.py:165, 217-267), so an operand packed from the rollout for slot i serves all epochs.  `open()` draws a
    generation that never repeats (process-wide) for the duration of a with-block; the trainer sets `slot` per mini-batch.  Outside an
    open generation everything is recomputed on every call."""
    _serial = itertools.count(1)

    def __init__(self):
        self.gen, self.slot, self._keys = None, 0, {}

    @contextlib.contextmanager
    def open(self):
        self.gen, self.slot = next(UpdateSlots._serial), 0
        try:
            yield self
        finally:
            self.gen = None

    def once(self, name, key=()):
        """-> (name of `name`'s buffer for the slot in flight, whether it must be (re)computed): True once per generation, slot and
        `key`; always with no generation open or key None (slot 0 then)."""
        k = None if self.gen is None or key is None else (self.gen, key)
        slot_name = f"{name}@{self.slot if k is not None else 0}"
        fresh = k is None or self._keys.get(slot_name) != k
        self._keys[slot_name] = k
        return slot_name, fresh

    def packed(self, ws, name, make, cols, rows, key=()):
        """Operand image `name` (ws.img) of the slot in flight, packed from the fp32 operand make() once per generation and `key`."""
        slot_name, fresh = self.once(name, key)
        img = ws.img(slot_name, cols)
        if fresh:
            img.pack(make(), rows)
        return img


class PaddedBuffers:
    """Persistent zero-initialised fp32 buffers [rows, width] of the padded [T * n_traj] recurrent layout, by name.  A mini-batch writes
    its valid rows only: the padding rows hold finite values nobody reads (outputs of padding steps are masked out, their gradients are
    zero).  Two zeroing rules: `zero(prefix)` at the start of an update (input projections: later mini-batches leave values of the same
    update there), and `get(..., slots=)`: one buffer per mini-batch slot, zeroed once per update and slot (a slot's valid rows are the
    same in every epoch and every mini-batch overwrites them).
    `grow`: a buffer is re-created only when it is too small (a view of its first rows otherwise; a re-created buffer counts as zeroed);
    else it is re-created whenever its row count changes.  RecurrentPPO and Memory keep the first rule, the decoder trainers the second:
    each keeps the fills it has always launched."""

    def __init__(self, grow):
        self.grow, self._bufs = grow, {}

    def get(self, name, rows, width, dev, slots=None):
        fresh = False
        if slots is not None:
            name, fresh = slots.once(name)
        t = self._bufs.get(name)
        if t is None or t.device != dev or t.shape[1] != width or (t.shape[0] < rows if self.grow else t.shape[0] != rows):
            t = self._bufs[name] = torch.zeros(rows, width, dtype=torch.float32, device=dev)
            fresh = fresh and not self.grow
        if fresh:
            t[:rows].zero_()
        return t[:rows]

    def zero(self, prefix):
        for name, t in self._bufs.items():
            if name.startswith(prefix):
                t.zero_()
