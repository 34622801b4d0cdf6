"""The two GRU heads of the recurrent trainers' policy step on operand images (dtc_amd/h2i.py), shared by RecurrentPPO and
RecurrentDecoderPPO: a 1-layer GRU with H % 128 == 0 per head, a mini-batch of M valid rows in the padded [T, R] layout (`unpad_idx`:
the padded row of each valid row, time-major).

A head runs in three parts -- input projection over the valid rows | recurrence over the padded layout | MLP on the valid rows --, the
critic's on the `aux` lane, the actor's on main; with DTC_GRU_MULTI=1 the two recurrences advance TOGETHER on the main lane instead
(ops.gru_fwd_multi / gru_bwd_multi: one launch per time step for both).  Backward: MLP -> row scatter into the padded layout ->
dtc_gru_bwd -> the recurrence's weight gradients over the valid rows (dgh_all taken from dtc_gru_bwd's workspace, dgi and h_{t-1}
gathered into images).  Every weight gradient leaves as a job (dZimg, Ximg, gW, wcol0, gb) for the trainer's `sink`.

With DTC_GRU_H2I=1 (dtc_set_gru_h2i; opt-in) the recurrence itself runs on operand images (csrc/gru_h2i.hip: ops.gru_fwd_h2i /
gru_bwd_h2i) and its kernels write the valid-row images the rest of the step reads -- hx, hp and the gate-gradient images -- through
`slot_row`, the inverse of `unpad_idx`: none of the packs above is launched.  The two heads then stay on their two lanes:
DTC_GRU_MULTI and DTC_GRU_SEQ* are ignored.
"""
from __future__ import annotations

import os

import torch

from .. import _ffi, h2i, ops
from .._ffi import seg, segmat


def seq_pair(T, R, H):
    """Both forward recurrences as ONE persistent launch (dtc_gru_fwd_multi -> dtc_gru_seq_fwd_pair) where that serves the shape: opt-in
    (DTC_GRU_SEQ=1 DTC_GRU_SEQ_PAIR=1), measured slower than two lanes."""
    return (os.environ.get("DTC_GRU_SEQ_PAIR", "0") == "1" and ops.SPLIT
            and bool(_ffi.lib().dtc_gru_seq_supported(int(T), int(R), int(H), 1)))


class GruHead:
    """One head: `mem` (a 1-layer GRU Memory) from the initial state h0 [R, H], then the MLP `layers`.  `dgi_image`: the head's input
    needs its data gradient (the composite's actor) -- dgh and dgi leave as whole [M, 3H] images (`dgii`).  Otherwise dgh and dgi share
    their r / z gate blocks (gru_gate_bwd_kernel: da_n vs da_n * r in the n block only): those 2H columns are packed once and each
    weight gradient runs as two jobs over the row ranges [0, 2H) and [2H, 3H)."""

    def __init__(self, tw, wset, slots, name, mem, layers, h0, unpad_idx, T, R, sink, dgi_image=False):
        self.tw, self.wset, self.slots, self.sink = tw, wset, slots, sink
        self.name, self.mem, self.layers, self.h0 = name, mem, layers, h0.contiguous()
        self.unpad_idx, self.T, self.R, self.dgi_image = unpad_idx, T, R, dgi_image
        self.H, self.M, self.dev = mem.hidden_size, unpad_idx.numel(), unpad_idx.device

    def _rows(self, t, c0, w):
        """Columns [c0, c0 + w) of the valid rows of the padded [T * R, .] tensor t, as a row-gathered operand (of a pack: it may be wide)."""
        return segmat([seg(t, c0, w, gather=True, wide=True)], self.unpad_idx)

    def project(self, X, cols=None, run=True):
        """Input projection of the valid rows (X: an image or a list of images, `cols`: W_ih's first column for each), scattered into the
        padded layout, then the forward recurrence (run=False: the caller runs both heads' in one launch)."""
        tw, mem, T, R, H = self.tw, self.mem, self.T, self.R, self.H
        self.X, self.cols = X, cols
        gi_v = tw.g("gi_" + self.name, 3 * H)
        h2i.linear_fwd(X, mem.W_ih, mem.b_ih, gi_v, None, None, wset=self.wset, cols=cols)
        self.gi = tw.padded("gi_" + self.name, T * R, 3 * H)
        ops.scatter_rows(gi_v, self.unpad_idx, self.gi)
        self.hs_all = torch.empty(T + 1, R, H, device=self.dev)
        self.gates, self.hn = torch.empty(T, R, 3 * H, device=self.dev), torch.empty(T, R, H, device=self.dev)
        self.on_images = ops.gru_h2i_on()
        if self.on_images:
            # the forward kernels write h_t straight into the MLP's input image (hs_all[1:] un-padded) and into the h_{t-1} operand of
            # the W_hh weight gradient (hs_all[:T] un-padded): every one of the M rows, in every step
            self.ws = ops.workspace(ops.gru_h2i_workspace_bytes(T, R, H), self.dev)
            self.slot_row = self._slot_row()
            self.hxi, self.hpi = self._img("hx_", H), self._img("hp_", H)
            ops.gru_fwd_h2i(*self.fwd_item(), self.slot_row, self.hxi, self.hpi)
            return
        self.ws = ops.workspace(ops.gru_workspace_bytes(T, R, H), self.dev)
        if run:
            ops.gru_fwd(*self.fwd_item())

    def _img(self, prefix, width):
        """A valid-row image the recurrence kernels write: exactly M rows, so that no row keeps what an earlier step left there."""
        im = self.tw.img(prefix + self.name, width)
        if im.M != self.M:
            raise _ffi.DtcError(f"image {prefix + self.name} has {im.M} rows, the mini-batch {self.M}: the step workspace must be the mini-batch's")
        return im

    def _slot_row(self):
        """int32 [T * R]: the valid row of each padded slot or -1, built on the device once per update and mini-batch slot (the generator
        yields the same trajectories in every epoch), per head: each head builds and reads its own on its own lane."""
        name, fresh = self.slots.once("slot_row_" + self.name)
        cache = self.tw.slot_rows
        if fresh or name not in cache or cache[name].numel() != self.T * self.R:
            cache[name] = ops.gru_slot_row(self.unpad_idx, self.T * self.R)
        return cache[name]

    def fwd_item(self):
        return (self.gi.view(self.T, self.R, 3 * self.H), self.h0, self.mem.W_hh, self.mem.b_hh, self.hs_all, self.gates, self.hn, self.ws)

    def mlp(self):
        """The MLP on the un-padded recurrence outputs (a row-gathered image); its hidden activations leave as fp32 (ELU derivative) AND
        as images."""
        tw, name, H = self.tw, self.name, self.H
        hx = self.hxi if self.on_images else tw.img("hx_" + name, H).pack(self._rows(self.hs_all[1:].reshape(self.T * self.R, H), 0, H), self.M)
        self.outs, self.imgs = [], [hx]
        for li, L in enumerate(self.layers):
            o = tw.g(f"{name}_o{li}", L.n_out)
            oi = tw.img(f"{name}_o{li}", L.n_out) if li < len(self.layers) - 1 else None
            h2i.linear_fwd(self.imgs[-1], L.W, L.b, o, oi, L.act, wset=self.wset)
            self.outs.append(o)
            self.imgs.append(oi)

    def mlp_backward(self, dOut, run=True):
        """MLP backward down to the padded gradient of the recurrence's outputs, then BPTT (run=False: the caller runs both heads' in one
        launch).  That padded buffer is zeroed once per update and mini-batch slot: a slot's padding rows are the same in every epoch,
        every scatter overwrites its valid rows (32 of 40 fills of 72 MB per step saved)."""
        tw, name, layers, T, R, H = self.tw, self.name, self.layers, self.T, self.R, self.H
        dZi = tw.img("dout_" + name, dOut.shape[1]).pack(dOut)
        d_in = tw.g(f"{name}_d0", H)
        for li in range(len(layers) - 1, -1, -1):
            L = layers[li]
            self.sink(dZi, self.imgs[li], L.gW, 0, L.gb)
            if li > 0:
                dXi = tw.img(f"{name}_d{li}", L.n_in)
                h2i.linear_dgrad(dZi, L.W, None, dXi, Xsaved=self.outs[li - 1], act=layers[li - 1].act, wset=self.wset)
                dZi = dXi
            else:
                h2i.linear_dgrad(dZi, L.W, d_in, None, wset=self.wset)
        self.dhs = tw.padded("dhs_" + name, T * R, H, slots=self.slots)
        ops.scatter_rows(d_in, self.unpad_idx, self.dhs)
        self.dgi, self.dh0 = torch.empty(T, R, 3 * H, device=self.dev), torch.empty(R, H, device=self.dev)
        if self.on_images:
            # the gate kernel writes the un-padded rows of dgh / dgi as the images recurrence_grads() hands to `sink`
            if self.dgi_image:
                self.gimgs = dict(dgh=self._img("dgh_", 3 * H), dgi_img=self._img("dgi_", 3 * H))
            else:
                self.gimgs = dict(drz=self._img("drz_", 2 * H), dnh=self._img("dnh_", H), dni=self._img("dni_", H))
            ops.gru_bwd_h2i(*self.bwd_item(), self.slot_row, **self.gimgs)
            return
        if run:
            ops.gru_bwd(self.dhs.view(T, R, H), self.hs_all, self.gates, self.hn, self.mem.W_hh, self.dgi, None, None, self.dh0, self.ws)

    def bwd_item(self):
        return (self.dhs.view(self.T, self.R, self.H), self.hs_all, self.gates, self.hn, self.mem.W_hh, self.dgi, self.dh0, self.ws)

    def recurrence_grads(self):
        """Behind the BPTT: the weight-gradient jobs of W_hh and W_ih over the valid rows."""
        tw, mem, name, T, R, H, M, sink = self.tw, self.mem, self.name, self.T, self.R, self.H, self.M, self.sink
        if self.on_images:
            hpi, gi = self.hpi, self.gimgs
            if self.dgi_image:
                self.dgii = gi["dgi_img"]
                sink(gi["dgh"], hpi, mem.gW_hh, 0, mem.gb_hh)
                for i, (xi, c0) in enumerate(zip(self.X, self.cols)):
                    sink(self.dgii, xi, mem.gW_ih, c0, mem.gb_ih if i == 0 else None)
                return
            for X, gW, gb, ni in ((hpi, mem.gW_hh, mem.gb_hh, gi["dnh"]), (self.X, mem.gW_ih, mem.gb_ih, gi["dni"])):
                sink(gi["drz"], X, gW[:2 * H], 0, gb[:2 * H])
                sink(ni, X, gW[2 * H:], 0, gb[2 * H:])
            return
        hpi = tw.img("hp_" + name, H).pack(self._rows(self.hs_all[:T].reshape(T * R, H), 0, H), M)
        dgh, dgi = ops.gru_dgh_all(self.ws, T, R, H), self.dgi.view(T * R, 3 * H)
        if self.dgi_image:
            dghi = tw.img("dgh_" + name, 3 * H).pack(self._rows(dgh, 0, 3 * H), M)
            self.dgii = tw.img("dgi_" + name, 3 * H).pack(self._rows(dgi, 0, 3 * H), M)
            sink(dghi, hpi, mem.gW_hh, 0, mem.gb_hh)
            for i, (xi, c0) in enumerate(zip(self.X, self.cols)):
                sink(self.dgii, xi, mem.gW_ih, c0, mem.gb_ih if i == 0 else None)
            return
        rzi = tw.img("drz_" + name, 2 * H).pack(self._rows(dgh, 0, 2 * H), M)
        nhi = tw.img("dnh_" + name, H).pack(self._rows(dgh, 2 * H, H), M)
        nii = tw.img("dni_" + name, H).pack(self._rows(dgi, 2 * H, H), M)
        for X, gW, gb, ni in ((hpi, mem.gW_hh, mem.gb_hh, nhi), (self.X, mem.gW_ih, mem.gb_ih, nii)):
            sink(rzi, X, gW[:2 * H], 0, gb[:2 * H])
            sink(ni, X, gW[2 * H:], 0, gb[2 * H:])


def forward_backward(tw, critic, actor, critic_input, actor_input, loss, multi, done=None):
    """Both heads forward and backward on the lanes of `tw` (begun by the caller).  critic_input() / actor_input() -> (X, cols) of a
    head's input projection, called on its lane (the actor's once the critic's projection is out: the composite runs its encoders
    there); loss(mean, value) -> (dmean, dval), on main between the passes; done(head), if given, on the head's lane once its last
    weight-gradient job is out.  `multi`: DTC_GRU_MULTI."""
    if ops.gru_h2i_on():
        multi = multi_fwd = False                   # the image recurrences run per head, each on its lane
    else:
        multi_fwd = multi or seq_pair(actor.T, actor.R, actor.H)
    with tw.lane("aux"):
        critic.project(*critic_input(), run=not multi_fwd)
    actor.project(*actor_input(), run=not multi_fwd)
    if multi_fwd:
        tw.order("aux", "main")                     # the critic's input projection is written
        ops.gru_fwd_multi([actor.fwd_item(), critic.fwd_item()])
        tw.order("main", "aux")
    with tw.lane("aux"):
        critic.mlp()
    actor.mlp()
    tw.order("aux", "main")
    dmean, dval = loss(actor.outs[-1], critic.outs[-1])
    tw.order("main", "aux")
    with tw.lane("aux"):
        critic.mlp_backward(dval, run=not multi)
    actor.mlp_backward(dmean, run=not multi)
    if multi:
        tw.order("aux", "main")
        ops.gru_bwd_multi([actor.bwd_item(), critic.bwd_item()])
        tw.order("main", "aux")
    for head, lane in ((critic, "aux"), (actor, "main")):
        with tw.lane(lane):
            head.recurrence_grads()
            if done is not None:
                done(head)
