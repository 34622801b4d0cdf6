"""PPO for the GRU + CE-net composite (ActorCriticDecoderRecurrent) -- BASELINE.json config 5.

Per recurrent mini-batch (N/4 envs x all 24 steps, rollout_storage.py:217-267) exactly the two optimisation steps
of ppo.py:189-338 (SURVEY.md §8a "Config 5"):
  1. the VAE step of `PPO` (inherited unchanged) on the valid (t, env) rows of the env slice -- the outlier
     statistics of the CE-net never see padding;
  2. the policy step with BPTT: CE-net / terrain encoder features -> GRU input projections on the valid rows
     (feature blocks are segments of the GEMM operand, nothing is concatenated) -> row scatter into the padded
     [T, n_traj] layout -> dtc_gru_fwd -> MLP heads with the un-padding folded in as a row gather -> fused PPO loss
     -> MLP backward -> row scatter -> dtc_gru_bwd -> row gather -> input-projection backward, whose data gradient
     fans out to z, mu[:, :3] and l_t -> CE-net / terrain encoder backward -> clip + Adam.
Hidden states are recorded BEFORE each rollout step (the convention of the commented lines ppo.py:138-139) and the
mini-batch takes the states at its trajectory starts, as `reccurent_mini_batch_generator` does.
LSTM and stacked memories (`rnn_type='lstm'`, `rnn_num_layers > 1`) run the fp32 schedule above layer by layer: layer 0
projects the composite features, layer k > 0 the valid rows of layer k-1's outputs; LSTM recurrences go forward through
dtc_lstm_fwd_fused (one fused launch per time step) and back through dtc_lstm_bwd, BPTT runs top-down, and layer 0's dgi
feeds the encoders as the 1-layer GRU's does.  The operand-image schedule serves the 1-layer GRU with H % 128 == 0 only.
Same constructor keywords / method names as `PPO`; weight gradients run on the side stream (see PPO._bwd).
"""
from __future__ import annotations

import contextlib
import os

import torch

from .. import _ffi, distributed as dp, h2i, ops
from .._ffi import seg, segmat
from ..modules.actor_critic_decoder import Dense
from ..modules.actor_critic_decoder_recurrent import ActorCriticDecoderRecurrent
from ..utils import split_and_pad_trajectories, true_indices
from .ppo import PPO, S_GNORM, S_SURR, STAT_COLS, Schedule, read_act_record, read_env_record, require_env_record
from .recurrent_heads import GruHead, forward_backward
from .recurrent_ppo import _share_rule


class RecurrentDecoderPPO(PPO):
    actor_critic: ActorCriticDecoderRecurrent
    row_sets = False                 # the mini-batches of update() are trajectories (recurrent_slices)
    # DTC_GRU_MULTI=1: the actor's and the critic's recurrence advance together, one launch per time step (dtc_gru_fwd_multi /
    # dtc_gru_bwd_multi; bit-identical).  Off: measured 136 vs 129 ms per step against one chain of launches per recurrence, each on
    # its own lane
    gru_multi = os.environ.get("DTC_GRU_MULTI", "0") == "1"

    # ---------------------------------------------------------------- rollout side
    def act(self, obs, privileged_obs, obs_history, base_vel, rew_buf=None):
        self._require_gpu()
        ac = self.actor_critic
        ac.ensure_arena()
        ac._ensure_hidden(obs.shape[0], obs.device)
        hidden = tuple(m.clone_hidden(h) for m, h in zip((ac.memory_a, ac.memory_c), ac.get_hidden_states()))   # state BEFORE this step
        actions = super().act(obs, privileged_obs, obs_history, base_vel, rew_buf)
        self.transition.hidden_states = hidden
        return actions

    def compute_returns(self, last_critic_obs, last_critic_privileged_obs, last_base_vel):
        self._require_gpu()
        ac = self.actor_critic
        keep = ac.memory_c.clone_hidden(ac.memory_c.hidden_states)
        if self.contain_nonfinite_act:             # (as in act(): a non-finite last observation costs its own env the bootstrap value, no other)
            with ops.rows_to_themselves():
                last_values = ac.evaluate(last_critic_obs, last_critic_privileged_obs, last_base_vel).detach()
        else:
            last_values = ac.evaluate(last_critic_obs, last_critic_privileged_obs, last_base_vel).detach()
        ac.memory_c.hidden_states = keep            # the bootstrap value must not advance the critic's state
        self.storage.compute_returns(last_values, self.gamma, self.lam)

    # ---------------------------------------------------------------- recurrent mini-batches as index data
    def recurrent_slices(self, hid_a=None, hid_c=None):
        """Yield, per mini-batch of envs [a, b): time-major flat row indices of its samples, the padded-layout
        row of each sample (`unpad_idx`), T, n_traj and the hidden states at the trajectory starts.
        hid_a / hid_c: saved states [T, L, N, H], or a tuple (h, c) of two such for an LSTM (default: the storage's).  The
        states at the trajectory starts are [R, H] for a 1-layer GRU (layer 0), else [L, R, H] (a pair of them for an LSTM).
        For an LSTM the critic receives the ACTOR's saved states, as the storage's recurrent generator hands them out
        (`lstm_critic_states`, rollout_storage.py:261-262)."""
        st = self.storage
        T, N = st.num_transitions_per_env, st.num_envs
        dev = st.dones.device
        as_list = lambda h: list(h) if isinstance(h, (tuple, list)) else [h]
        hid_a = as_list(st.saved_hidden_states_a if hid_a is None else hid_a)
        hid_c = as_list(st.saved_hidden_states_c if hid_c is None else hid_c)
        plain = len(hid_a) == 1 and hid_a[0].shape[1] == 1
        actor_states_for_critic = len(hid_a) > 1 and getattr(st, "lstm_critic_states", "reference") == "reference"
        mb = N // self.num_mini_batches
        _, masks_all = split_and_pad_trajectories(st.dones, st.dones)
        dones = st.dones.squeeze(-1)
        lwd = torch.zeros_like(dones, dtype=torch.bool)
        lwd[1:] = dones[:-1].bool()
        lwd[0] = True
        counts = lwd.view(T, self.num_mini_batches, mb).sum(dim=(0, 2)).tolist()     # one host sync per update
        first = 0
        for i in range(self.num_mini_batches):
            a, b = i * mb, (i + 1) * mb
            last = first + int(counts[i])
            masks = masks_all[:, first:last]
            R = last - first
            flat_rt = true_indices(masks.transpose(1, 0), mb * T)      # no nonzero() sync: the count is known
            traj, pos = flat_rt // T, flat_rt % T
            unpad_idx = (pos * R + traj).view(mb, T).transpose(1, 0).reshape(-1).contiguous()
            idx = (torch.arange(T, device=dev).unsqueeze(1) * N + torch.arange(a, b, device=dev)).reshape(-1).contiguous()
            starts = true_indices(lwd[:, a:b].permute(1, 0), R)      # (env, t) of every trajectory start, env-major; count known
            s_env, s_t = a + starts // T, starts % T
            if plain:
                pick = lambda hs: hs[0][s_t, 0, s_env].contiguous()      # [R, H]: layer 0's saved state at every trajectory start
            else:
                pick1 = lambda h: h[s_t, :, s_env].transpose(0, 1).contiguous()          # [L, R, H]
                pick = lambda hs: pick1(hs[0]) if len(hs) == 1 else tuple(pick1(h) for h in hs)
            ha = pick(hid_a)
            hc = ha if actor_states_for_critic else pick(hid_c)
            yield dict(a=a, b=b, idx=idx, unpad_idx=unpad_idx, T=T, R=R, hid_a=ha, hid_c=hc)
            first = last

    # ---------------------------------------------------------------- policy step with BPTT
    def _image_mode(self, fw, ragged=False):
        """The recurrent schedules (padded [T, R] layout, GRU time steps on images) are built for whole 128-row tiles: no ragged form."""
        return fw.B % 128 == 0 and super()._image_mode(fw, False)

    def _memory_images(self):
        """The operand-image schedule of the policy step is built for 1-layer GRU memories with H % 128 == 0."""
        ac = self.actor_critic
        return (all(m.kind == 'gru' and m.num_layers == 1 for m in (ac.memory_a, ac.memory_c)) and ac.rnn_hidden_size % 128 == 0)

    def _ppo_step_recurrent(self, fw, tw, flat, bt, eps, stats, cfg):
        sched = tw.schedule
        if sched.images and self._memory_images():
            # every GEMM outside the GRU time steps on operand images (dtc_amd/h2i.py), as in PPO._ppo_step
            early = self._run_phase("ppo_recurrent", fw, tw, self._ppo_recurrent_forward_backward_images, flat, bt, eps, stats, cfg)
        else:
            tw.schedule = Schedule()                               # this phase alone runs on the converting kernels, whatever the VAE step ran on
            with self._images("ppo_recurrent"):                    # weight images of the step's split-path layers: one launch
                early = self._ppo_recurrent_forward_backward(fw, tw, flat, bt, eps, stats, cfg)
            tw.schedule = sched
        if not early:
            self._allreduce_grads(self.optimizer)
        self._lr_from_header(stats)
        if self.capture_grads:
            self.captured["main"] = self.actor_critic.arena.grad.clone()
        self.optimizer.step(self.max_grad_norm, stats[S_GNORM:S_GNORM + 1])

    def _ppo_recurrent_forward_backward(self, fw, tw, flat, bt, eps, stats, cfg):
        ac = self.actor_critic
        H, M = ac.rnn_hidden_size, tw.B
        idx, unpad_idx, T, R = bt["idx"], bt["unpad_idx"], bt["T"], bt["R"]
        dev = idx.device
        # lanes: the critic head (raw-input features -> GRU -> MLP) is independent of the CE-net / terrain encoders and
        # of the actor head until the loss, and again until the optimiser step: it runs on `aux`, the small per-time-
        # step kernels of the two recurrences overlap
        _ffi.lib().dtc_set_concurrency_hint(int(bool(self.overlap_wgrad)))
        tw.begin(self.overlap_lanes and self.overlap_wgrad)
        Xa = ac.actor_input(fw, flat["observations"], idx)
        Xc = ac.critic_input(flat["observations"], flat["base_vel"], flat["privileged_observations"], idx)

        def head_forward(name, X, mem, proj, layers, hid):
            """Every layer of the memory (layer 0 projects the features X, layer k > 0 the valid rows of layer k-1's outputs),
            then the MLP head on the valid rows of the top layer's outputs."""
            G = mem.G
            h0, c0 = mem._split(hid)
            recs, cur = [], X
            for l in range(mem.num_layers):
                key = name if l == 0 else f"{name}{l}"
                lin = proj if l == 0 else Dense(mem.Wih[l], mem.bih[l], mem.gWih[l], mem.gbih[l], None)
                gi_v = tw.g("gi_" + key, G * H)
                ops.linear_fwd(cur, lin.W, lin.b, gi_v, None, M=M)
                gi_p = tw.padded("gi_" + key, T * R, G * H)     # padded steps keep finite stale values (never used)
                ops.scatter_rows(gi_v, unpad_idx, gi_p)
                hs_all = torch.empty(T + 1, R, H, device=dev)
                rec = dict(X=cur, lin=lin, hs_all=hs_all, gates=torch.empty(T, R, G * H, device=dev))
                if mem.kind == 'gru':
                    rec.update(hn=torch.empty(T, R, H, device=dev), ws=ops.workspace(ops.gru_workspace_bytes(T, R, H), dev))
                    ops.gru_fwd(gi_p.view(T, R, 3 * H), h0[l].contiguous(), mem.Whh[l], mem.bhh[l], hs_all, rec["gates"], rec["hn"],
                                rec["ws"])
                else:
                    rec.update(cs_all=torch.empty(T + 1, R, H, device=dev), ws=ops.workspace(ops.lstm_workspace_bytes(T, R, H), dev))
                    ops.lstm_fwd_fused(gi_p.view(T, R, 4 * H), h0[l].contiguous(), c0[l].contiguous(), mem.Whh[l], mem.bhh[l], hs_all,
                                       rec["cs_all"], rec["gates"], rec["ws"])
                recs.append(rec)
                cur = segmat([seg(hs_all[1:].reshape(T * R, H), 0, H, gather=True)], unpad_idx)
            X0 = cur
            outs = []
            for li, L in enumerate(layers):
                o = tw.g(f"{name}_o{li}", L.n_out)
                ops.linear_fwd(cur, L.W, L.b, o, L.act, M=M)
                outs.append(o)
                cur = o
            return dict(name=name, X=X, mem=mem, proj=proj, layers=layers, recs=recs, X0=X0, outs=outs)

        def head_backward(hd, dOut):
            name, layers, outs = hd["name"], hd["layers"], hd["outs"]
            dZ = dOut
            for li in range(len(layers) - 1, -1, -1):
                dX = tw.g(f"{name}_d{li}", layers[li].n_in)
                if li > 0:
                    self._bwd(tw, layers[li], dZ, outs[li - 1], dX, outs[li - 1], layers[li - 1].act)
                else:
                    self._bwd(tw, layers[li], dZ, hd["X0"], dX, None, None)
                dZ = dX
            # BPTT top-down; returns layer 0's dgi over the valid rows (the caller runs its input projection's backward)
            mem = hd["mem"]
            G = mem.G
            for l in range(mem.num_layers - 1, -1, -1):
                rec, key = hd["recs"][l], (name if l == 0 else f"{name}{l}")
                dhs = tw.padded("dhs_" + key, T * R, H)
                dhs.zero_()
                ops.scatter_rows(dZ, unpad_idx, dhs)
                dgi_p, dh0 = torch.empty(T, R, G * H, device=dev), torch.empty(R, H, device=dev)
                if mem.kind == 'gru':
                    ops.gru_bwd(dhs.view(T, R, H), rec["hs_all"], rec["gates"], rec["hn"], mem.Whh[l], dgi_p, mem.gWhh[l], mem.gbhh[l],
                                dh0, rec["ws"], rows=unpad_idx)          # the W_hh weight gradient skips the padding slots
                else:
                    ops.lstm_bwd(dhs.view(T, R, H), rec["hs_all"], rec["cs_all"], rec["gates"], mem.Whh[l], dgi_p, mem.gWhh[l],
                                 mem.gbhh[l], dh0, torch.empty(R, H, device=dev), rec["ws"])
                dgi = ops.gather_rows(dgi_p.view(T * R, G * H), unpad_idx, out=tw.g("dgi_" + key, G * H))
                if l == 0:
                    return dgi
                dZ = tw.g(f"dx_{key}", H)                 # gradient w.r.t. layer l-1's outputs (valid rows)
                self._bwd(tw, rec["lin"], dgi, rec["X"], dZ, None, None)

        with tw.lane("aux"):
            hc = head_forward("c", Xc, ac.memory_c, ac.proj_c, ac.Cr, bt["hid_c"])
        ac.cenet_forward_(fw, flat["observation_histories"], eps, idx, masks=self.relu_masks)
        ac.terrain_encoder_(fw, flat["privileged_observations"], idx, masks=self.relu_masks)
        ha = head_forward("a", Xa, ac.memory_a, ac.proj_a, ac.A, bt["hid_a"])
        tw.order("aux", "main")
        if self.after_forward_hook is not None:
            self.after_forward_hook(fw, "ppo")
        mean, value = ha["outs"][-1], hc["outs"][-1]
        ops.ppo_loss(mean, ac.std_view, value, flat["actions"], flat["actions_log_prob"], flat["mu"], flat["sigma"],
                     flat["advantages"], flat["returns"], flat["values"], idx, cfg, tw.dmean, tw.dval, ac.std_grad,
                     stats[S_SURR:S_SURR + 4], self.optimizer.lr_dev, tw.loss_ws)
        self._kl_to_header(stats)
        tw.order("main", "aux")
        with tw.lane("aux"):
            self._bwd(tw, hc["proj"], head_backward(hc, tw.dval), hc["X"])
        dgi_a = head_backward(ha, tw.dmean)
        # the actor features' gradient fans out to z, mu[:, :3], l_t (observations need none)
        tw.dmulv.zero_()
        dst = segmat([seg(None, 0, ac.num_obs), seg(tw.dz, 0, 16), seg(tw.dmulv, 0, 3), seg(tw.dlt, 0, 512)])
        self._bwd(tw, ha["proj"], dgi_a, ha["X"], dst, None, None)
        # every gradient of the first bucket (both MLP heads, both GRUs, both input projections, std) has been written or
        # queued: it travels (with the KL header) while the encoders run backward
        early = self._exchange_bucket(tw, "main_only")
        ops.cenet_latent_bwd(tw.dmulv, tw.dz, eps, fw.mulv, fw.mask, fw.info, fw.lat_ws)
        self._terrain_encoder_backward(fw, tw, flat, idx)
        self._cenet_encoder_backward(fw, tw, flat, idx)
        if early:
            self._exchange_bucket(tw, "shared")
        self._join(tw)
        return early

    def _ppo_recurrent_forward_backward_images(self, fw, tw, flat, bt, eps, stats, cfg, wset):
        """The policy step with BPTT on operand images: encoders as in PPO._ppo_forward_backward, the GRU heads as in
        recurrent_heads.py -- the critic's input projection reads its input packed once per update and mini-batch, the actor's reads the
        l_t image + the packed observations + the latent kernel's [z | mu[:, :3]] image --, every weight gradient joins the bucket's
        grouped image launches; the actor's dgi image then fans out to the encoders."""
        ac = self.actor_critic
        idx, unpad_idx, T, R = bt["idx"], bt["unpad_idx"], bt["T"], bt["R"]
        obs, priv = flat["observations"], flat["privileged_observations"]
        imn = self.narrow_images
        _ffi.lib().dtc_set_concurrency_hint(int(bool(self.overlap_wgrad)))
        tw.begin(self.overlap_lanes and self.overlap_wgrad)
        tw.live_img.clear()
        sink = lambda *job: self._wgrad_img(tw, *job)
        hc = GruHead(tw, wset, fw.slots, "c", ac.memory_c, ac.Cr, bt["hid_c"], unpad_idx, T, R, sink)
        ha = GruHead(tw, wset, fw.slots, "a", ac.memory_a, ac.A, bt["hid_a"], unpad_idx, T, R, sink, dgi_image=True)

        def critic_input():
            return ac.packed_input(fw, "p_c", ac.critic_input(obs, flat["base_vel"], priv, idx, wide=True), idx, reuse=True), None

        def actor_input():
            ac.cenet_forward_(fw, flat["observation_histories"], eps, idx, masks=self.relu_masks, split=False, images=imn, wset=wset)
            ac.terrain_encoder_(fw, priv, idx, masks=self.relu_masks, images=True, wset=wset, lt_fp32=False)
            if imn:    # the actor's features as three images: l_t, the gathered observations (packed once), the latent kernel's [z | mu[:, :3]]
                return ([fw.img("lt"), ac.packed_input(fw, "p_obs", segmat([seg(obs, 0, ac.num_obs, gather=True, wide=True)], idx), idx, reuse=True),
                         fw.cur["p_zmu"]], [ac.num_obs + 19, 0, ac.num_obs])
            return ([fw.img("lt"), ac.packed_input(fw, "p_a", segmat([seg(obs, 0, ac.num_obs, gather=True, wide=True), seg(fw.z, 0, 16),
                                                                      seg(fw.mulv, 0, 3)], idx))], [ac.num_obs + 19, 0])

        def loss(mean, value):
            if self.after_forward_hook is not None:
                self.after_forward_hook(fw, "ppo")
            ops.ppo_loss(mean, ac.std_view, value, flat["actions"], flat["actions_log_prob"], flat["mu"], flat["sigma"],
                         flat["advantages"], flat["returns"], flat["values"], idx, cfg, tw.dmean, tw.dval, ac.std_grad,
                         stats[S_SURR:S_SURR + 4], self.optimizer.lr_dev, tw.loss_ws)
            self._kl_to_header(stats)
            return tw.dmean, tw.dval

        forward_backward(tw, hc, ha, critic_input, actor_input, loss, self.gru_multi)
        tw.held.append((hc, ha))
        # the actor features' gradient fans out to z, mu[:, :3] (fp32) and l_t (image); the observations need none
        tw.dmulv.zero_()
        h2i.linear_dgrad(ha.dgii, ac.proj_a.W, segmat([seg(None, 0, 512), seg(tw.dz, 0, 16), seg(tw.dmulv, 0, 3)]), tw.img("dlt", 512),
                         window=[(ac.num_obs + 19, 512), (ac.num_obs, 19)], wset=wset)
        tw.live_img |= {"dlt"}
        early = self._exchange_bucket(tw, "main_only")
        tw.order("main", "aux")                                    # dz, d mu[:, :3] are written
        self._terrain_encoder_backward(fw, tw, flat, idx, wset)
        with tw.lane("aux"):
            ops.cenet_latent_bwd(tw.dmulv, tw.dz, eps, fw.mulv, fw.mask, fw.info, fw.lat_ws)
            self._cenet_encoder_backward(fw, tw, flat, idx, split=False, wset=wset if imn else None)
        if early:
            self._exchange_bucket(tw, "shared")
        self._join(tw)
        return early

    def step_minibatch(self, bt, eps1, eps2, which="both", stats=None):
        """One recurrent mini-batch `bt` (an item of `recurrent_slices`): VAE step, policy step, or both."""
        self._require_gpu()
        st, ac = self.storage, self.actor_critic
        self._arena()
        dev = ac.std.device
        B = bt["idx"].numel()
        flat = {k: st.flat(k) for k in self._FLAT_NAMES}
        fw, tw = ac._fwd_ws(B), self._train_ws(B)
        own_gen = fw.slots.gen is None                # outside update(): the packed rollout rows serve this call only
        if own_gen:      # (inside update(): once per update -- the knobs and the storage do not change between mini-batches)
            tw.schedule = self._resolve_schedule(fw, flat)
            self._amax_static(flat, images=tw.schedule.images and self._memory_images())
        with fw.slots.open() if own_gen else contextlib.nullcontext():
            if own_gen:
                # (inside update() the device-side learning rate carries the adaptive schedule from mini-batch to mini-batch, ppo.py:301-307:
                # re-seeding it here from the host copy made every mini-batch adapt from the rate the update STARTED with -- found by
                # test_two_consecutive_updates_vs_oracle, round 6)
                self.optimizer.set_lr(self.learning_rate)
            stats = torch.zeros(STAT_COLS, dtype=torch.float32, device=dev) if stats is None else stats
            if which in ("vae", "both"):
                self._vae_step(fw, tw, flat, bt["idx"], eps1.to(dev).contiguous(), stats)
            if which in ("ppo", "both"):
                self._ppo_step_recurrent(fw, tw, flat, bt, eps2.to(dev).contiguous(), stats, self._loss_cfg())
            if own_gen:
                ops.amax_static_clear()
        return stats

    def update(self, eps1=None, eps2=None, return_stats=False):
        self._require_gpu()
        _share_rule()
        st, ac = self.storage, self.actor_critic
        if self.contain_nonfinite_envs:
            require_env_record(self)
        self._arena()
        dev = ac.std.device
        nmb, epochs = self.num_mini_batches, self.num_learning_epochs
        B = (st.num_envs // nmb) * st.num_transitions_per_env
        steps = nmb * epochs
        if eps1 is None or eps2 is None:
            seed = ops.draw_seed()
            eps1 = ops.randn((steps, B, 16), dev, seed + 1) if eps1 is None else eps1
            eps2 = ops.randn((steps, B, 16), dev, seed + 2) if eps2 is None else eps2
        stats = torch.zeros(steps, STAT_COLS, dtype=torch.float32, device=dev)
        tw = self._train_ws(B)
        tw.pad.zero("gi_")                            # padded input projections: the padding slots start every update from zero
        slices = list(self.recurrent_slices())
        k = 0
        fw = ac._fwd_ws(B)
        self.optimizer.set_lr(self.learning_rate)      # once per update: the schedule then lives on the device (lr_dev)
        # amax records of the stored rollout tensors ONCE per update (they were recomputed by every mini-batch: 100 passes over up to
        # 546 MB = 6.5 ms of a 133 ms step)
        flat = {k: st.flat(k) for k in self._FLAT_NAMES}
        tw.schedule = self._resolve_schedule(fw, flat)
        self._amax_static(flat, images=tw.schedule.images and self._memory_images())
        with fw.slots.open():                    # the slices are the same in every epoch: their packed rollout rows serve all five
            try:
                for _ in range(epochs):
                    for i, bt in enumerate(slices):
                        fw.slots.slot = i
                        self.step_minibatch(bt, eps1[k], eps2[k], "both", stats[k])
                        k += 1
            finally:
                ops.amax_static_clear()          # the storage is about to be refilled: its amax slots are void
        host, out = self._read_back(stats)
        ops.gru_seq_check()                      # (the persistent recurrence launches of this update all ran to their end)
        if self.contain_nonfinite_act:
            read_act_record(self)
        if self.contain_nonfinite_envs:
            read_env_record(self)
        st.clear()
        return (out, host) if return_stats else out
