"""PPO for the recurrent (GRU / LSTM) actor-critic -- BASELINE.json config 3 ("ActorCriticRecurrent (GRU hidden
512) BPTT over 24 steps").

The reference's `PPO` cannot drive `ActorCriticRecurrent` at this commit (it needs `.vae`, ppo.py:79, and its
update unpacks 16 items where the recurrent generator yields 11 -- SURVEY.md F2), so this class is the upstream
rsl_rl PPO step the code base was forked from: ppo.py:288-335 (log-prob / entropy / KL-adaptive learning rate /
clipped surrogate + clipped value loss / clip_grad_norm_ / Adam) fed by `reccurent_mini_batch_generator`
(rollout_storage.py:217-267), with hidden states recorded BEFORE each rollout step (the convention of the
commented lines ppo.py:138-139).  Same constructor keywords and method names as `PPO`.

Kernel schedule per mini-batch (N/4 envs x all 24 steps): input projection GEMM -> dtc_gru_fwd -> MLP with the
un-padding folded in as a row gather -> fused PPO loss -> MLP backward -> row scatter -> dtc_gru_bwd (BPTT) ->
input-projection weight gradient -> one fused clip+Adam over the flat parameter arena.
"""
from __future__ import annotations

import torch

from .. import _ffi, distributed as dp, h2i, ops
from .._ffi import seg, segmat
from ..modules.actor_critic_recurrent import ActorCriticRecurrent
from ..storage import RolloutStorage
from ..utils import UpdateSlots, true_indices
import os

from .ppo import (FusedAdam, S_ENTROPY, S_GNORM, S_KL, S_SURR, S_VALUE, STAT_COLS, _StepWorkspace, contain_act, init_act_containment,
                  read_act_record, read_env_record, require_contained_update, require_env_record)
from .recurrent_heads import GruHead, forward_backward


def _share_rule():
    """Several ranks of a job on ONE device (the gloo rehearsals of the data-parallel path): more than two persistent recurrence launches
    could be in flight on the device at once, and their workgroups must all be resident to meet (csrc/gru_seq.hip) -- per-step launches
    there.  One process per GPU (RCCL) keeps the persistent launches."""
    if dp.world_size() > 1 and dp.backend() != "nccl":
        ops.gru_seq_allow(False)


class RecurrentPPO:
    actor_critic: ActorCriticRecurrent

    def __init__(self, actor_critic, num_learning_epochs=5, num_mini_batches=4, clip_param=0.2, gamma=0.99, lam=0.95,
                 value_loss_coef=1.0, entropy_coef=0.01, learning_rate=5.e-4, max_grad_norm=1.0,
                 use_clipped_value_loss=True, schedule="adaptive", desired_kl=0.01, device='cpu', *, contain_nonfinite_envs=False,
                 contain_nonfinite_act=False):
        self.device = device
        # PPO's keyword of the same name: envs that hold anything non-finite are overwritten in the storage by valid ones before update()
        self.contain_nonfinite_envs = bool(contain_nonfinite_envs)
        self.last_nonfinite_envs = 0
        # ... and PPO's: an env whose rollout step read or produced anything non-finite leaves act() with zero actions and a cleared state
        self.contain_nonfinite_act = bool(contain_nonfinite_act)
        self.last_nonfinite_act = 0
        require_contained_update(self)
        self.desired_kl, self.schedule, self.learning_rate = desired_kl, schedule, learning_rate
        self.actor_critic = actor_critic
        self.actor_critic.to(self.device)
        self.storage = None
        self.optimizer = None
        if torch.device(device).type == "cuda":
            arena = actor_critic.ensure_arena()
            self.optimizer = FusedAdam(arena, arena.main_range, actor_critic.parameters(), lr=learning_rate)
            from .. import distributed as dp
            dp.broadcast_parameters_(arena.flat)             # data parallel: all ranks start from rank 0's weights
        self.transition = RolloutStorage.Transition()
        self.clip_param, self.num_learning_epochs, self.num_mini_batches = clip_param, num_learning_epochs, num_mini_batches
        self.value_loss_coef, self.entropy_coef = value_loss_coef, entropy_coef
        self.gamma, self.lam, self.max_grad_norm = gamma, lam, max_grad_norm
        self.use_clipped_value_loss = use_clipped_value_loss
        self.capture_grads, self.captured = False, {}
        self.last_update_stats = None
        # actor and critic are independent recurrences until the loss and again until the optimiser step: the critic
        # runs on a second stream, every weight gradient on a third (DTC_OVERLAP_LANES=0 / DTC_OVERLAP_WGRAD=0: serial)
        self.overlap = os.environ.get("DTC_OVERLAP_LANES", "1") != "0" and os.environ.get("DTC_OVERLAP_WGRAD", "1") != "0"
        # DTC_GRU_MULTI=1: memory_a and memory_c advance together, one launch per time step (dtc_gru_fwd_multi / dtc_gru_bwd_multi;
        # bit-identical, measured slower: 100.7 vs 92.7 ms per step); default: one chain of launches each, on its lane
        self.gru_multi = os.environ.get("DTC_GRU_MULTI", "0") == "1"
        self._tws = {}                     # (M, device) -> the step workspace (lanes, buffers, images)
        self._slots = UpdateSlots()        # opened by update(): what is packed / zeroed once per update and mini-batch slot
        self._wimages = None
        # every GEMM outside the GRU time steps on block-scaled fp16 operand images (dtc_amd/h2i.py; DTC_H2I=0: round 4's converting
        # kernels): the input projection reads the padded observations' valid rows as an image packed once per update and mini-batch,
        # the MLP activations / gradients live as images, and the weight gradients of a recurrence -- W_ih, W_hh and the MLP layers --
        # are ONE grouped image-operand launch on the weight-gradient stream
        self.use_images = os.environ.get("DTC_H2I", "1") != "0"
        self._wset = None                  # h2i.WeightSet: the step's weight images, rebuilt by one launch per optimisation step

    def _require_gpu(self):
        if self.optimizer is None:
            raise _ffi.DtcError("dtc_amd.RecurrentPPO computes on an MI355X only (device='cuda:N')")

    def init_storage(self, num_envs, num_transitions_per_env, actor_obs_shape, critic_obs_shape, action_shape):
        self.storage = RolloutStorage(num_envs, num_transitions_per_env, actor_obs_shape, critic_obs_shape, [1],
                                      action_shape, self.device)
        if self.contain_nonfinite_envs:
            self.storage.contain_nonfinite_envs = True
        if self.contain_nonfinite_act:
            init_act_containment(self)

    def test_mode(self):
        self.actor_critic.eval()

    def train_mode(self):
        self.actor_critic.train()

    # ---------------------------------------------------------------- rollout side
    def act(self, obs, critic_obs):
        self._require_gpu()
        ac, tr = self.actor_critic, self.transition
        N = obs.shape[0]
        for m in (ac.memory_a, ac.memory_c):
            if m.hidden_states is None:
                m.hidden_states = m.init_hidden(N, obs.device)
        tr.hidden_states = tuple(m.clone_hidden(h) for m, h in zip((ac.memory_a, ac.memory_c), ac.get_hidden_states()))   # BEFORE this step
        if self.contain_nonfinite_act:
            with ops.rows_to_themselves():         # (one env's non-finite element must not reach the others' rows: there would be none to keep)
                tr.actions, tr.values = ac.act(obs).detach(), ac.evaluate(critic_obs).detach()
        else:
            tr.actions = ac.act(obs).detach()
            tr.values = ac.evaluate(critic_obs).detach()
        tr.actions_log_prob = ac.get_actions_log_prob(tr.actions).detach()
        tr.action_mean, tr.action_sigma = ac.action_mean.detach(), ac.action_std.detach()
        if self.contain_nonfinite_act:
            contain_act(self, (obs, critic_obs))
        tr.observations, tr.critic_observations, tr.privileged_observations = obs, critic_obs, critic_obs
        tr.observation_histories = torch.zeros(N, 1, device=obs.device)
        tr.base_vel = torch.zeros(N, 3, device=obs.device)
        return tr.actions

    def process_env_step(self, rewards, dones, infos, next_obs=None):
        tr = self.transition
        tr.rewards, tr.dones = rewards.clone(), dones
        tr.next_observations = next_obs if next_obs is not None else tr.observations
        if 'time_outs' in infos:
            tr.rewards += self.gamma * torch.squeeze(tr.values * infos['time_outs'].unsqueeze(1).to(self.device), 1)
        self.storage.add_transitions(tr)
        tr.clear()
        self.actor_critic.reset(dones)

    def compute_returns(self, last_critic_obs):
        self._require_gpu()
        ac = self.actor_critic
        keep = ac.memory_c.clone_hidden(ac.memory_c.hidden_states)
        if self.contain_nonfinite_act:             # (as in act(): a non-finite last observation costs its own env the bootstrap value, no other)
            with ops.rows_to_themselves():
                last_values = ac.evaluate(last_critic_obs).detach()
        else:
            last_values = ac.evaluate(last_critic_obs).detach()
        ac.memory_c.hidden_states = keep            # the bootstrap value must not advance the critic's state
        self.storage.compute_returns(last_values, self.gamma, self.lam)

    # ---------------------------------------------------------------- update
    def _loss_cfg(self):
        cfg = _ffi.DtcPpoCfg()
        cfg.clip_param, cfg.value_loss_coef, cfg.entropy_coef = self.clip_param, self.value_loss_coef, self.entropy_coef
        cfg.desired_kl = float(self.desired_kl) if self.desired_kl is not None else 0.0
        cfg.use_clipped_value_loss = int(bool(self.use_clipped_value_loss))
        adaptive = self.desired_kl is not None and self.schedule == 'adaptive'
        cfg.adaptive_schedule = int(adaptive and not dp.data_parallel())
        # data parallel: the finalize launch also deposits the KL mean in slot 0 of the gradient header (averaged by the exchange)
        cfg.kl_mirror = self.actor_critic.ensure_arena().kl_slot.data_ptr() if (adaptive and dp.data_parallel()) else None
        return cfg

    def _train_ws(self, M, dev):
        ws = self._tws.get((M, dev))
        if ws is None:
            ws = self._tws[(M, dev)] = _StepWorkspace(M, dev)
        return ws

    def _ppo_loss(self, mean, value, store_idx, stats, M, dev):
        """The fused PPO loss (rows of the rollout tensors addressed through store_idx: no slicing copies) -> (dmean, dval, workspace).
        (Data parallel: the KL mean travels in the header of the gradient exchange -- deposited by the loss's finalize launch, _loss_cfg.)"""
        ac, flat = self.actor_critic, self.storage.flat
        dmean, dval = torch.empty_like(mean), torch.empty(M, 1, device=dev)
        lws = ops.workspace(_ffi.lib().dtc_loss_workspace(M), dev)
        ops.ppo_loss(mean, ac.std_view, value, flat("actions"), flat("actions_log_prob"), flat("mu"), flat("sigma"),
                     flat("advantages"), flat("returns"), flat("values"), store_idx, self._loss_cfg(), dmean, dval,
                     ac.std_grad, stats[S_SURR:S_SURR + 4], self.optimizer.lr_dev, lws)
        return dmean, dval, lws

    def _wgrad(self, tw, dZ, X, gW, gb, M, rows=None):
        """Weight gradient on the side stream (off the critical path until the optimiser step)."""
        ws = tw.wgrad_ws(gW.shape[0], gW.shape[1], M)
        if self.overlap:
            ev = tw.event()
            ev.record()
            tw.side.wait_event(ev)
            ops.linear_wgrad(dZ, X, gW, gb, ws, M=M, stream_ptr=tw.side.cuda_stream, rows=rows)
            tw.side_busy = True
        else:
            ops.linear_wgrad(dZ, X, gW, gb, ws, M=M, rows=rows)

    def _mlp_backward(self, tw, layers, outs, dOut, X0, M, dev, keep):
        """Backward through an MLP given the saved layer outputs; returns the gradient w.r.t. its input rows.
        Every gradient buffer goes into `keep`: the side stream still reads it for the weight gradient after this
        lane has moved on, so it must not return to the caching allocator before the join."""
        dZ = dOut
        for li in range(len(layers) - 1, -1, -1):
            L = layers[li]
            X = outs[li - 1] if li > 0 else X0
            self._wgrad(tw, dZ, X, L.gW, L.gb, M)
            dX = torch.empty(M, L.n_in, device=dev)
            keep.append(dX)
            if li > 0:
                ops.linear_dgrad(dZ, L.W, dX, outs[li - 1], layers[li - 1].act, M=M)
            else:
                ops.linear_dgrad(dZ, L.W, dX, None, None, M=M)
            dZ = dX
        return dZ

    def step_minibatch(self, batch, start, stop, stats=None):
        """One recurrent mini-batch: `batch` = 11-tuple of reccurent_mini_batch_generator, envs [start, stop)."""
        self._require_gpu()
        ac, st = self.actor_critic, self.storage
        arena = ac.ensure_arena()
        if self.optimizer.arena is not arena:            # the model moved: re-bind the optimiser's views
            arena._named = list(ac.named_parameters())
            self.optimizer.rebind(arena)
        (obs_b, cobs_b, _a, _v, _adv, _r, _lp, _mu, _sg, (hid_a, hid_c), masks) = batch
        dev = obs_b.device
        T, R = masks.shape
        N, Nmb = st.num_envs, stop - start
        M = T * Nmb
        tw = self._train_ws(M, dev)
        # un-padding as a row map: padded row (pos*R + traj) of each (t, env) in time-major order
        flat_rt = true_indices(masks.transpose(1, 0), M)          # every (env, t) has exactly one padded slot: no nonzero() sync
        traj, pos = flat_rt // T, flat_rt % T
        unpad_idx = (pos * R + traj).view(Nmb, T).transpose(1, 0).reshape(-1).contiguous()
        store_idx = (torch.arange(T, device=dev).unsqueeze(1) * N + torch.arange(start, stop, device=dev)).reshape(-1).contiguous()
        stats = torch.zeros(STAT_COLS, device=dev) if stats is None else stats
        if self._slots.gen is None:
            # outside update() only.  Inside it the device-side learning rate carries the adaptive schedule from mini-batch to mini-batch
            # (ppo.py:301-307): re-seeding it here from the host copy made every mini-batch adapt from the rate the update STARTED with
            # (found by test_two_consecutive_updates_vs_oracle, round 6)
            self.optimizer.set_lr(self.learning_rate)
        _ffi.lib().dtc_set_concurrency_hint(int(bool(self.overlap)))
        if self._wimages is None:
            self._wimages = ops.WeightImages()
        if self._image_mode(M):
            if self._wset is None:
                self._wset = h2i.WeightSet()
            self._wset.rebuild()                     # the optimiser wrote the weights since the images were built: one grouped launch
            self._forward_backward_images(tw, batch, stats, unpad_idx, store_idx, M, T, R, dev)
        else:
            with self._wimages:                      # weight images of the step's split-path layers: one launch
                self._forward_backward(tw, batch, stats, unpad_idx, store_idx, M, T, R, dev)
        arena = ac.arena
        dp_adaptive = dp.data_parallel() and self.desired_kl is not None and self.schedule == 'adaptive'
        if dp.data_parallel():
            self._exchange(tw, arena)
        if dp_adaptive:
            ops.lr_adapt(arena.kl_slot, self.optimizer.lr_dev, float(self.desired_kl), kl_out=stats[S_KL:S_KL + 1])
        if self.capture_grads:
            self.captured["main"] = ac.arena.grad.clone()
        self.optimizer.step(self.max_grad_norm, stats[S_GNORM:S_GNORM + 1])
        return stats

    def _exchange(self, tw, arena):
        """Data parallel: header (KL) + every gradient, one collective per optimiser step, after the join.  With the overlapped schedule
        it is issued on the weight-gradient stream, as the bucket exchanges of PPO._exchange_bucket are -- the library-owned lane of
        _lane_streams, not torch's current stream --, ordered behind the joined step and in front of the optimiser."""
        if not self.overlap:
            dp.allreduce_mean_(arena.grad_full)
            return
        main = torch.cuda.current_stream()
        ev = tw.event()
        ev.record(main)
        tw.side.wait_event(ev)
        with torch.cuda.stream(tw.side):
            dp.allreduce_mean_(arena.grad_full)
        tw.joined.record(tw.side)
        main.wait_event(tw.joined)
        tw._ev_next = 0

    def _forward_backward(self, tw, batch, stats, unpad_idx, store_idx, M, T, R, dev):
        ac = self.actor_critic
        (obs_b, cobs_b, _a, _v, _adv, _r, _lp, _mu, _sg, (hid_a, hid_c), masks) = batch
        tw.begin(self.overlap)
        # forward: critic recurrence on the second lane
        with tw.lane("aux"):
            ac.evaluate(cobs_b, masks, hid_c, unpad_idx)
            c_outs, c_saved = ac._critic_outs, ac.memory_c.saved
        ac.act(obs_b, masks, hid_a, unpad_idx)
        a_outs, a_saved = ac._actor_outs, ac.memory_a.saved
        tw.order("aux", "main")
        dmean, dval, lws = self._ppo_loss(a_outs[-1], c_outs[-1], store_idx, stats, M, dev)
        tw.order("main", "aux")
        # backward: MLPs -> scatter into the padded layout -> BPTT -> input-projection weight gradient
        H = ac.rnn_hidden_size
        keep = []                                   # buffers read by the side stream stay alive until the join

        def head_backward(layers, outs, saved, mem, dOut):
            hs_flat = saved["hs_all"][1:].reshape(T * R, H)
            X0 = segmat([seg(hs_flat, 0, H, gather=True)], unpad_idx)
            d_in = self._mlp_backward(tw, layers, outs, dOut, X0, M, dev, keep)
            dhs = torch.zeros(T * R, H, device=dev)
            ops.scatter_rows(d_in, unpad_idx, dhs)
            # unpad_idx doubles as the list of valid (t, r) slots: the recurrent weight gradients skip the padding
            dgi = mem.backward(saved, dhs.view(T, R, H), rows=unpad_idx,
                               wgrad=lambda dZ, X, gW, gb: self._wgrad(tw, dZ, X, gW, gb, T * R, rows=unpad_idx))
            keep.extend((d_in, dhs, dgi, X0, outs, saved))

        with tw.lane("aux"):
            head_backward(ac.Cr, c_outs, c_saved, ac.memory_c, dval)
        head_backward(ac.A, a_outs, a_saved, ac.memory_a, dmean)
        tw.join()

    # ---------------------------------------------------------------- the same step on operand images
    def _image_mode(self, M):
        ac = self.actor_critic
        return (self.use_images and ops.SPLIT and M % 128 == 0 and ac.memory_a.kind == 'gru' and ac.memory_c.kind == 'gru'
                and ac.memory_a.num_layers == 1 and ac.memory_c.num_layers == 1 and ac.rnn_hidden_size % 128 == 0)

    def _packed_obs(self, name, x, unpad_idx, M, dev):
        """Image of the valid rows of the padded observations x [T, R, I].  Inside an update the generator yields the SAME
        trajectories for mini-batch i in every epoch (rollout_storage.py:217-267: no shuffling), so each mini-batch's image is packed
        once per update into its own buffer; outside an update every call packs."""
        def rows():
            x2 = x.float().contiguous().view(-1, x.shape[-1])     # (the generator's slice of the padded trajectories: copied only here)
            return segmat([seg(x2, 0, x2.shape[1], gather=True, wide=True)], unpad_idx)     # (a pack's source: may span 2 GiB and more)
        return self._slots.packed(self._train_ws(M, dev), name, rows, x.shape[-1], M)

    def _wgrad_group(self, tw, jobs):
        """A head's weight gradients -- MLP layers, W_hh, W_ih -- as ONE grouped launch on the weight-gradient stream, behind everything
        its lane has issued."""
        ws = tw.group_ws_img(jobs)
        if self.overlap:
            ev = tw.event()
            ev.record()
            tw.side.wait_event(ev)
            h2i.wgrad_group(jobs, tw.B, ws, stream_ptr=tw.side.cuda_stream)
            tw.side_busy = True
        else:
            h2i.wgrad_group(jobs, tw.B, ws)

    def _forward_backward_images(self, tw, batch, stats, unpad_idx, store_idx, M, T, R, dev):
        ac = self.actor_critic
        (obs_b, cobs_b, _a, _v, _adv, _r, _lp, _mu, _sg, (hid_a, hid_c), masks) = batch
        tw.begin(self.overlap)
        jobs = dict(c=[], a=[])

        def head(name, mem, layers, hid):
            return GruHead(tw, self._wset, self._slots, name, mem, layers, mem._split(hid)[0][0], unpad_idx, T, R,
                           lambda *job: jobs[name].append(job))
        hc, ha = head("c", ac.memory_c, ac.Cr, hid_c), head("a", ac.memory_a, ac.A, hid_a)

        def loss(mean, value):
            ac._dist = (mean, ac.std_view.detach().expand_as(mean))
            ac._actor_outs, ac._critic_outs = ha.outs, hc.outs
            ac.memory_a.saved = dict(hs_all=ha.hs_all, out=ha.hs_all[1:])
            ac.memory_c.saved = dict(hs_all=hc.hs_all, out=hc.hs_all[1:])
            dmean, dval, lws = self._ppo_loss(mean, value, store_idx, stats, M, dev)
            self._held = (ha, hc, jobs, dmean, dval, lws)       # (until the next step: nothing here returns to the allocator early)
            return dmean, dval

        forward_backward(tw, hc, ha, lambda: (self._packed_obs("x_c", cobs_b, unpad_idx, M, dev), None),
                         lambda: (self._packed_obs("x_a", obs_b, unpad_idx, M, dev), None), loss, self.gru_multi,
                         done=lambda h: self._wgrad_group(tw, jobs[h.name]))
        tw.join()

    def update(self):
        self._require_gpu()
        _share_rule()
        st = self.storage
        if self.contain_nonfinite_envs:
            require_env_record(self)
        nmb, epochs = self.num_mini_batches, self.num_learning_epochs
        mb = st.num_envs // nmb
        dev = self.actor_critic.std.device
        stats = torch.zeros(nmb * epochs, STAT_COLS, device=dev)
        k = 0
        # the padded input projections start every update from zero (the image path's here, the converting path's in Memory)
        self._train_ws(st.num_transitions_per_env * mb, dev).pad.zero("gi_")
        for mem in (self.actor_critic.memory_a, self.actor_critic.memory_c):
            mem.new_update()
        self.optimizer.set_lr(self.learning_rate)      # once per update: the schedule then lives on the device (lr_dev)
        with self._slots.open():                       # the observation images of this update: packed once per mini-batch slot
            for batch in st.reccurent_mini_batch_generator(nmb, epochs):
                i = k % nmb
                self._slots.slot = i
                self.step_minibatch(batch, i * mb, (i + 1) * mb, stats[k])
                k += 1
        host = stats.cpu()
        ops.gru_seq_check()                      # (the persistent recurrence launches of this update all ran to their end)
        self.learning_rate = float(self.optimizer.lr_dev.item())
        self.last_update_stats = host
        m = host.double().mean(dim=0)
        if self.contain_nonfinite_act:
            read_act_record(self)
        if self.contain_nonfinite_envs:
            read_env_record(self)
        st.clear()
        return float(m[S_VALUE]), float(m[S_SURR])
