"""contain_nonfinite_act=True on all three trainers: an env whose rollout step read or produced anything non-finite leaves act() with zero
actions and a cleared live recurrent state, is named in alg.nonfinite_act_envs for the env side and in storage.act_valid for the update.

Every case: 16 envs x 24 steps driven through act() / process_env_step() / compute_returns() / update() on the synthetic rollout of
dtc_amd.synthetic (observations, rewards and dones of S.rollout, fed step by step), 4 mini-batches, 2 epochs.  All comparisons are bit
for bit.  The clean run of a model WITHOUT the new flag is computed once and shared."""
import datetime
import functools
import os

import pytest
import torch

from dtc_amd import synthetic as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T, N, NMB, EPOCHS = 24, 16, 4, 2
# PPO with the decoder under either containment of the update, RecurrentPPO with a 1-layer GRU (H = 128) and a 2-layer LSTM (H = 50),
# RecurrentDecoderPPO
KINDS = ("ppo", "ppo_rows", "rppo_gru", "rppo_lstm2", "rdppo")
RECURRENT = ("rppo_gru", "rppo_lstm2", "rdppo")
STORED = ("observations", "next_observations", "privileged_observations", "observation_histories", "actions", "rewards", "values",
          "actions_log_prob", "mu", "sigma", "base_vel", "dones")
NAN_OBS = dict(step=5, env=3)
INF_STATE = dict(step=9, env=7)


def _make(kind, act_flag):
    """A trainer of `kind`, from the same weights every time, with the containment of the update the kind names."""
    from dtc_amd.algorithms import PPO, RecurrentDecoderPPO, RecurrentPPO
    from dtc_amd.modules import ActorCriticDecoder, ActorCriticDecoderRecurrent, ActorCriticRecurrent
    # (mini-batches of 96 rows: the row containment runs on the operand-image schedule, which takes them with ragged_images)
    contain = dict(contain_nonfinite=True, ragged_images=True) if kind == "ppo_rows" else dict(contain_nonfinite_envs=True)
    common = dict(learning_rate=1e-3, entropy_coef=0.003, device=DEV, num_learning_epochs=EPOCHS, num_mini_batches=NMB,
                  contain_nonfinite_act=act_flag, **contain)
    torch.manual_seed(3)
    if kind in ("ppo", "ppo_rows"):
        alg = PPO(ActorCriticDecoder(53, 1389, 12), **common)
    elif kind == "rdppo":
        alg = RecurrentDecoderPPO(ActorCriticDecoderRecurrent(53, 1389, 12), **common)
    else:
        rnn = dict(rnn_type="gru", rnn_hidden_size=128, rnn_num_layers=1) if kind == "rppo_gru" else \
            dict(rnn_type="lstm", rnn_hidden_size=50, rnn_num_layers=2)
        ac = ActorCriticRecurrent(53, 1389, 12, actor_hidden_dims=[512, 256, 128], critic_hidden_dims=[512, 256, 128], activation='elu', **rnn)
        alg = RecurrentPPO(ac, **common)
    if kind.startswith("rppo"):
        alg.init_storage(N, T, [53], [1389], [12])
    else:
        alg.init_storage(N, T, [53], [1389], [265], [12])
    return alg


@functools.lru_cache(maxsize=None)
def _data():
    d = {k: v.to(DEV) for k, v in S.rollout(N, T, seed=4).items()}
    d["dones"][:, 0] = 0                                                   # one env without a reset: a full-length trajectory
    d["dones"][8:11, INF_STATE["env"]] = 0                                 # ... and no reset of env 7 around the steps case 3 looks at
    return d


def _states(h):
    return list(h) if isinstance(h, (tuple, list)) else [h]


def _live_states(alg):
    ac = alg.actor_critic
    return [s for h in ac.get_hidden_states() for s in _states(h)] if hasattr(ac, "memory_a") else []


def _storage_tensors(st):
    out = {k: getattr(st, k) for k in STORED}
    for name, net in (("hidden_a", st.saved_hidden_states_a), ("hidden_c", st.saved_hidden_states_c)):
        for i, s in enumerate(net or []):
            out[f"{name}{i}"] = s
    return out


def _state(alg):
    out = dict(flat=alg.actor_critic.arena.flat.clone(), lr=alg.learning_rate, stats=alg.last_update_stats.clone())
    for i, opt in enumerate([alg.optimizer] + ([alg.vae_optimizer] if hasattr(alg, "vae_optimizer") else [])):
        out[f"m{i}"], out[f"v{i}"], out[f"lr_dev{i}"] = opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.lr_dev.clone()
    return {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in out.items()}


def _bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _first_difference(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if not (_bits_equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k]):
            return k
    return None


def _update(kind, alg):
    perm, e1, e2 = (t.to(DEV) for t in S.update_noise(N, T, NMB, EPOCHS, seed=123))
    torch.manual_seed(99)                                                  # (whatever an update draws itself: the same in every run)
    if kind in ("ppo", "ppo_rows"):
        return alg.update(perm=perm, eps1=e1, eps2=e2)
    if kind.startswith("rppo"):
        return alg.update()
    return alg.update(eps1=e1, eps2=e2)


def _compute_returns(kind, alg, d, nan_last=None):
    """the trainer's own compute_returns on the last observations -> the bootstrap values it handed to the storage.  `nan_last`: an env
    whose last (critic) observation holds a NaN"""
    st, seen = alg.storage, {}
    inner = st.compute_returns

    def spy(last_values, gamma, lam):
        seen["last_values"] = last_values.clone()
        return inner(last_values, gamma, lam)
    st.compute_returns = spy
    try:
        obs, priv, vel = d["next_observations"][T - 1], d["privileged_observations"][T - 1], d["base_vel"][T - 1]
        if nan_last is not None:
            priv = priv.clone()
            priv[nan_last, 700] = float("nan")                            # (a column every critic reads: the composite's takes 693 and up)
        alg.compute_returns(priv) if kind.startswith("rppo") else alg.compute_returns(obs, priv, vel)
    finally:
        del st.compute_returns
    return seen["last_values"]


def _rollout(kind, alg, nan_obs=False, inf_state=False, graph=False):
    """T steps through act() and process_env_step() -> what the tests look at.  Returns are not computed yet.  `graph`: the policy step
    replayed from a captured graph (PPO.graph_rollout)."""
    d = _data()
    flag = alg.contain_nonfinite_act
    alg.graph_rollout = graph
    torch.manual_seed(11)                                                  # the policy's exploration noise: the same in every run
    out = dict(actions=[], masks=[], mask_ids=set(), live={})
    for t in range(T):
        obs, priv, hist, vel = (d[k][t].clone() for k in ("observations", "privileged_observations", "observation_histories", "base_vel"))
        if nan_obs and t == NAN_OBS["step"]:
            obs[NAN_OBS["env"], 7] = float("nan")
        if inf_state and t == INF_STATE["step"]:
            _states(alg.actor_critic.memory_a.hidden_states)[0][-1, INF_STATE["env"], :] = float("inf")
        actions = alg.act(obs, priv) if kind.startswith("rppo") else alg.act(obs, priv, hist, vel)
        out["actions"].append(actions.clone())
        if flag:
            out["masks"].append(alg.nonfinite_act_envs.clone())
            out["mask_ids"].add(id(alg.nonfinite_act_envs))
        if t in (INF_STATE["step"], INF_STATE["step"] + 1):
            out["live"][t] = [s.clone() for s in _live_states(alg)]
        alg.process_env_step(rewards=d["rewards"][t, :, 0].clone(), dones=d["dones"][t, :, 0].clone(), next_obs=d["next_observations"][t],
                             infos={})
    out["actions"] = torch.stack(out["actions"])
    out["masks"] = torch.stack(out["masks"]).cpu() if flag else None
    out["storage"] = {k: v.clone() for k, v in _storage_tensors(alg.storage).items()}
    out["act_valid"] = alg.storage.act_valid.cpu().clone() if flag else None
    return out


@functools.lru_cache(maxsize=None)
def _clean_reference(kind):
    """the clean rollout and update of a trainer WITHOUT the new flag: computed once per model, never written afterwards"""
    from dtc_amd import ops
    alg = _make(kind, False)
    assert alg.storage.act_valid is None and not hasattr(alg, "nonfinite_act_envs")
    keep = ops.act_contain

    def never(*a, **k):
        raise AssertionError("ops.act_contain was reached with the flag off")
    ops.act_contain = never                                                # the whole flag-off run: act(), compute_returns(), update()
    try:
        run = _rollout(kind, alg)
        _compute_returns(kind, alg, _data())
        _update(kind, alg)
    finally:
        ops.act_contain = keep
    assert alg.last_nonfinite_act == 0 and alg.storage.act_valid is None
    run["state"] = _state(alg)
    assert bool(torch.isfinite(run["state"]["flat"]).all())
    return run


def _invalid_units(kind, st):
    """what the storage's record keeps out of the update -> sorted [(step, env)] (row containment) or [env] (env containment)"""
    if kind == "ppo_rows":
        rows = torch.nonzero(st.row_valid == 0).flatten().cpu().tolist()
        return [(r // N, r % N) for r in rows]
    return torch.nonzero(st.env_valid == 0).flatten().cpu().tolist()


# ------------------------------------------------------------------------------------------------ 1. clean rollout
@pytest.mark.parametrize("kind", KINDS)
def test_clean_rollout_gives_the_bits_of_the_run_without_the_flag(kind):
    """On the recurrent models this rests on the rollout step keeping its arithmetic under the flag: the two-term fp16 kernels still run,
    only the exponent of an operand is taken from its finite elements (ops.rows_to_themselves), which on a clean rollout are all of
    them."""
    ref = _clean_reference(kind)
    alg = _make(kind, True)
    run = _rollout(kind, alg)
    assert _bits_equal(run["actions"], ref["actions"])
    assert run["storage"].keys() == ref["storage"].keys() and len(run["storage"]) >= len(STORED) + (2 if kind in RECURRENT else 0)
    for k in ref["storage"]:
        assert _bits_equal(run["storage"][k], ref["storage"][k]), k
    assert not bool(run["masks"].any()) and bool((run["act_valid"] == 1).all()) and len(run["mask_ids"]) == 1
    _compute_returns(kind, alg, _data())
    assert _invalid_units(kind, alg.storage) == []
    _update(kind, alg)
    assert alg.last_nonfinite_act == 0 and isinstance(alg.last_nonfinite_act, int)
    assert _first_difference(_state(alg), ref["state"]) is None
    assert bool((alg.storage.act_valid == 1).all())


# ------------------------------------------------------------------------------------------------ 2. a NaN observation
@pytest.mark.parametrize("kind", KINDS)
def test_nan_observation_of_one_env_at_one_step(kind):
    ref = _clean_reference(kind)
    s, e = NAN_OBS["step"], NAN_OBS["env"]
    others = [n for n in range(N) if n != e]
    alg = _make(kind, True)
    run = _rollout(kind, alg, nan_obs=True)
    # zeros (+0.0, every bit) for env 3 at that step; the other 15 envs act as in the clean run, at every step
    assert not bool(run["actions"][s, e].view(torch.int32).any())
    assert _bits_equal(run["actions"][:, others], ref["actions"][:, others])
    assert bool(torch.isfinite(run["actions"]).all())
    if kind not in RECURRENT:                                              # (no memory: env 3 itself is back on the clean run's actions)
        rest = [t for t in range(T) if t != s]
        assert _bits_equal(run["actions"][rest], ref["actions"][rest])
    want = torch.zeros(T, N, dtype=torch.uint8)
    want[s, e] = 1
    assert torch.equal(run["masks"], want) and len(run["mask_ids"]) == 1    # 1 at (5, 3) only: 0 again at step 6; one tensor throughout
    assert torch.equal(run["act_valid"], 1 - want)
    assert not bool(run["storage"]["actions"][s, e].view(torch.int32).any())          # the transition stored the repaired actions
    for state in _live_states(alg):
        assert bool(torch.isfinite(state).all())
    last_values = _compute_returns(kind, alg, _data())
    st = alg.storage
    invalid = _invalid_units(kind, st)
    if kind == "ppo_rows":
        # row (5, 3) -- and, as the row containment has it, the earlier rows of env 3's trajectory, whose returns the value of (5, 3) enters
        assert (s, e) in invalid and all(n == e and t <= s for t, n in invalid)
    else:
        assert invalid == [e]
    _update(kind, alg)
    assert alg.last_nonfinite_act == 1
    assert (alg.last_nonfinite_rows if kind == "ppo_rows" else alg.last_nonfinite_envs) == len(invalid)
    got = _state(alg)
    assert bool(torch.isfinite(got["flat"]).all()) and bool(torch.isfinite(got["stats"]).all())
    assert bool((st.act_valid == 1).all())                                 # update() cleared the storage
    # the containment of the update as it was, on a storage that holds the same bytes: the same weights -- the new record only adds (5, 3)
    plain = _make(kind, False)
    for k, v in run["storage"].items():
        if k.startswith("hidden"):
            continue
        getattr(plain.storage, k).copy_(v)
    if kind in RECURRENT:
        plain.storage.saved_hidden_states_a = [v.clone() for k, v in sorted(run["storage"].items()) if k.startswith("hidden_a")]
        plain.storage.saved_hidden_states_c = [v.clone() for k, v in sorted(run["storage"].items()) if k.startswith("hidden_c")]
    plain.storage.step = T
    plain.storage.compute_returns(last_values, plain.gamma, plain.lam)
    assert _invalid_units(kind, plain.storage) == invalid
    _update(kind, plain)
    assert _first_difference(got, _state(plain)) is None


# ------------------------------------------------------------------------------------------------ 3. a diverged live state
@pytest.mark.parametrize("kind", RECURRENT)
def test_infinite_live_state_is_cleared_and_the_env_acts_again(kind):
    ref = _clean_reference(kind)
    s, e = INF_STATE["step"], INF_STATE["env"]
    others = [n for n in range(N) if n != e]
    alg = _make(kind, True)
    run = _rollout(kind, alg, inf_state=True)
    want = torch.zeros(T, N, dtype=torch.uint8)
    want[s, e] = 1
    assert torch.equal(run["masks"], want) and torch.equal(run["act_valid"], 1 - want)
    # every layer of both memories: zero at env 7 behind act(), the other envs' states as in the clean run
    assert len(run["live"][s]) == (4 if kind == "rppo_lstm2" else 2)
    for state, clean in zip(run["live"][s], ref["live"][s]):
        assert state.shape[0] == (2 if kind == "rppo_lstm2" else 1)
        assert not bool(state[:, e].view(torch.int32).any())
        assert _bits_equal(state[:, others], clean[:, others]) and bool(clean[:, e].any())
    assert not bool(run["actions"][s, e].view(torch.int32).any())
    assert bool(torch.isfinite(run["actions"]).all()) and bool(run["actions"][s + 1, e].any())      # step 10: finite, and acting again
    for state in run["live"][s + 1]:
        assert bool(torch.isfinite(state).all())
    assert _bits_equal(run["actions"][:, others], ref["actions"][:, others])
    _compute_returns(kind, alg, _data())
    assert _invalid_units(kind, alg.storage) == [e]
    _update(kind, alg)
    assert alg.last_nonfinite_act == 1 and alg.last_nonfinite_envs == 1
    got = _state(alg)
    assert bool(torch.isfinite(got["flat"]).all()) and bool(torch.isfinite(got["stats"]).all())


def test_a_repaired_step_with_clean_stored_bytes_still_leaves_the_update():
    """the case the record exists for: the stored bytes of a repaired (step, env) look clean, the update must not see it all the same"""
    kind = "rppo_gru"
    alg = _make(kind, True)
    _rollout(kind, alg)
    st = alg.storage
    st.act_valid[11, 2] = 0                                                # as dtc_act_contain would have left it
    for k, v in _storage_tensors(st).items():
        assert bool(torch.isfinite(v.float()).all()), k
    _compute_returns(kind, alg, _data())
    assert _invalid_units(kind, st) == [2]
    _update(kind, alg)
    assert alg.last_nonfinite_act == 1 and alg.last_nonfinite_envs == 1


@pytest.mark.parametrize("kind", RECURRENT)
def test_nan_in_the_last_observation_costs_its_own_env_the_bootstrap_value_and_no_other(kind):
    """compute_returns of the recurrent trainers evaluates the critic on the last observations with the same kernels as act(): under the
    flag it runs under the same switch, so env 2's NaN stays env 2's"""
    ref = _clean_reference(kind)
    alg = _make(kind, True)
    _rollout(kind, alg)
    before = [s.clone() for s in _live_states(alg)]
    last_values = _compute_returns(kind, alg, _data(), nan_last=2)
    finite = torch.isfinite(last_values.reshape(-1)).cpu()
    assert not bool(finite[2]) and int(finite.sum()) == N - 1
    assert _invalid_units(kind, alg.storage) == [2]
    for a, b in zip(before, _live_states(alg)):                            # the bootstrap value does not advance the live state
        assert _bits_equal(a, b)
    _update(kind, alg)
    assert alg.last_nonfinite_act == 0 and alg.last_nonfinite_envs == 1
    assert bool(torch.isfinite(_state(alg)["flat"]).all()) and bool(torch.isfinite(ref["state"]["flat"]).all())


@functools.lru_cache(maxsize=None)
def _graphed_reference():
    alg = _make("ppo", False)
    return _rollout("ppo", alg, graph=True)


@pytest.mark.parametrize("nan_obs", [False, True])
def test_graphed_rollout_step_with_the_flag(nan_obs):
    """PPO.graph_rollout: the new launch runs behind the replay, outside the captured graph, on the capture's static output buffers.  The
    exploration noise of a replay is not the eager launches', so actions are compared with the graphed run without the flag; the value
    head draws nothing and is compared with it too."""
    ref = _graphed_reference()
    s, e = NAN_OBS["step"], NAN_OBS["env"]
    others = [n for n in range(N) if n != e]
    alg = _make("ppo", True)
    run = _rollout("ppo", alg, nan_obs=nan_obs, graph=True)
    assert len(alg._rollout_graphs) == 1
    want = torch.zeros(T, N, dtype=torch.uint8)
    if nan_obs:
        want[s, e] = 1
    assert torch.equal(run["masks"], want) and torch.equal(run["act_valid"], 1 - want)
    assert _bits_equal(run["actions"][:, others], ref["actions"][:, others])
    assert _bits_equal(run["storage"]["values"][:, others], ref["storage"]["values"][:, others])
    assert _bits_equal(run["storage"]["actions"], run["actions"])          # the transition stored what act() returned
    if nan_obs:
        assert not bool(run["actions"][s, e].view(torch.int32).any()) and bool(torch.isfinite(run["actions"]).all())
        rest = [t for t in range(T) if t != s]
        assert _bits_equal(run["actions"][rest], ref["actions"][rest])
    else:
        assert _bits_equal(run["actions"], ref["actions"])
        for k in ref["storage"]:
            assert _bits_equal(run["storage"][k], ref["storage"][k]), k


# ------------------------------------------------------------------------------------------------ 4. one forced RCCL rank, the runner
def _dirty_env():
    from dtc_amd.env import ReplayEnv

    class DirtyEnv(ReplayEnv):
        """ReplayEnv whose 6th step returns a NaN observation for env 3, with the env-side line of INTEGRATION.md.  (It does not go on
        to reset env 3 as a simulator would: the history wrapper keeps the NaN in env 3's observation history for its five steps,
        unless a done of the replay falls on env 3 in between.)"""
        calls = 0
        flagged = None

        def step(self, actions):
            self.calls += 1
            out = super().step(actions)
            if self.calls == 6:
                self.obs_buf[3, 7] = float("nan")
            if getattr(self, "nonfinite_act_envs", None) is not None:
                # the env-side line, into a buffer of its own: the dones the runner sees stay those of the run without the flag,
                # which the test compares the log entries with (one torch op, no host read)
                self.would_reset = self.reset_buf | self.nonfinite_act_envs
                self.flagged = torch.zeros_like(self.reset_buf) if self.flagged is None else self.flagged
                self.flagged += self.would_reset - self.reset_buf
                self.finite_actions = bool(getattr(self, "finite_actions", True)) and bool(torch.isfinite(actions).all())
            return self.obs_buf, self.privileged_obs_buf, self.rew_buf, self.reset_buf, self.extras
    return DirtyEnv


DP_MODELS = dict(
    ppo=dict(policy_class_name="ActorCriticDecoder", algorithm_class_name="PPO", policy=dict()),
    rppo_gru=dict(policy_class_name="ActorCriticRecurrent", algorithm_class_name="RecurrentPPO",
                  policy=dict(actor_hidden_dims=[512, 256, 128], critic_hidden_dims=[512, 256, 128], activation="elu", rnn_type="gru",
                              rnn_hidden_size=128, rnn_num_layers=1)),
    rppo_lstm2=dict(policy_class_name="ActorCriticRecurrent", algorithm_class_name="RecurrentPPO",
                    policy=dict(actor_hidden_dims=[512, 256, 128], critic_hidden_dims=[512, 256, 128], activation="elu", rnn_type="lstm",
                                rnn_hidden_size=50, rnn_num_layers=2)),
    rdppo=dict(policy_class_name="ActorCriticDecoderRecurrent", algorithm_class_name="RecurrentDecoderPPO", policy=dict()))
# (env class, flag) of the runs of a model.  PPO keeps a NaN observation in its row without the flag, so both of its runs are dirty.  On
# the recurrent models the flag-off run of a dirty rollout loses every env of the step and update() raises: their
# with / without comparison runs on the clean replay, and a third run, dirty, with the flag, shows the job's sum
DP_RUNS = dict(ppo=(("without", "dirty", False), ("with", "dirty", True)),
               recurrent=(("without", "clean", False), ("with", "clean", True), ("dirty", "dirty", True)))


def _dp_child(port, log_dir, out, model):
    import torch.distributed as dist
    from dtc_amd import distributed as dp
    from dtc_amd.env import ReplayEnv
    from dtc_amd.runners import OnPolicyRunner
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device(DEV), timeout=datetime.timedelta(seconds=120))
    cfg = DP_MODELS[model]
    runner = dict(policy_class_name=cfg["policy_class_name"], algorithm_class_name=cfg["algorithm_class_name"], num_steps_per_env=T,
                  save_interval=100)
    try:
        for name, env_kind, flag in DP_RUNS["ppo" if model == "ppo" else "recurrent"]:
            with dp.force_data_parallel(True):
                dp.trace_collectives(True)
                torch.manual_seed(3)
                algo = dict(learning_rate=1e-3, num_learning_epochs=1, contain_nonfinite_envs=True, contain_nonfinite_act=flag)
                env = (_dirty_env() if env_kind == "dirty" else ReplayEnv)(N, DEV, seed=0)
                os.makedirs(os.path.join(log_dir, name))
                r = OnPolicyRunner(env, dict(runner=runner, algorithm=algo, policy=dict(cfg["policy"])), log_dir=os.path.join(log_dir, name),
                                   device=DEV)
                scalars, log = [], r.log
                r.log = lambda *a, **k: scalars.append(log(*a, **k)) or scalars[-1]
                r.learn(2)
                torch.cuda.synchronize()
                flagged = getattr(env, "flagged", None)
                out[name] = dict(scalars=scalars, log=dp.assert_same_collective_sequence(), flat=r.alg.actor_critic.arena.flat.cpu(),
                                 flagged=None if flagged is None else flagged.cpu(), finite_actions=getattr(env, "finite_actions", None),
                                 same_mask=getattr(env, "nonfinite_act_envs", None) is getattr(r.alg, "nonfinite_act_envs", 0))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("model", list(DP_MODELS))
def test_one_forced_rccl_rank_logs_the_jobs_sum_and_keeps_the_present_entries(tmp_path, model):
    import torch.multiprocessing as mp
    import test_hip_dp as D
    ctx = mp.get_context("spawn")
    out = ctx.Manager().dict()
    p = ctx.Process(target=_dp_child, args=(D._free_port(), str(tmp_path), out, model))
    p.start()
    p.join(300)
    assert p.exitcode == 0, f"child exited with {p.exitcode}"
    without, with_ = out["without"], out["with"]
    dirty = with_ if model == "ppo" else out["dirty"]
    assert len(without["scalars"]) == len(with_["scalars"]) == len(dirty["scalars"]) == 2
    # the job's sum (one rank).  The NaN observation is part of env 3's five-step observation history at five consecutive act() calls;
    # RecurrentPPO takes no history: one call
    count = 1 if model.startswith("rppo") else 5
    assert [s["Train/nonfinite_act"] for s in dirty["scalars"]] == [count, 0]
    assert [s["Train/nonfinite_envs"] for s in dirty["scalars"]] == [1, 0]
    if model != "ppo":
        assert [s["Train/nonfinite_act"] for s in with_["scalars"]] == [0, 0] == [s["Train/nonfinite_envs"] for s in with_["scalars"]]
    for a, b in zip(without["scalars"], with_["scalars"]):
        assert "Train/nonfinite_act" not in a
        timed = {k for k in b if k.startswith("Perf/")}
        assert set(b) == set(a) | {"Train/nonfinite_act"} and timed == {"Perf/total_fps", "Perf/collection time", "Perf/learning_time"}
        for k in a:
            if k not in timed:
                assert a[k] == b[k], k                                       # position and value of every present entry
    assert torch.equal(without["flat"], with_["flat"]) and bool(torch.isfinite(with_["flat"]).all())
    assert bool(torch.isfinite(dirty["flat"]).all())
    # the one all-reduce of the iteration carries one more float64, behind the others
    per_it = lambda res: [e[1] for e in res["log"] if e[0] == "all_reduce_sum" and e[2] == "float64" and e[1] >= 10]
    assert per_it(without) == [11, 11] and per_it(with_) == [12, 12] == per_it(dirty)
    assert len(with_["log"]) == len(without["log"])
    # the env side saw the mask through the attribute the runner set: env 3, at those steps, and never a non-finite action
    assert without["flagged"] is None and dirty["same_mask"] and dirty["finite_actions"] is True
    want = torch.zeros(N, dtype=torch.long)
    want[3] = count
    assert torch.equal(dirty["flagged"], want)
