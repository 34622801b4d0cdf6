"""contain_nonfinite_envs=True on all three trainers: envs of the stored rollout that hold anything non-finite -- a stored element, a
saved hidden state, the bootstrap value, a return or an advantage -- are overwritten in the storage by valid envs before
RolloutStorage.compute_returns (rollout_storage.py:138-152) takes its statistics, and update() is the default update.

Every case: 16 envs x 24 steps, 4 mini-batches (env slices of 4 for the recurrent trainers), 2 epochs, the synthetic rollout of
dtc_amd.synthetic.  A contained update is the default update on a repaired storage and nothing else: the dirty case is compared bit for bit
with a trainer WITHOUT the flag whose storage the test repairs itself, with torch indexing, by the replacement rule."""
import datetime
import os

import numpy as np
import pytest
import torch

from dtc_amd import synthetic as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T, N, NMB, EPOCHS = 24, 16, 4, 2
KINDS = ("gru", "lstm2", "rppo", "ppo")
RECURRENT = ("gru", "lstm2", "rppo")
SCANNED = ("observations", "next_observations", "privileged_observations", "observation_histories", "actions", "rewards", "values",
           "actions_log_prob", "mu", "sigma", "base_vel")
# name -> list of (where, index, value); where: a storage attribute, "hidden_a" / "hidden_c" (first state tensor), or "last_values"
DIRT = dict(observation=[("observations", (5, 3, 7), "nan")],
            reward=[("rewards", (9, 6, 0), "inf")],
            privileged=[("privileged_observations", (23, 15, 1388), "nan")],
            hidden=[("hidden_a", (0, 0, 10, 1), "nan")],                    # t = 0: a trajectory start of every env
            last_value=[("last_values", (12, 0), "-inf")],
            two_slices=[("actions", (2, 1, 11), "nan"), ("base_vel", (17, 14, 2), "inf")])
HIDDEN_C = [("hidden_c", (17, 0, 14, 0), "inf")]


def _states_shapes(kind):
    """(tensors per memory, layers, H) of the saved hidden states"""
    return dict(gru=(1, 1, 512), lstm2=(2, 2, 50), rppo=(1, 1, 512), ppo=None)[kind]


def _make(kind, **kw):
    """A trainer of `kind` on the synthetic rollout, from the same weights every time; returns are NOT computed yet."""
    from dtc_amd.algorithms import PPO, RecurrentDecoderPPO, RecurrentPPO
    from dtc_amd.modules import ActorCriticDecoder, ActorCriticDecoderRecurrent, ActorCriticRecurrent
    common = dict(learning_rate=1e-3, entropy_coef=0.003, device=DEV, num_learning_epochs=EPOCHS, num_mini_batches=NMB, **kw)
    torch.manual_seed(3)
    if kind == "ppo":
        alg = PPO(ActorCriticDecoder(53, 1389, 12), **common)
    elif kind == "rppo":
        ac = ActorCriticRecurrent(53, 1389, 12, actor_hidden_dims=[512, 256, 128], critic_hidden_dims=[512, 256, 128], activation='elu',
                                  rnn_type='gru', rnn_hidden_size=512, rnn_num_layers=1)
        alg = RecurrentPPO(ac, **common)
    elif kind == "gru":
        alg = RecurrentDecoderPPO(ActorCriticDecoderRecurrent(53, 1389, 12), **common)
    else:
        alg = RecurrentDecoderPPO(ActorCriticDecoderRecurrent(53, 1389, 12, rnn_type="lstm", rnn_num_layers=2, rnn_hidden_size=50), **common)
    if kind == "rppo":
        alg.init_storage(N, T, [53], [1389], [12])
    else:
        alg.init_storage(N, T, [53], [1389], [265], [12])
    d = S.rollout(N, T, seed=4)
    if kind != "ppo":
        d["dones"][:, 0] = 0                                               # one env without a reset: a full-length trajectory
    st = alg.storage
    for k, v in d.items():
        if k == "last_values" or (kind == "rppo" and k == "observation_histories"):
            continue
        getattr(st, k).copy_(v.to(DEV))
    st.step = T
    shp = _states_shapes(kind)
    if shp is not None:
        g = torch.Generator().manual_seed(55)
        per, L, H = shp
        st.saved_hidden_states_a, st.saved_hidden_states_c = ([(0.1 * torch.randn(T, L, N, H, generator=g)).to(DEV) for _ in range(per)]
                                                              for _ in range(2))
    return alg, d["last_values"].to(DEV).clone()


def _plant(alg, last_values, dirt):
    st = alg.storage
    for where, index, value in DIRT[dirt] if isinstance(dirt, str) else dirt:
        target = last_values if where == "last_values" else st.saved_hidden_states_a[0] if where == "hidden_a" else \
            st.saved_hidden_states_c[0] if where == "hidden_c" else getattr(st, where)
        target[index] = float(value)


def _applies(kind, dirt):
    return not (kind == "ppo" and any(w.startswith("hidden") for w, _, _ in DIRT[dirt]))


def _noise():
    perm, e1, e2 = S.update_noise(N, T, NMB, EPOCHS, seed=123)
    return perm.to(DEV), e1.to(DEV), e2.to(DEV)


def _update(kind, alg):
    perm, e1, e2 = _noise()
    if kind == "ppo":
        return alg.update(perm=perm, eps1=e1, eps2=e2)
    if kind == "rppo":
        return alg.update()
    return alg.update(eps1=e1, eps2=e2)


def _state(alg):
    out = dict(flat=alg.actor_critic.arena.flat.clone(), lr=alg.learning_rate, stats=alg.last_update_stats.clone())
    for i, opt in enumerate([alg.optimizer] + ([alg.vae_optimizer] if hasattr(alg, "vae_optimizer") else [])):
        out[f"m{i}"], out[f"v{i}"], out[f"lr_dev{i}"] = opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.lr_dev.clone()
    return {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in out.items()}


def _first_difference(a, b):
    assert a.keys() == b.keys()
    for k in a:
        # (bit for bit: NaN patterns included)
        same = (a[k].shape == b[k].shape and torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8))) if torch.is_tensor(a[k]) \
            else a[k] == b[k]
        if not same:
            return k
    return None


def _storage_tensors(st):
    out = {k: getattr(st, k) for k in SCANNED + ("dones", "returns", "advantages")}
    for name, net in (("hidden_a", st.saved_hidden_states_a), ("hidden_c", st.saved_hidden_states_c)):
        for i, s in enumerate(net or []):
            out[f"{name}{i}"] = s
    return out


def _env_valid_numpy(st, last_values):
    """the env record on the host: every stored element, every layer's saved state and the bootstrap value of the env finite, and the
    float32 GAE scan of rollout_storage.py:138-150 gives finite returns and advantages at all its steps"""
    f = np.float32
    ok = np.ones((T, N), dtype=bool)
    for name in SCANNED:
        ok &= np.isfinite(getattr(st, name).cpu().numpy()).all(-1)
    for net in (st.saved_hidden_states_a, st.saved_hidden_states_c):
        for s in net or []:
            ok &= np.isfinite(s.cpu().numpy()).all(axis=(1, 3))
    r, v, d = (getattr(st, k).cpu().numpy()[..., 0] for k in ("rewards", "values", "dones"))
    adv, nxt = np.zeros(N, dtype=f), last_values.cpu().numpy().reshape(-1).astype(f)
    ok &= np.isfinite(nxt)[None, :]
    with np.errstate(all="ignore"):
        for t in range(T - 1, -1, -1):
            ng = (f(1.0) - d[t].astype(f)) * f(0.99)
            delta = (r[t] + ng * nxt) - v[t]
            adv = delta + (ng * f(0.95)) * adv
            ret = adv + v[t]
            ok[t] &= np.isfinite(ret) & np.isfinite(ret - v[t])
            nxt = v[t]
    return ok.all(axis=0)


def _sources_numpy(env_valid):
    valid_list = np.nonzero(env_valid)[0]
    src = np.arange(env_valid.size)
    if valid_list.size:
        bad = np.nonzero(~env_valid)[0]
        src[bad] = valid_list[bad % valid_list.size]
    return src


# ------------------------------------------------------------------------------------------------ 1. clean rollout
@pytest.mark.parametrize("kind", KINDS)
def test_clean_rollout_gives_the_bits_of_the_default_update(kind):
    states, storages = [], []
    for flag in (False, True):
        alg, lv = _make(kind, contain_nonfinite_envs=flag)
        st = alg.storage
        before = {k: v.clone() for k, v in _storage_tensors(st).items()}
        st.compute_returns(lv, 0.99, 0.95)
        after = _storage_tensors(st)
        for k in before:
            if k not in ("returns", "advantages"):
                assert torch.equal(before[k].view(torch.uint8), after[k].view(torch.uint8)), (k, flag)
        assert float(lv.abs().sum()) == 0.0                                # the caller's bootstrap values stay the caller's
        if flag:
            assert st.env_record_fresh and int(st.n_valid_envs) == N and bool(st.env_valid.all())
            assert torch.equal(st.env_src.cpu(), torch.arange(N))
        else:
            assert st.env_valid is None and st.env_src is None and not st.env_record_fresh and not hasattr(st, "_env_rows")
        storages.append({k: v.clone() for k, v in after.items()})
        _update(kind, alg)
        assert alg.last_nonfinite_envs == 0 and not st.env_record_fresh
        states.append(_state(alg))
    for k in storages[0]:
        assert torch.equal(storages[0][k].view(torch.uint8), storages[1][k].view(torch.uint8)), k
    assert _first_difference(*states) is None
    assert bool(torch.isfinite(states[0]["flat"]).all())


# ------------------------------------------------------------------------------------------------ 2. the need
@pytest.mark.parametrize("kind", RECURRENT)
def test_dirty_rollout_without_the_flag_ends_the_run(kind):
    """today's behaviour and the reason for the feature: one NaN reward among 384 samples and the weights are not finite after the update"""
    alg, lv = _make(kind)
    _plant(alg, lv, [("rewards", (9, 6, 0), "nan")])
    alg.storage.compute_returns(lv, 0.99, 0.95)
    _update(kind, alg)
    assert not bool(torch.isfinite(alg.actor_critic.arena.flat).all())


# ------------------------------------------------------------------------------------------------ 3. contained
@pytest.mark.parametrize("kind,dirt", [(k, d) for k in KINDS for d in DIRT if _applies(k, d)])     # (plain PPO saves no hidden states)
def test_dirty_rollout_is_contained(kind, dirt):
    alg, lv = _make(kind, contain_nonfinite_envs=True)
    _plant(alg, lv, dirt)
    st = alg.storage
    want = _env_valid_numpy(st, lv)
    bad_envs = sorted({index[-2] if where.startswith("hidden") else index[0] if where == "last_values" else index[1]
                       for where, index, _ in DIRT[dirt]})
    assert sorted(np.nonzero(~want)[0].tolist()) == bad_envs               # the dirt's envs, and no others
    st.compute_returns(lv, 0.99, 0.95)
    assert np.array_equal(st.env_valid.cpu().numpy().astype(bool), want)
    assert np.array_equal(st.env_src.cpu().numpy(), _sources_numpy(want)) and int(st.n_valid_envs) == N - len(bad_envs)
    for k, v in _storage_tensors(st).items():
        assert bool(torch.isfinite(v.float()).all()), k
    out = _update(kind, alg)
    assert isinstance(alg.last_nonfinite_envs, int) and alg.last_nonfinite_envs == len(bad_envs)
    assert bool(torch.isfinite(alg.actor_critic.arena.flat).all())
    assert bool(torch.isfinite(alg.last_update_stats).all()) and all(np.isfinite(v) for v in out)
    assert 1e-5 <= alg.learning_rate <= 1e-2
    assert not st.env_record_fresh                                         # the update cleared the storage: its record is void


# ------------------------------------------------------------------------------------------------ 4. equivalence
@pytest.mark.parametrize("kind", KINDS)
def test_a_contained_update_is_the_default_update_on_a_repaired_storage(kind):
    dirt = DIRT["observation"] + DIRT["reward"] + DIRT["last_value"] + ([] if kind == "ppo" else DIRT["hidden"] + HIDDEN_C)
    alg, lv = _make(kind, contain_nonfinite_envs=True)
    _plant(alg, lv, dirt)
    want = _env_valid_numpy(alg.storage, lv)
    assert int((~want).sum()) == (3 if kind == "ppo" else 5)
    alg.storage.compute_returns(lv, 0.99, 0.95)
    _update(kind, alg)
    # the same dirt, repaired here by the rule with torch indexing, through the DEFAULT compute_returns and update
    plain, lv2 = _make(kind)
    _plant(plain, lv2, dirt)
    src = torch.from_numpy(_sources_numpy(want)).to(DEV)
    for k, v in _storage_tensors(plain.storage).items():
        v.copy_(v.index_select(2 if k.startswith("hidden") else 1, src))
    plain.storage.compute_returns(lv2[src].contiguous(), 0.99, 0.95)
    assert plain.storage.env_valid is None
    _update(kind, plain)
    assert _first_difference(_state(alg), _state(plain)) is None
    assert bool(torch.isfinite(alg.actor_critic.arena.flat).all()) and alg.last_nonfinite_envs == int((~want).sum())


# ------------------------------------------------------------------------------------------------ 5. errors
@pytest.mark.parametrize("kind", ("gru", "rppo", "ppo"))
def test_no_valid_env_and_a_stale_record_are_errors(kind):
    from dtc_amd import _ffi
    alg, lv = _make(kind, contain_nonfinite_envs=True)
    with pytest.raises(_ffi.DtcError, match="no env record"):              # compute_returns has not run for this rollout
        _update(kind, alg)
    alg.storage.compute_returns(lv, 0.99, 0.95)
    _update(kind, alg)                                                     # ... clears the storage: the record is void
    with pytest.raises(_ffi.DtcError, match="no env record"):
        _update(kind, alg)
    alg, lv = _make(kind, contain_nonfinite_envs=True)
    alg.storage.rewards.fill_(float("nan"))
    alg.storage.compute_returns(lv, 0.99, 0.95)
    assert torch.equal(alg.storage.env_src.cpu(), torch.arange(N)) and int(alg.storage.n_valid_envs) == 0
    with pytest.raises(_ffi.DtcError, match=f"0 valid envs of {N}"):
        _update(kind, alg)
    assert alg.last_nonfinite_envs == N and alg.storage.step == 0 and not alg.storage.env_record_fresh


def test_both_containment_flags_together_are_refused():
    from dtc_amd.algorithms import PPO
    from dtc_amd.modules import ActorCriticDecoder
    with pytest.raises(ValueError, match="contain_nonfinite_envs"):
        PPO(ActorCriticDecoder(53, 1389, 12), device=DEV, contain_nonfinite=True, contain_nonfinite_envs=True)


# ------------------------------------------------------------------------------------------------ 6. one forced data-parallel rank
def _dp_child(port, out):
    import torch.distributed as dist
    from dtc_amd import distributed as dp
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device(DEV), timeout=datetime.timedelta(seconds=120))
    try:
        for name, flag, forced in (("default", False, True), ("forced", True, True), ("plain", True, False)):
            with dp.force_data_parallel(forced):
                dp.trace_collectives(True)
                alg, lv = _make("gru", contain_nonfinite_envs=flag)
                if flag:
                    _plant(alg, lv, "two_slices")
                before = len(dp.collective_log())
                alg.storage.compute_returns(lv, 0.99, 0.95)
                returns_log = dp.collective_log()[before:]
                _update("gru", alg)
                torch.cuda.synchronize()
                log = dp.assert_same_collective_sequence()
                out[name] = dict(state=_state(alg), returns_log=returns_log, log=log, envs=alg.last_nonfinite_envs)
    finally:
        dist.destroy_process_group()


def test_one_forced_data_parallel_rank_gives_the_same_bits():
    import torch.multiprocessing as mp
    import test_hip_dp as D
    ctx = mp.get_context("spawn")
    out = ctx.Manager().dict()
    p = ctx.Process(target=_dp_child, args=(D._free_port(), out))
    p.start()
    p.join(300)
    assert p.exitcode == 0, f"child exited with {p.exitcode}"
    default, forced, plain = out["default"], out["forced"], out["plain"]
    # compute_returns: the sum in one collective, the squared deviations in a second -- as without the flag; each rank repairs locally
    assert [e[:3] for e in forced["returns_log"]] == [("all_reduce_sum", 1, "float64")] * 2 == [e[:3] for e in default["returns_log"]]
    assert forced["log"] == default["log"] and len(forced["log"]) > 2      # ops, sizes, dtypes and lanes of the whole update
    assert plain["returns_log"] == [] and plain["log"] == []
    assert _first_difference(forced["state"], plain["state"]) is None
    assert bool(torch.isfinite(forced["state"]["flat"]).all()) and forced["envs"] == plain["envs"] == 2


# ------------------------------------------------------------------------------------------------ 7. runner
def test_runner_passes_the_keyword_and_logs_the_count():
    from dtc_amd.env import ReplayEnv
    from dtc_amd.runners import OnPolicyRunner
    runner = dict(policy_class_name="ActorCriticDecoderRecurrent", algorithm_class_name="RecurrentDecoderPPO", num_steps_per_env=T,
                  save_interval=10)
    for algo, want in ((dict(learning_rate=1e-3, num_learning_epochs=1, contain_nonfinite_envs=True), True),
                       (dict(learning_rate=1e-3, num_learning_epochs=1), False)):
        r = OnPolicyRunner(ReplayEnv(N, DEV), dict(runner=runner, algorithm=algo, policy=dict()), log_dir=None, device=DEV)
        assert r.alg.contain_nonfinite_envs is want and r.alg.storage.contain_nonfinite_envs is want
        r.learn(1)
        assert r.alg.last_nonfinite_envs == 0 and (r.alg.storage.env_valid is not None) is want
        sd = r.alg.actor_critic.state_dict()
        assert all(torch.isfinite(v).all() for v in sd.values())
        scalars = r.log(1, 2, (0.0,) * 7, collection_time=1.0, learn_time=1.0, tracker=None, finished=None)
        assert ("Train/nonfinite_envs" in scalars) is want
        if want:
            assert scalars["Train/nonfinite_envs"] == 0
