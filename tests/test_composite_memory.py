"""The recurrent composite (ActorCriticDecoderRecurrent + RecurrentDecoderPPO) with LSTM and stacked memories, and the fused
LSTM time step (dtc_lstm_step_fwd / dtc_lstm_fwd_fused) it runs on.

Oracle: oracle.composite_ref.RefCompositeAC with its `.acr` replaced by oracle.gru_ref.RefActorCriticRecurrent(..., rnn_type,
num_layers) -- the same composition with torch.nn.LSTM / a deeper torch.nn.GRU -- stepped by RefCompositePPO (its forward hands
the hidden states to `rnn(...)` as they come: a tensor for a GRU, (h, c) for an LSTM).  The recurrent mini-batches come from a
tuple-aware restatement of composite_ref.recurrent_slices below (rollout_storage.py:261-262: for an LSTM the critic receives the
actor's saved states)."""
import ctypes

import numpy as np
import pytest
import torch

from dtc_amd import synthetic as S
from oracle import composite_ref as CR
from oracle import gru_ref as GR
from oracle import ppo_ref as OP

DEV = "cuda:0"
N, NMB, T = 16, 4, 24
# (rnn_type, rnn_num_layers, rnn_hidden_size): AC_Args' values (actor_critic_decoder.py:85-88) among them
CONFIGS = [("lstm", 1, 512), ("lstm", 2, 512), ("gru", 2, 50), ("lstm", 1, 50)]


def oracle_model(rnn_type, layers, H):
    torch.manual_seed(3)
    m = CR.RefCompositeAC()
    m.acr = GR.RefActorCriticRecurrent(CR.ACTOR_FEATURES, CR.CRITIC_FEATURES, 12, (512, 256, 128), H, rnn_type, layers)
    return OP.fill_parameters_(m, 23)


def hip_model(rnn_type, layers, H):
    from dtc_amd.modules import ActorCriticDecoderRecurrent
    return ActorCriticDecoderRecurrent(53, 1389, 12, rnn_type=rnn_type, rnn_num_layers=layers, rnn_hidden_size=H)


def _strip(sd):
    return {k.replace("acr.", ""): v for k, v in sd.items()}


def saved_states(rnn_type, layers, H, n, seed=77):
    """Saved hidden states [T, L, n, H] of both memories (a pair (h, c) of them each for an LSTM)."""
    g = torch.Generator().manual_seed(seed)
    r = lambda: 0.1 * torch.randn(T, layers, n, H, generator=g)
    if rnn_type == "lstm":
        return (r(), r()), (r(), r())
    return r(), r()


def recurrent_slices(st, hid_a, hid_c, num_mini_batches):
    """composite_ref.recurrent_slices for GRU states [T, L, N, H] and LSTM states (h, c): the states at the trajectory starts
    are [L, R, H] (a pair of them for an LSTM), and an LSTM's critic receives the ACTOR's states (rollout_storage.py:261-262)."""
    T_, N_ = st.dones.shape[0], st.dones.shape[1]
    mb = N_ // num_mini_batches
    dones = st.dones.squeeze(-1)
    lwd = torch.zeros_like(dones, dtype=torch.bool)
    lwd[1:] = dones[:-1].bool()
    lwd[0] = True
    tup = isinstance(hid_a, (tuple, list))
    for i in range(num_mini_batches):
        a, b = i * mb, (i + 1) * mb
        idx = (torch.arange(T_).unsqueeze(1) * N_ + torch.arange(a, b)).reshape(-1)
        pick1 = lambda h: h[:, :, a:b].permute(2, 0, 1, 3)[lwd[:, a:b].permute(1, 0)].transpose(1, 0).contiguous()
        pick = lambda h: tuple(pick1(x) for x in h) if tup else pick1(h)
        ha = pick(hid_a)
        yield dict(a=a, b=b, idx=idx, dones=st.dones[:, a:b], hid_a=ha, hid_c=ha if tup else pick(hid_c))


def _dev(h):
    return tuple(x.to(DEV) for x in h) if isinstance(h, tuple) else h.to(DEV)


# ------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("rnn_type,layers,H", CONFIGS)
def test_composite_constructs_with_oracle_state_dict(rnn_type, layers, H):
    ac = hip_model(rnn_type, layers, H)
    assert ac.memory_a.kind == rnn_type and ac.memory_a.num_layers == layers and ac.rnn_hidden_size == H
    mine = {k: tuple(v.shape) for k, v in ac.state_dict().items()}
    ref = {k: tuple(v.shape) for k, v in _strip(oracle_model(rnn_type, layers, H).state_dict()).items()}
    assert sorted(mine) == sorted(ref)
    assert mine == ref
    assert f"memory_c.rnn.weight_hh_l{layers - 1}" in mine
    ac.load_state_dict(_strip(oracle_model(rnn_type, layers, H).state_dict()))      # a reference-style checkpoint loads


def test_composite_keeps_activation_check():
    from dtc_amd.modules import ActorCriticDecoderRecurrent
    with pytest.raises(NotImplementedError):
        ActorCriticDecoderRecurrent(53, 1389, 12, activation="tanh", rnn_type="lstm", rnn_num_layers=2)


def test_lstm_step_entry_points_reject_bad_arguments():
    """Shape and null-pointer checks run before any device work (no GPU needed)."""
    from dtc_amd import _ffi
    lib = _ffi.lib()
    p = ctypes.cast(ctypes.create_string_buffer(64), ctypes.POINTER(ctypes.c_float))
    assert lib.dtc_lstm_step_fwd(*[p] * 8, 64, 50, None) == -1
    assert b"multiple of 32" in lib.dtc_last_error()
    assert lib.dtc_lstm_step_fwd(*[p] * 8, 0, 64, None) == -1
    assert lib.dtc_lstm_step_fwd(p, None, *[p] * 6, 64, 64, None) == -1
    assert b"null" in lib.dtc_last_error()
    assert lib.dtc_lstm_step_fwd(*[p] * 8, 1 << 20, 512, None) == -1
    assert b"too large" in lib.dtc_last_error()
    assert lib.dtc_lstm_fwd_fused(*[p] * 8, None, 24, 64, 64, None) == -1
    assert b"null" in lib.dtc_last_error()
    assert lib.dtc_lstm_fwd_fused(*[p] * 8, p, 0, 64, 64, None) == -1


# ------------------------------------------------------------------------------------------ GPU: the fused LSTM time step
def _lstm_case(T_, R, H, I=16, seed=0):
    g = torch.Generator().manual_seed(seed * 7919 + R * 31 + H)
    rnn = torch.nn.LSTM(input_size=I, hidden_size=H, num_layers=1)
    with torch.no_grad():
        for p in rnn.parameters():
            p.copy_(torch.randn(p.shape, generator=g) / (p.shape[-1] ** 0.5 if p.dim() == 2 else 4.0))
    rnn = rnn.double()
    x = torch.randn(T_, R, I, generator=g, dtype=torch.float64)
    h0 = 0.5 * torch.randn(1, R, H, generator=g, dtype=torch.float64)
    c0 = 0.5 * torch.randn(1, R, H, generator=g, dtype=torch.float64)
    with torch.no_grad():
        out, (hT, cT) = rnn(x, (h0, c0))
        gi = x @ rnn.weight_ih_l0.T + rnn.bias_ih_l0
    f = lambda t: t.detach().float().contiguous().to(DEV)
    return rnn, out, cT, dict(gi=f(gi), h0=f(h0[0]), c0=f(c0[0]), W_hh=f(rnn.weight_hh_l0), b_hh=f(rnn.bias_hh_l0))


def _run(fn, d, T_, R, H):
    from dtc_amd import ops
    hs, cs, gates = (torch.empty(T_ + 1, R, H, device=DEV), torch.empty(T_ + 1, R, H, device=DEV),
                     torch.empty(T_, R, 4 * H, device=DEV))
    ws = ops.workspace(ops.lstm_workspace_bytes(T_, R, H), DEV)
    fn(d["gi"], d["h0"], d["c0"], d["W_hh"], d["b_hh"], hs, cs, gates, ws)
    return hs, cs, gates


@pytest.mark.gpu
@pytest.mark.parametrize("H", [32, 128, 256, 512])
@pytest.mark.parametrize("R", [1, 37, 1536, 4096])
def test_hip_lstm_fused_vs_torch_float64(R, H):
    """dtc_lstm_fwd_fused (T = 24) and one dtc_lstm_step_fwd against torch.nn.LSTM in float64, at the bound test_hip_lstm.py holds
    dtc_lstm_fwd to (2e-5 relative and absolute); dtc_lstm_fwd on the same inputs is reported alongside."""
    from dtc_amd import ops
    rnn, out, cT, d = _lstm_case(T, R, H)
    hs, cs, gates = _run(ops.lstm_fwd_fused, d, T, R, H)
    hs0, cs0, gates0 = _run(ops.lstm_fwd, d, T, R, H)
    torch.cuda.synchronize()
    ref = out.numpy()
    np.testing.assert_allclose(hs[1:].cpu().double().numpy(), ref, rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(cs[-1].cpu().double().numpy(), cT[0].numpy(), rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(hs0[1:].cpu().double().numpy(), ref, rtol=2e-5, atol=2e-5)
    assert torch.equal(hs[0], d["h0"]) and torch.equal(cs[0], d["c0"])
    np.testing.assert_allclose(gates.cpu().numpy(), gates0.cpu().numpy(), rtol=2e-5, atol=2e-5)
    # one step on its own: the first time step of the float64 recurrence
    h1, c1, g1 = torch.empty(R, H, device=DEV), torch.empty(R, H, device=DEV), torch.empty(R, 4 * H, device=DEV)
    ops.lstm_step_fwd(d["h0"], d["c0"], d["W_hh"], d["b_hh"], d["gi"][0], h1, c1, g1)
    np.testing.assert_allclose(h1.cpu().double().numpy(), ref[0], rtol=2e-5, atol=2e-5)
    assert torch.equal(h1, hs[1]) and torch.equal(c1, cs[1]) and torch.equal(g1, gates[0])
    print(f"R={R} H={H}: max |fused - float64| h {float((hs[1:].cpu().double() - out).abs().max()):.2e}, "
          f"max |fused - dtc_lstm_fwd| h {float((hs - hs0).abs().max()):.2e} c {float((cs - cs0).abs().max()):.2e} "
          f"gates {float((gates - gates0).abs().max()):.2e}")


@pytest.mark.gpu
def test_hip_lstm_fused_fallback_off_the_32_grid():
    """H % 32 != 0: dtc_lstm_fwd_fused runs dtc_lstm_fwd's GEMM + gate pair -- the same bits."""
    from dtc_amd import _ffi, ops
    rnn, out, cT, d = _lstm_case(T, 37, 50)
    hs, cs, gates = _run(ops.lstm_fwd_fused, d, T, 37, 50)
    hs0, cs0, gates0 = _run(ops.lstm_fwd, d, T, 37, 50)
    assert torch.equal(hs, hs0) and torch.equal(cs, cs0) and torch.equal(gates, gates0)
    np.testing.assert_allclose(hs[1:].cpu().double().numpy(), out.numpy(), rtol=2e-5, atol=2e-5)
    with pytest.raises(_ffi.DtcError, match="multiple of 32"):
        ops.lstm_step_fwd(d["h0"], d["c0"], d["W_hh"], d["b_hh"], d["gi"][0], hs[1], cs[1], gates[0])


# ------------------------------------------------------------------------------------------ GPU: rollout mode
@pytest.mark.gpu
@pytest.mark.parametrize("rnn_type,layers,H", CONFIGS)
def test_hip_rollout_mode_carries_and_resets_state(rnn_type, layers, H):
    """24 rollout steps with random dones: mean actions, values and every layer's h (and c) against the oracle stepped one step at a
    time, done envs reset in every layer (rtol 1e-5, atol 2e-6: the bound of test_hip_rollout_mode_forward_carries_state)."""
    data = S.rollout(N, T, seed=6)
    g = torch.Generator().manual_seed(5)
    dones = torch.rand(T, N, generator=g) < 0.15
    rac = oracle_model(rnn_type, layers, H)
    ac = hip_model(rnn_type, layers, H).to(DEV)
    ac.load_state_dict(_strip(rac.state_dict()))
    ha = hc = None
    for t in range(T):
        e = torch.randn(N, 16, generator=g)
        obs, hist, priv, bv = (data[k][t] for k in ("observations", "observation_histories", "privileged_observations", "base_vel"))
        with torch.no_grad():
            out, ha = rac.memory_a.rnn(rac.actor_features(obs, hist, priv, e).unsqueeze(0), ha)
            mean_ref = rac.actor(out.squeeze(0))
            out, hc = rac.memory_c.rnn(rac.critic_features(obs, priv, bv).unsqueeze(0), hc)
            val_ref = rac.critic(out.squeeze(0))
        ac.update_distribution(obs.to(DEV), hist.to(DEV), priv.to(DEV), eps=e.to(DEV))
        val = ac.evaluate(obs.to(DEV), priv.to(DEV), bv.to(DEV))
        np.testing.assert_allclose(ac.action_mean.cpu().numpy(), mean_ref.numpy(), rtol=1e-5, atol=2e-6, err_msg=f"t={t}")
        np.testing.assert_allclose(val.cpu().numpy(), val_ref.numpy(), rtol=1e-5, atol=2e-6, err_msg=f"t={t}")
        for mine, ref in ((ac.memory_a.hidden_states, ha), (ac.memory_c.hidden_states, hc)):
            mine, ref = (mine, ref) if rnn_type == "lstm" else ((mine,), (ref,))
            for m, r in zip(mine, ref):
                assert m.shape == (layers, N, H)
                np.testing.assert_allclose(m.cpu().numpy(), r.numpy(), rtol=1e-5, atol=2e-6, err_msg=f"t={t}")
        ac.reset(dones[t].to(DEV))
        with torch.no_grad():
            for h in ((ha, hc) if rnn_type == "gru" else (*ha, *hc)):
                h[..., dones[t], :] = 0.0
        if bool(dones[t].any()):
            states = ac.get_hidden_states()[0]
            for s in (states if rnn_type == "lstm" else (states,)):
                assert float(s[:, dones[t].to(DEV)].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------ GPU: teacher-forced mini-batches
def _oracle_alg(data, cfg, n, **kw):
    alg = CR.RefCompositePPO(oracle_model(*cfg), learning_rate=1e-3, entropy_coef=0.003, **kw)
    alg.init_storage(n, T)
    for k, v in data.items():
        if k != "last_values":
            getattr(alg.storage, k).copy_(v)
    alg.storage.compute_returns(data["last_values"], 0.99, 0.95)
    return alg


def _hip_alg(ref, data, cfg, n, **kw):
    from dtc_amd.algorithms import RecurrentDecoderPPO
    alg = RecurrentDecoderPPO(hip_model(*cfg), learning_rate=1e-3, entropy_coef=0.003, device=DEV, **kw)
    alg.init_storage(n, T, [53], [1389], [265], [12])
    alg.actor_critic.load_state_dict(_strip(ref.actor_critic.state_dict()))
    for k, v in data.items():
        if k != "last_values":
            getattr(alg.storage, k).copy_(v.to(DEV))
    alg.storage.compute_returns(data["last_values"].to(DEV), 0.99, 0.95)
    return alg


def _memory_grads_counted(grads, layers):
    names = {k.replace("acr.", "") for k in grads}
    want = {f"memory_{s}.rnn.{w}_{p}_l{l}" for s in "ac" for w in ("weight", "bias") for p in ("ih", "hh") for l in range(layers)}
    return want <= names


def _teacher_forced(cfg, n, mini_batches, knife_edges):
    from test_composite_path import _grad_report
    from test_hip_ppo import _force_oracle_signs, _relu_mask_mismatches
    from dtc_amd.algorithms import ppo as P
    rnn_type, layers, H = cfg
    tol = 5e-5 if rnn_type == "lstm" else 2e-5
    data = S.rollout(n, T, seed=4)
    data["dones"][:, 0] = 0
    hid_a, hid_c = saved_states(*cfg, n)
    g = torch.Generator().manual_seed(78)
    B = T * (n // NMB)
    eps, eps2 = torch.randn(NMB, B, 16, generator=g), torch.randn(NMB, B, 16, generator=g)
    for i in mini_batches:
        ref = _oracle_alg(data, cfg, n)
        ref.capture_grads = True
        alg = _hip_alg(ref, data, cfg, n)
        alg.capture_grads = True
        forced = _force_oracle_signs(ref, alg)
        bt_ref = list(recurrent_slices(ref.storage, hid_a, hid_c, NMB))[i]
        bt = list(alg.recurrent_slices(_dev(hid_a), _dev(hid_c)))[i]
        R = (bt_ref["hid_a"][0] if rnn_type == "lstm" else bt_ref["hid_a"]).shape[1]
        assert bt["R"] == R and torch.equal(bt["idx"].cpu(), bt_ref["idx"])
        if rnn_type == "lstm":
            assert bt["hid_c"] is bt["hid_a"]                     # the critic starts from the actor's saved states
            assert all(torch.equal(x.cpu(), y) for x, y in zip(bt["hid_a"], bt_ref["hid_a"]))
        rec = OP.StepRecord()
        ref.vae_step(bt_ref["idx"], eps[i], rec)
        row = alg.step_minibatch(bt, eps[i].to(DEV), eps2[i].to(DEV), which="vae").cpu()
        for key, col in (("recons", P.S_RECONS), ("vel", P.S_VEL), ("kld", P.S_KLD), ("height", P.S_HEIGHT), ("vae_gnorm", P.S_VAE_GNORM)):
            assert abs(float(row[col]) - getattr(rec, key)) <= 1e-5 * max(1.0, abs(getattr(rec, key))), (i, key)
        edges = _relu_mask_mismatches(ref, alg, "vae") if knife_edges else None
        assert _grad_report(rec.extra["vae_grads"], alg, "vae", 2e-5, (), knife_edges=edges) >= 20
        alg.actor_critic.load_state_dict(_strip(ref.actor_critic.state_dict()))
        ref.ppo_step(bt_ref, eps2[i], rec)
        row = alg.step_minibatch(bt, eps[i].to(DEV), eps2[i].to(DEV), which="ppo").cpu()
        for key, col in (("surrogate", P.S_SURR), ("value", P.S_VALUE), ("entropy", P.S_ENTROPY), ("gnorm", P.S_GNORM), ("kl_mean", P.S_KL)):
            assert abs(float(row[col]) - getattr(rec, key)) <= 1e-5 * max(1.0, abs(getattr(rec, key))), (i, key, float(row[col]), getattr(rec, key))
        assert abs(float(alg.optimizer.lr_dev.item()) - ref.learning_rate) <= 1e-12
        fw = alg.actor_critic._fwd_ws(bt["idx"].numel())
        assert int(fw.info[0]) == ref.actor_critic.vae.last_outliers and int(fw.info[1]) == ref.actor_critic.vae.last_median_index, forced
        edges = _relu_mask_mismatches(ref, alg, "ppo") if knife_edges else None
        n_grads = _grad_report(rec.extra["grads"], alg, "main", tol, (), knife_edges=edges)
        # std, 2 MLPs, CE-net encoder + heads, terrain encoder, and 4 tensors per layer of each memory
        assert n_grads >= 35 + 8 * (layers - 1) and _memory_grads_counted(rec.extra["grads"], layers)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", [("lstm", 1, 512), ("lstm", 2, 512), ("gru", 2, 512)])
def test_hip_teacher_forced_minibatches_vs_oracle(cfg):
    """Each of the 4 recurrent mini-batches, VAE step + PPO step from the oracle's weights: scalars 1e-5 relative, every parameter
    gradient (BPTT through every layer of both memories into the encoders) 2e-5 (GRU) / 5e-5 (LSTM) of the tensor's max."""
    _teacher_forced(cfg, N, range(NMB), knife_edges=False)


@pytest.mark.gpu
def test_hip_teacher_forced_minibatch_full_size_lstm():
    """4096 envs, LSTM 1 layer, H = 512: the first recurrent mini-batch (~1500 padded trajectories), both steps."""
    _teacher_forced(("lstm", 1, 512), 4096, [0], knife_edges=True)


# ------------------------------------------------------------------------------------------ GPU: runner end to end
def _by_name(opt_sd, ref_module, hip_module):
    ref_pos = {k.replace("acr.", ""): i for i, (k, _) in enumerate(ref_module.named_parameters())}
    state = {}
    for j, (name, _) in enumerate(hip_module.named_parameters()):
        i = ref_pos[name]
        if i in opt_sd["state"]:
            state[j] = opt_sd["state"][i]
    return dict(state=state, param_groups=opt_sd["param_groups"])


@pytest.mark.gpu
@pytest.mark.parametrize("layers", [1, 2])
def test_runner_lstm_composite_two_updates_vs_oracle(layers, tmp_path):
    """OnPolicyRunner resolves the LSTM composite by name; two rounds of rollout -> compute_returns (the critic's state does not
    advance) -> update() (1 epoch x 4 recurrent mini-batches), each against the oracle stepping the same mini-batches from the
    same weights, Adam states and learning rate (the F4 envelope of test_two_consecutive_updates_vs_oracle); then save / load
    reproduces the same actions."""
    from dtc_amd.algorithms import ppo as P
    from dtc_amd.env import ReplayEnv
    from dtc_amd.runners import OnPolicyRunner
    n, H = 64, 512
    cfg = dict(runner=dict(policy_class_name="ActorCriticDecoderRecurrent", algorithm_class_name="RecurrentDecoderPPO",
                           num_steps_per_env=T, save_interval=10),
               algorithm=dict(learning_rate=1e-3, entropy_coef=0.003, num_learning_epochs=1),
               policy=dict(rnn_type="lstm", rnn_num_layers=layers, rnn_hidden_size=H))
    torch.manual_seed(11)
    r = OnPolicyRunner(ReplayEnv(n, DEV), cfg, log_dir=None, device=DEV)
    alg, ac = r.alg, r.alg.actor_critic
    assert ac.memory_a.kind == "lstm" and ac.memory_a.num_layers == layers
    ref = CR.RefCompositePPO(oracle_model("lstm", layers, H), learning_rate=1e-3, entropy_coef=0.003, num_learning_epochs=1)
    ref.init_storage(n, T)
    ac.load_state_dict(_strip(ref.actor_critic.state_dict()))
    cols = dict(recons=P.S_RECONS, vel=P.S_VEL, kld=P.S_KLD, height=P.S_HEIGHT, vae_gnorm=P.S_VAE_GNORM,
                surrogate=P.S_SURR, value=P.S_VALUE, entropy=P.S_ENTROPY, kl_mean=P.S_KL, gnorm=P.S_GNORM)
    envelope = (1e-5, 3e-4, 1.5e-3, 5e-3)
    state = dict(obs_dict=r.env.get_observations(), rew_buf=r.env.get_reward_buf())
    worst = []
    for u in range(2):
        # rollout (the runner's loop), then compute_returns must leave the critic's recurrent state where the rollout left it
        obs_dict = state["obs_dict"]
        obs, priv, hist = r._observe(obs_dict)
        with torch.inference_mode():
            for _ in range(T):
                actions = alg.act(obs, priv, hist, obs_dict["base_vel"], state["rew_buf"])
                obs_dict, rewards, dones, infos = r.env.step(actions)
                obs, priv, hist = r._observe(obs_dict)
                alg.process_env_step(rewards.to(DEV), dones.to(DEV), next_obs=obs_dict["obs"], infos=infos)
            before = [t.clone() for t in ac.memory_c.hidden_states]
            alg.compute_returns(obs, priv, obs_dict["base_vel"])
            assert all(torch.equal(a, b) for a, b in zip(before, ac.memory_c.hidden_states))
        state["obs_dict"] = obs_dict
        st = alg.storage
        assert isinstance(ac.memory_a.hidden_states, tuple) and len(st.saved_hidden_states_a) == 2
        assert st.saved_hidden_states_a[0].shape == (T, layers, n, H)
        for k in OP.RefStorage.FIELDS:
            getattr(ref.storage, k).copy_(getattr(st, k).reshape(T, n, -1).cpu())
        ref.storage.dones.copy_(st.dones.reshape(T, n, 1).cpu())
        hid_a = tuple(h.cpu() for h in st.saved_hidden_states_a)
        hid_c = tuple(h.cpu() for h in st.saved_hidden_states_c)
        # every update starts from the oracle's weights / Adam states / learning rate: its first mini-batch is a 1e-5 comparison
        ac.load_state_dict(_strip(ref.actor_critic.state_dict()))
        alg.optimizer.load_state_dict(_by_name(ref.optimizer.state_dict(), ref.actor_critic, ac))
        alg.vae_optimizer.load_state_dict(_by_name(ref.vae_optimizer.state_dict(), ref.actor_critic.vae, ac.vae))
        alg.learning_rate = ref.learning_rate
        alg.vae_optimizer.set_lr(5e-4)
        g = torch.Generator().manual_seed(300 + u)
        B = T * (n // NMB)
        e1, e2 = torch.randn(NMB, B, 16, generator=g), torch.randn(NMB, B, 16, generator=g)
        recs = [ref.step(bt, e1[i], e2[i]) for i, bt in enumerate(recurrent_slices(ref.storage, hid_a, hid_c, NMB))]
        out = alg.update(e1.to(DEV), e2.to(DEV))
        assert all(np.isfinite(out)), out
        rows = alg.last_update_stats
        assert rows.shape[0] == NMB
        for k, rec in enumerate(recs):
            for key, c in cols.items():
                refv = getattr(rec, key)
                worst.append((abs(float(rows[k, c]) - refv) / max(1.0, abs(refv)) / envelope[k], u, k, key, float(rows[k, c]), refv))
        assert abs(alg.learning_rate - ref.learning_rate) <= 1e-12, (u, alg.learning_rate, ref.learning_rate)
    assert max(w for w in worst if w[2] == 0)[0] <= 1.0, sorted((w for w in worst if w[2] == 0), reverse=True)[:4]
    assert max(worst)[0] <= 1.0, sorted(worst, reverse=True)[:6]
    # save / load: a fresh runner on the checkpoint acts as the trained one
    path = str(tmp_path / "model.pt")
    r.save(path)
    torch.manual_seed(12)
    r2 = OnPolicyRunner(ReplayEnv(n, DEV), cfg, log_dir=None, device=DEV)
    r2.load(path)
    ob = r.env.get_observations()
    ob = dict(obs=ob["obs"].to(DEV), obs_history=ob["obs_history"].to(DEV), privileged_obs=ob["privileged_obs"].to(DEV))
    p1, p2 = r.get_inference_policy(), r2.get_inference_policy()
    with torch.inference_mode():
        for m in (ac, r2.alg.actor_critic):
            m.reset()
        for _ in range(3):
            a1, a2 = p1(ob), p2(ob)
            assert torch.equal(a1, a2)


# ------------------------------------------------------------------------------------------ GPU: the default stays put
@pytest.mark.gpu
def test_explicit_gru_1_layer_equals_default_bitwise():
    """rnn_type='gru', rnn_num_layers=1 named explicitly and left at the defaults: one update gives identical parameters."""
    from dtc_amd.algorithms import RecurrentDecoderPPO
    from dtc_amd.modules import ActorCriticDecoderRecurrent
    n = 32
    d = S.rollout(n, T, seed=9, device=DEV)
    results = []
    for kw in (dict(), dict(rnn_type="gru", rnn_num_layers=1, rnn_hidden_size=512)):
        torch.manual_seed(3)
        ac = ActorCriticDecoderRecurrent(53, 1389, 12, **kw)
        alg = RecurrentDecoderPPO(ac, learning_rate=1e-3, entropy_coef=0.003, device=DEV, num_learning_epochs=1)
        alg.init_storage(n, T, [53], [1389], [265], [12])
        for t in range(T):
            alg.act(d["observations"][t], d["privileged_observations"][t], d["observation_histories"][t], d["base_vel"][t])
            alg.process_env_step(d["rewards"][t, :, 0], d["dones"][t, :, 0], d["next_observations"][t], {})
        alg.compute_returns(d["observations"][-1], d["privileged_observations"][-1], d["base_vel"][-1])
        g = torch.Generator().manual_seed(41)
        e1, e2 = torch.randn(NMB, T * (n // NMB), 16, generator=g), torch.randn(NMB, T * (n // NMB), 16, generator=g)
        alg.update(e1.to(DEV), e2.to(DEV))
        results.append({k: v.detach().cpu().clone() for k, v in ac.state_dict().items()})
    assert list(results[0]) == list(results[1])
    assert all(torch.equal(results[0][k], results[1][k]) for k in results[0])
