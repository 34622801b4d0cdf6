"""32768 envs x 24 steps on one device: the rollout storage's privileged observations are a 4.37 GB tensor, past 2^31 and past 2^32
bytes.  The trainers' default path (operand images) reads it through the 64-bit pack and loss-target kernels
(tests/test_hip_wide_sources.py); here the trainers themselves run on such a storage.

Every optimisation step is compared bit for bit with the same step on a compact twin storage that holds the mini-batch's rows only
(below 2 GiB: the kernels every other trainer test runs): a mini-batch step is a function of the selected rows, the parameters and
the noise, not of where the rows lie.  The big storage is built once per module, on the device, and no test writes to it."""
import numpy as np
import pytest
import torch

from dtc_amd import synthetic as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_BIG, T = 32768, 24
SHAPES = ([53], [1389], [265], [12])


@pytest.fixture(scope="module")
def big():
    """The filled RolloutStorage(32768, 24) with returns and advantages, and saved recurrent states for the composite model."""
    from dtc_amd.storage.rollout_storage import RolloutStorage
    d = S.rollout(N_BIG, T, seed=4, device=DEV)
    st = RolloutStorage(N_BIG, T, *SHAPES, DEV)
    for k in list(d):
        if k != "last_values":
            getattr(st, k).copy_(d.pop(k))
    st.compute_returns(d["last_values"], 0.99, 0.95)
    g = torch.Generator(device=DEV).manual_seed(77)
    st.saved_hidden_states_a = [0.1 * torch.randn(T, 1, N_BIG, 512, generator=g, device=DEV)]
    st.saved_hidden_states_c = [0.1 * torch.randn(T, 1, N_BIG, 512, generator=g, device=DEV)]
    assert st.privileged_observations.numel() * 4 > 1 << 32
    yield st
    del st


def _twin(big, rows, n_envs):
    """RolloutStorage(n_envs, 24) whose flat rows are rows `rows` of the big storage, in that order."""
    from dtc_amd.algorithms import PPO
    from dtc_amd.storage.rollout_storage import RolloutStorage
    st = RolloutStorage(n_envs, T, *SHAPES, DEV)
    for k in PPO._FLAT_NAMES:
        st.flat(k).copy_(big.flat(k)[rows])
    return st


def _ppo(storage):
    from dtc_amd.algorithms import PPO
    from dtc_amd.modules import ActorCriticDecoder
    torch.manual_seed(3)
    alg = PPO(ActorCriticDecoder(53, 1389, 12), learning_rate=1e-3, entropy_coef=0.003, device=DEV)
    alg.storage = storage
    return alg


def _assert_same_step(a, b, out_a, out_b, moments=True):
    (row_a, lr_a), (row_b, lr_b) = out_a, out_b
    for (k, v), (_, w) in zip(a.actor_critic.state_dict().items(), b.actor_critic.state_dict().items()):
        assert torch.equal(v, w), k
    if moments:
        for name in ("optimizer", "vae_optimizer"):
            for m in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(getattr(getattr(a, name), m), getattr(getattr(b, name), m)), (name, m)
    assert torch.equal(row_a, row_b), (row_a, row_b)
    assert lr_a == lr_b
    assert bool(torch.isfinite(row_a).all())


def _small_index_list():
    """1536 rows: the rows that straddle 2^31 and 2^32 bytes of the privileged tensor (386 516, 773 032) with their neighbours, the
    first and the last row, and equal shares of seeded random rows of the three ranges those borders cut, shuffled."""
    g = torch.Generator().manual_seed(2031)
    special = [0, 386515, 386516, 386517, 773031, 773032, 773033, N_BIG * T - 1]
    parts = [torch.tensor(special)]
    for lo, hi in ((0, 386516), (386516, 773032), (773032, N_BIG * T)):
        parts.append(lo + torch.randperm(hi - lo, generator=g)[:-(-(1536 - len(special)) // 3)])
    rows = torch.cat(parts)[:1536]
    return rows[torch.randperm(1536, generator=g)].contiguous()


def test_ppo_minibatch_step_on_rows_across_2_gib_and_4_gib_equals_the_step_on_a_compact_storage(big):
    """B = 1536: the straddling rows, the first and the last row of the rollout and random rows of all three ranges."""
    idx = _small_index_list().to(DEV)
    g = torch.Generator().manual_seed(5)
    e1, e2 = torch.randn(idx.numel(), 16, generator=g), torch.randn(idx.numel(), 16, generator=g)
    wide, twin = _ppo(big), _ppo(_twin(big, idx, 64))
    twin.actor_critic.load_state_dict(wide.actor_critic.state_dict())
    out_w = wide.step_minibatch(idx, e1, e2, "both")
    out_t = twin.step_minibatch(torch.arange(idx.numel()), e1, e2, "both")
    _assert_same_step(wide, twin, out_w, out_t)
    init = _ppo(twin.storage).actor_critic.state_dict()
    assert any(not torch.equal(v, init[k]) for k, v in wide.actor_critic.state_dict().items())       # (the step stepped)


def test_ppo_minibatch_step_at_production_size(big):
    """B = 196 608 rows of a seeded permutation of all 786 432 -- a mini-batch of the 32768-env configuration, the largest in the
    suite -- against RolloutStorage(8192, 24) holding those rows (privileged observations of 1.09 GB: below 2 GiB)."""
    B = N_BIG * T // 4
    idx = torch.randperm(N_BIG * T, generator=torch.Generator().manual_seed(6))[:B].to(DEV)
    g = torch.Generator(device=DEV).manual_seed(7)
    e1, e2 = torch.randn(B, 16, generator=g, device=DEV), torch.randn(B, 16, generator=g, device=DEV)
    wide, twin = _ppo(big), _ppo(_twin(big, idx, B // T))
    twin.actor_critic.load_state_dict(wide.actor_critic.state_dict())
    out_w = wide.step_minibatch(idx, e1, e2, "both")
    out_t = twin.step_minibatch(torch.arange(B, device=DEV), e1, e2, "both")
    _assert_same_step(wide, twin, out_w, out_t)


def test_rollout_side_and_returns_at_32768_envs(big):
    """PPO.act + process_env_step into steps 11 and 23 of a 32768-env storage (their privileged rows lie across 2^31 and beyond 2^32
    bytes): the stored rows are the inputs.  Then compute_returns on the filled storage against oracle/gae.py, at the tolerances of
    tests/test_hip_kernels.py::test_gae_vs_oracle."""
    from dtc_amd.storage.rollout_storage import RolloutStorage
    from oracle import gae as OG
    alg = _ppo(RolloutStorage(N_BIG, T, *SHAPES, DEV))
    st = alg.storage
    g = torch.Generator(device=DEV).manual_seed(11)
    rn = lambda *s: torch.randn(*s, generator=g, device=DEV)
    for t in (11, 23):
        obs, priv, hist, vel, nxt = rn(N_BIG, 53), rn(N_BIG, 1389), rn(N_BIG, 265), rn(N_BIG, 3), rn(N_BIG, 53)
        rew, dones = rn(N_BIG), (torch.rand(N_BIG, generator=g, device=DEV) < 0.02).to(torch.uint8)
        st.step = t
        actions = alg.act(obs, priv, hist, vel).clone()
        alg.process_env_step(rew, dones, nxt, {})
        assert st.step == t + 1
        for name, want in (("observations", obs), ("privileged_observations", priv), ("observation_histories", hist), ("base_vel", vel),
                           ("next_observations", nxt), ("actions", actions), ("rewards", rew.view(-1, 1)), ("dones", dones.view(-1, 1))):
            assert torch.equal(getattr(st, name)[t], want), (t, name)
        assert bool(torch.isfinite(st.values[t]).all()) and float(st.values[t].abs().max()) > 0.0
        for nb in (t - 1, t + 1):                           # the neighbouring steps of the fresh storage are untouched
            assert nb >= T or float(st.privileged_observations[nb].abs().max()) == 0.0
    for k in ("rewards", "values", "dones"):
        getattr(st, k).copy_(getattr(big, k))
    last = (rn(N_BIG, 53), rn(N_BIG, 1389), rn(N_BIG, 3))
    last_values = alg.actor_critic.evaluate(*last).detach().clone()
    alg.compute_returns(*last)
    sq = lambda v: v.squeeze(-1).cpu().numpy()
    ret, adv = OG.compute_returns(sq(st.rewards), sq(st.values), sq(st.dones), sq(last_values))
    np.testing.assert_array_equal(sq(st.returns), ret)
    np.testing.assert_allclose(sq(st.advantages), adv, rtol=2e-6, atol=2e-6)


def test_composite_trainer_minibatch_on_the_last_quarter_of_32768_envs(big):
    """RecurrentDecoderPPO (1-layer GRU heads), the last of the four recurrent mini-batches of the 32768-env storage -- envs 24576 ..
    32767 at all 24 steps, seeded dones -- against the only mini-batch of an 8192-env storage holding those envs' data and saved
    states (the twin is built from plain slices of the storage; both descriptors come from recurrent_slices)."""
    from dtc_amd.algorithms import RecurrentDecoderPPO
    from dtc_amd.modules import ActorCriticDecoderRecurrent
    from dtc_amd.storage.rollout_storage import RolloutStorage
    n = N_BIG // 4
    small = RolloutStorage(n, T, *SHAPES, DEV)
    for k in ("observations", "next_observations", "privileged_observations", "observation_histories", "rewards", "actions", "dones",
              "actions_log_prob", "values", "returns", "advantages", "mu", "sigma", "base_vel"):
        getattr(small, k).copy_(getattr(big, k)[:, N_BIG - n:])
    small.saved_hidden_states_a = [h[:, :, N_BIG - n:].contiguous() for h in big.saved_hidden_states_a]
    small.saved_hidden_states_c = [h[:, :, N_BIG - n:].contiguous() for h in big.saved_hidden_states_c]
    algs = []
    for st, nmb in ((big, 4), (small, 1)):
        torch.manual_seed(3)
        alg = RecurrentDecoderPPO(ActorCriticDecoderRecurrent(53, 1389, 12), learning_rate=1e-3, entropy_coef=0.003, num_mini_batches=nmb,
                                  device=DEV)
        alg.storage = st
        algs.append(alg)
    wide, twin = algs
    twin.actor_critic.load_state_dict(wide.actor_critic.state_dict())
    bt_w, bt_t = list(wide.recurrent_slices())[3], list(twin.recurrent_slices())[0]
    assert (bt_w["a"], bt_w["b"]) == (N_BIG - n, N_BIG) and bt_w["R"] == bt_t["R"] > n and torch.equal(bt_w["unpad_idx"], bt_t["unpad_idx"])
    B = n * T
    g = torch.Generator(device=DEV).manual_seed(9)
    e1, e2 = torch.randn(B, 16, generator=g, device=DEV), torch.randn(B, 16, generator=g, device=DEV)
    row_w = wide.step_minibatch(bt_w, e1, e2, "both").cpu()
    row_t = twin.step_minibatch(bt_t, e1, e2, "both").cpu()
    _assert_same_step(wide, twin, (row_w, wide.optimizer.lr_dev.item()), (row_t, twin.optimizer.lr_dev.item()))
