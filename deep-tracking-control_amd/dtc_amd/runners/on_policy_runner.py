"""OnPolicyRunner with the reference's constructor / learn / save / load / get_inference_policy
(rsl_rl/rsl_rl/runners/on_policy_runner.py:45-273).  The rollout loop and the checkpoint dictionary
layout are kept; TensorBoard is optional (logging is not part of the hot path).

Under a process group (`distributed.data_parallel()`: one process per GPU, each with its own env shard -- INTEGRATION.md §4) rank 0 alone
creates the TensorBoard writer, prints the log block and writes checkpoints; the episode means, the loss means and the throughput it
logs are those of the whole job, gathered by ONE small all-reduce per iteration that every rank joins."""
import os
import time

import torch

from .. import distributed as dp
from ..algorithms import PPO, RecurrentDecoderPPO, RecurrentPPO
from ..env import HistoryWrapper
from ..modules import ActorCritic, ActorCriticDecoder, ActorCriticDecoderRecurrent, ActorCriticRecurrent  # resolved by name from train_cfg

try:                                       # not installed in every image
    from torch.utils.tensorboard import SummaryWriter
except Exception:                          # pragma: no cover
    SummaryWriter = None

# on_policy_runner.py:38-42, 60, 67 resolve the classes with eval(): the same names are reachable here.  `PPO` needs a
# model with a `.vae` (ppo.py:79) exactly as in the reference; the recurrent actor-critic of BASELINE configs[2] trains
# with `RecurrentPPO` (the upstream PPO step the fork dropped), the composite with `RecurrentDecoderPPO`.
_POLICIES = {"ActorCritic": ActorCritic, "ActorCriticRecurrent": ActorCriticRecurrent, "ActorCriticDecoder": ActorCriticDecoder,
             "ActorCriticDecoderRecurrent": ActorCriticDecoderRecurrent}
_ALGORITHMS = {"PPO": PPO, "RecurrentPPO": RecurrentPPO, "RecurrentDecoderPPO": RecurrentDecoderPPO}


_LOCAL = object()          # log(finished=...): take the means from the tracker


class _EpisodeTracker:
    """Return and length of the episode in flight per env; finished episodes go into a device-side ring of the most
    recent `keep` (the numbers the reference's logger averages) -- no host round trip per env step, one at log time."""

    def __init__(self, num_envs, device, keep=100):
        self.keep = keep
        self.ret = torch.zeros(num_envs, dtype=torch.float32, device=device)
        self.length = torch.zeros(num_envs, dtype=torch.float32, device=device)
        self.ring = torch.zeros(keep + 1, 2, dtype=torch.float32, device=device)     # slot `keep` absorbs the non-finished envs
        self.finished = torch.zeros((), dtype=torch.long, device=device)

    def step(self, rewards, dones):
        self.ret += rewards
        self.length += 1
        done = dones > 0
        order = torch.cumsum(done, 0) - 1                                   # 0, 1, ... among the envs finishing now
        slot = torch.where(done, (self.finished + order) % self.keep, torch.full_like(order, self.keep))
        self.ring[slot] = torch.stack((self.ret, self.length), dim=1)
        self.finished += done.sum()
        keep_going = (~done).to(self.ret.dtype)
        self.ret *= keep_going
        self.length *= keep_going

    def means(self):
        n = min(int(self.finished), self.keep)
        if n == 0:
            return None
        m = self.ring[:n].mean(dim=0)
        return float(m[0]), float(m[1])

    def sums(self):
        """float64 [3] on the device: sum of returns, sum of lengths and count over the ring entries `means()` averages -- what a rank
        contributes to the job's means; no host round trip."""
        n = self.finished.clamp(max=self.keep)
        live = (torch.arange(self.keep, device=self.ring.device) < n).to(torch.float64).unsqueeze(1)
        return torch.cat(((self.ring[:self.keep].double() * live).sum(dim=0), n.to(torch.float64).reshape(1)))


class OnPolicyRunner:
    def __init__(self, env, train_cfg, log_dir=None, device='cpu'):
        self.cfg = train_cfg["runner"]
        self.alg_cfg = train_cfg["algorithm"]
        self.policy_cfg = train_cfg["policy"]
        self.device = device
        self.env = HistoryWrapper(env)
        num_critic_obs = self.env.num_privileged_obs if self.env.num_privileged_obs is not None else self.env.num_obs
        actor_critic_class = _POLICIES[self.cfg["policy_class_name"]]
        actor_critic = actor_critic_class(self.env.num_obs, num_critic_obs, self.env.num_actions,
                                          **self.policy_cfg).to(self.device)
        alg_class = _ALGORITHMS[self.cfg["algorithm_class_name"]]
        self.alg = alg_class(actor_critic, device=self.device, **self.alg_cfg)
        self.num_steps_per_env = self.cfg["num_steps_per_env"]
        self.save_interval = self.cfg["save_interval"]
        # upstream-style trainers (actor obs / critic obs only) take no observation history, base velocity or reward buffer
        self._plain = isinstance(self.alg, RecurrentPPO)
        if self._plain:
            self.alg.init_storage(self.env.num_envs, self.num_steps_per_env, [self.env.num_obs], [num_critic_obs],
                                  [self.env.num_actions])
        else:
            self.alg.init_storage(self.env.num_envs, self.num_steps_per_env, [self.env.num_obs],
                                  [self.env.num_privileged_obs], [self.env.num_obs_history], [self.env.num_actions])
        self.log_dir = log_dir
        self.writer = None
        self.tracker = None                    # the _EpisodeTracker of the last learn() that logged
        self.tot_timesteps = 0
        self.tot_time = 0
        self.current_learning_iteration = 0
        self.env.reset()

    # ---------------------------------------------------------------- training loop
    def _observe(self, obs_dict):
        dev = self.device
        return obs_dict["obs"].to(dev), obs_dict["privileged_obs"].to(dev), obs_dict["obs_history"].to(dev)

    def _collect(self, state, tracker, ep_infos):
        """One rollout of `num_steps_per_env` env steps into the storage, then the bootstrap values / returns."""
        obs_dict, rew_buf = state["obs_dict"], state["rew_buf"]
        obs, priv, hist = self._observe(obs_dict)
        with torch.inference_mode():
            for _ in range(self.num_steps_per_env):
                actions = self.alg.act(obs, priv) if self._plain else self.alg.act(obs, priv, hist, obs_dict['base_vel'], rew_buf)
                obs_dict, rewards, dones, infos = self.env.step(actions)
                obs, priv, hist = self._observe(obs_dict)
                rewards, dones = rewards.to(self.device), dones.to(self.device)
                self.alg.process_env_step(rewards, dones, next_obs=obs_dict['obs'], infos=infos)
                if tracker is not None:
                    tracker.step(rewards, dones)
                    if 'episode' in infos:
                        # an env may hand out views of device scalars it rewrites at every reset (the surrogate env does): keep the
                        # values, as one stacked tensor per step (one launch when every entry is a device scalar)
                        ep = infos['episode']
                        vals = [torch.as_tensor(v, dtype=torch.float32, device=self.device) for v in ep.values()]
                        ep_infos.append((tuple(ep), torch.stack([v if v.dim() == 0 else v.mean() for v in vals])))
            if self._plain:
                self.alg.compute_returns(priv)
            else:
                self.alg.compute_returns(obs, priv, obs_dict['base_vel'])
        state["obs_dict"] = obs_dict

    def learn(self, num_learning_iterations, init_at_random_ep_len=False):
        logging = self.log_dir is not None
        dpj = dp.data_parallel()
        if dpj:
            # one small collective settles on every rank alike whether anyone logs: then every rank keeps a tracker and joins the
            # per-iteration all-reduce of _job_means, or none does.  Files are rank 0's business alone, whatever log_dir the others got
            wanted = torch.tensor([float(logging)], dtype=torch.float64, device=self.device)
            tracking = float(dp.allreduce_sum_(wanted)) > 0
            logging = logging and dp.rank() == 0
        else:
            tracking = logging
        if logging and self.writer is None and SummaryWriter is not None:
            self.writer = SummaryWriter(log_dir=self.log_dir, flush_secs=10)
        if init_at_random_ep_len:
            self.env.episode_length_buf = torch.randint_like(self.env.episode_length_buf,
                                                             high=int(self.env.max_episode_length))
        if self._contains_act():
            # uint8 [N] on the device, rewritten by every act(): the env (the wrapped one, not the history wrapper) ORs it into its reset
            # buffer
            self.env.env.nonfinite_act_envs = self.alg.nonfinite_act_envs
        self.alg.actor_critic.train()
        state = dict(obs_dict=self.env.get_observations(), rew_buf=self.env.get_reward_buf())
        tracker = self.tracker = _EpisodeTracker(self.env.num_envs, self.device) if tracking else None
        ep_infos = []
        first, last = self.current_learning_iteration, self.current_learning_iteration + num_learning_iterations
        for it in range(first, last):
            t0 = time.time()
            self._collect(state, tracker, ep_infos)
            t1 = time.time()
            losses = self.alg.update()           # (value, surrogate, adaptation, decoder, recons, vel, kld) means
            t2 = time.time()
            finished, self._job_nonfinite, self._job_nonfinite_envs, self._job_nonfinite_act = _LOCAL, None, None, None
            if dpj and tracking:
                losses, finished = self._job_means(losses, tracker)
            if logging:
                self.log(it, last, losses, collection_time=t1 - t0, learn_time=t2 - t1, tracker=tracker, finished=finished, ep_infos=ep_infos)
                if it % self.save_interval == 0:
                    self.save(os.path.join(self.log_dir, f'model_{it}.pt'))
            ep_infos.clear()
        self.current_learning_iteration = last
        if logging:
            self.save(os.path.join(self.log_dir, f'model_{last}.pt'))

    def _job_means(self, losses, tracker):
        """Data parallel: ONE all-reduce (sum) of a float64 device tensor per iteration, joined by every rank -- the tracker's local sum of
        returns, sum of lengths and count, and the seven loss means of update() -> (loss means of the job, (mean reward, mean episode
        length) over the finished episodes of ALL ranks or None)."""
        local = tuple(float(x) for x in losses) + (0.0,) * (7 - len(losses))
        if self._contains():
            local += (float(self.alg.last_nonfinite_rows),)     # the job's SUM of invalid rows rides in the same all-reduce
        envs_at = 3 + len(local)                                # (position in `total`, behind the tracker's three sums)
        if self._contains_envs():
            local += (float(self.alg.last_nonfinite_envs),)     # ... and the job's sum of repaired envs, behind every entry above
        act_at = 3 + len(local)
        if self._contains_act():
            local += (float(self.alg.last_nonfinite_act),)      # ... and of repaired rollout steps, behind those
        local = torch.tensor(local, dtype=torch.float64, device=self.device)
        total = dp.allreduce_sum_(torch.cat((tracker.sums(), local))).tolist()
        count = total[2]
        finished = (total[0] / count, total[1] / count) if count > 0 else None
        if self._contains():
            self._job_nonfinite = int(total[10])
        if self._contains_envs():
            self._job_nonfinite_envs = int(total[envs_at])
        if self._contains_act():
            self._job_nonfinite_act = int(total[act_at])
        return tuple(x / dp.world_size() for x in total[3:10]), finished

    def _contains(self):
        return bool(getattr(self.alg, "contain_nonfinite", False))

    def _contains_envs(self):
        return bool(getattr(self.alg, "contain_nonfinite_envs", False))

    def _contains_act(self):
        return bool(getattr(self.alg, "contain_nonfinite_act", False))

    def log(self, it, last, losses, collection_time, learn_time, tracker, width=80, pad=35, finished=_LOCAL, ep_infos=None):
        """Writes and prints the scalars of iteration `it` and returns them.  `finished`: the (mean reward, mean episode length) to log
        instead of the tracker's own (data parallel: the job's, _job_means); throughput counts the envs of every rank.  `ep_infos`: one
        (keys, stacked values) pair per step of the rollout, from extras["episode"]; the mean of every entry over the steps is logged as
        'Episode/<key>', as the reference's runner does (on_policy_runner.py:171-182), with one host read for all of them."""
        value_loss, surrogate_loss, _adaptation, _decoder, recons_loss, vel_loss, kld_loss = tuple(losses) + (0.0,) * (7 - len(losses))
        steps = self.num_steps_per_env * self.env.num_envs * dp.world_size()
        self.tot_timesteps += steps
        self.tot_time += collection_time + learn_time
        scalars = {
            'Loss/value_function': value_loss, 'Loss/surrogate': surrogate_loss, 'Loss/recons_loss': recons_loss,
            'Loss/vel_loss': vel_loss, 'Loss/kld_loss': kld_loss, 'Loss/learning_rate': self.alg.learning_rate,
            'Policy/mean_noise_std': float(self.alg.actor_critic.std.mean()),
            'Perf/total_fps': int(steps / (collection_time + learn_time)),
            'Perf/collection time': collection_time, 'Perf/learning_time': learn_time}
        if finished is _LOCAL:
            finished = tracker.means()
        if finished is not None:
            scalars['Train/mean_reward'], scalars['Train/mean_episode_length'] = finished
        if self._contains():
            # rows of the last update that were not finite and stayed out of it (data parallel: the job's sum, _job_means)
            job = getattr(self, "_job_nonfinite", None)
            scalars['Train/nonfinite_rows'] = self.alg.last_nonfinite_rows if job is None else job
        if self._contains_envs():
            # envs of the last rollout that held something non-finite and were overwritten by valid ones (data parallel: the job's sum)
            job = getattr(self, "_job_nonfinite_envs", None)
            scalars['Train/nonfinite_envs'] = self.alg.last_nonfinite_envs if job is None else job
        if self._contains_act():
            # (step, env) pairs of the last rollout that act() repaired: zero actions, cleared live state (data parallel: the job's sum)
            job = getattr(self, "_job_nonfinite_act", None)
            scalars['Train/nonfinite_act'] = self.alg.last_nonfinite_act if job is None else job
        if ep_infos:
            keys = ep_infos[0][0]
            for k, v in zip(keys, torch.stack([row for names, row in ep_infos if names == keys]).mean(dim=0).tolist()):
                scalars['Episode/' + k] = v
        if self.writer is not None:
            for k, v in scalars.items():
                self.writer.add_scalar(k, v, it)
        lines = [f" Learning iteration {it}/{last} ".center(width, ' ')]
        lines += [f"{k + ':':>{pad}} {v:.4f}" for k, v in scalars.items()]
        print("#" * width + "\n" + "\n".join(lines))
        return scalars

    def save(self, path, infos=None):
        torch.save({'model_state_dict': self.alg.actor_critic.state_dict(),
                    'optimizer_state_dict': self.alg.optimizer.state_dict(),
                    'iter': self.current_learning_iteration, 'infos': infos}, path)

    def load(self, path, load_optimizer=True):
        loaded_dict = torch.load(path, map_location="cpu")
        self.alg.actor_critic.load_state_dict(loaded_dict['model_state_dict'])
        if load_optimizer:
            self.alg.optimizer.load_state_dict(loaded_dict['optimizer_state_dict'])
            self.alg.learning_rate = self.alg.optimizer.param_groups[0]['lr']
        self.current_learning_iteration = loaded_dict['iter']
        return loaded_dict['infos']

    def get_inference_policy(self, env_t=None, device=None):
        self.alg.actor_critic.eval()
        if device is not None:
            self.alg.actor_critic.to(device)
        if env_t == True:                      # noqa: E712  (on_policy_runner.py:269-272)
            return self.alg.actor_critic.act_expert
        return self.alg.actor_critic.act_inference
