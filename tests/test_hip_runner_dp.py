"""OnPolicyRunner under a process group: rank 0 alone writes files and logs, and what it logs are the means and the throughput of the
whole job, gathered by one all-reduce per iteration.  Two gloo ranks on one device (the rehearsal form of the other data-parallel
tests; RCCL refuses two ranks on one device), one forced `nccl` rank, and no process group at all (the runner's plain code path)."""
import datetime
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_ENVS, STEPS = 32, 24
CFG = dict(runner=dict(policy_class_name="ActorCriticDecoder", algorithm_class_name="PPO", num_steps_per_env=STEPS, save_interval=1),
           algorithm=dict(learning_rate=1e-3), policy=dict())


def _learn(env_seed, model_seed, log_dir, iterations=2):
    """A runner on ReplayEnv(32, seed=env_seed) through learn(2) -> what the tests compare.  Per iteration: the scalars log() returned
    (ranks that log), the tracker's ring and finished count as they were when the iteration was logged, the loss means of update()."""
    from dtc_amd.env import ReplayEnv
    from dtc_amd.runners import OnPolicyRunner
    torch.manual_seed(model_seed)
    r = OnPolicyRunner(ReplayEnv(N_ENVS, DEV, seed=env_seed), CFG, log_dir=log_dir, device=DEV)
    scalars, rings, losses, means = [], [], [], []
    update, log = r.alg.update, r.log

    def spy_update():
        out = update()
        losses.append(tuple(out))
        if r.tracker is not None:
            rings.append((r.tracker.ring.cpu().clone(), int(r.tracker.finished)))
            means.append(r.tracker.means())
        return out

    def spy_log(*a, **k):
        scalars.append(log(*a, **k))
        return scalars[-1]
    r.alg.update, r.log = spy_update, spy_log
    r.learn(iterations)
    torch.cuda.synchronize()
    files = sorted(os.listdir(log_dir)) if log_dir is not None else []
    return r, dict(scalars=scalars, rings=rings, losses=losses, means=means, files=files, iteration=r.current_learning_iteration,
                   flat=r.alg.actor_critic.arena.flat.cpu().clone(), lr=r.alg.learning_rate)


def _worker(rank, world, port, out, backend, dirs):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    kw = dict(device_id=torch.device(DEV)) if backend == "nccl" else {}
    dist.init_process_group(backend, rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120), **kw)
    try:
        from dtc_amd import distributed as dp
        res = {}
        if world == 1:
            # the plain runner first, on the same env and model seeds, no files
            dp.trace_collectives(True)
            _, res["plain"] = _learn(0, 3, None)
            res["plain"]["log"] = dp.collective_log()
        with dp.force_data_parallel(world == 1):
            dp.trace_collectives(True)
            # every rank seeds its model differently: the rank-0 broadcast at the trainer's construction undoes it
            _, res["dp"] = _learn(rank, 3 + 17 * rank, dirs[rank])
            res["dp"]["log"] = dp.assert_same_collective_sequence()
        out[rank] = res
    finally:
        dist.destroy_process_group()


def _spawn(world, backend, dirs, limit=300):
    import test_hip_dp as D
    ctx = mp.get_context("spawn")
    out = ctx.Manager().dict()
    port = D._free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, out, backend, dirs)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(limit)
        assert p.exitcode == 0, f"rank exited with {p.exitcode}"
    return dict(out)


def _job_means(rings):
    """(mean reward, mean episode length, count) over the ring entries every rank's tracker would average, in float64."""
    total = torch.zeros(2, dtype=torch.float64)
    count = 0
    for ring, finished in rings:
        n = min(finished, ring.shape[0] - 1)
        total += ring[:n].double().sum(dim=0)
        count += n
    return float(total[0] / count), float(total[1] / count), count


def _close(a, b, rel=1e-6):
    return abs(a - b) <= rel * max(abs(a), abs(b))


def _check_throughput(s, envs):
    assert s["Perf/total_fps"] == int(STEPS * envs / (s["Perf/collection time"] + s["Perf/learning_time"]))


def test_two_ranks_rank0_logs_the_job_and_writes_alone(tmp_path):
    dirs = [str(tmp_path / f"rank{r}") for r in range(2)]
    for d in dirs:
        os.makedirs(d)
    out = _spawn(2, "gloo", dirs)
    a, b = out[0]["dp"], out[1]["dp"]
    assert {"model_0.pt", "model_1.pt", "model_2.pt"} <= set(a["files"])
    assert b["files"] == [] and b["scalars"] == []                     # rank 1 writes no file and logs nothing
    assert torch.equal(a["flat"], b["flat"]) and a["lr"] == b["lr"] and torch.isfinite(a["flat"]).all()
    assert a["iteration"] == b["iteration"] == 2
    assert len(a["scalars"]) == 2 and len(a["rings"]) == len(b["rings"]) == 2
    for it, s in enumerate(a["scalars"]):
        reward, length, count = _job_means([a["rings"][it], b["rings"][it]])
        assert count > 0 and a["rings"][it][1] > 0 and b["rings"][it][1] > 0       # both shards finished episodes: both enter the mean
        assert _close(s["Train/mean_reward"], reward) and _close(s["Train/mean_episode_length"], length), (it, s, reward, length)
        _check_throughput(s, 2 * N_ENVS)
        for key, col in (("Loss/value_function", 0), ("Loss/surrogate", 1), ("Loss/recons_loss", 4), ("Loss/vel_loss", 5), ("Loss/kld_loss", 6)):
            assert _close(s[key], 0.5 * (a["losses"][it][col] + b["losses"][it][col]), 1e-12), (it, key)
    assert a["log"] == b["log"]                                         # (also compared inside the workers, across the ranks)
    ops = [e[0] for e in a["log"]]
    # beside the trainer's collectives: one all-reduce that settles whether anyone logs and one [10] float64 all-reduce per iteration
    assert [e for e in a["log"] if e[0] == "all_reduce_sum" and e[2] == "float64" and e[1] == 10] == [("all_reduce_sum", 10, "float64", "default")] * 2
    assert ops.count("broadcast") == 1 and ops.count("all_reduce_sum") == 1 + 2 * (2 + 1)
    ck = torch.load(os.path.join(dirs[0], "model_2.pt"), map_location="cpu")
    assert ck["iter"] == 2 and set(ck) == {"model_state_dict", "optimizer_state_dict", "iter", "infos"}


def test_one_forced_rccl_rank_logs_what_the_plain_runner_computes(tmp_path):
    d = str(tmp_path / "rank0")
    os.makedirs(d)
    out = _spawn(1, "nccl", [d])[0]
    forced, plain = out["dp"], out["plain"]
    assert {"model_0.pt", "model_1.pt", "model_2.pt"} <= set(forced["files"])
    assert plain["log"] == [] and [e[0] for e in forced["log"]].count("all_reduce_mean") == 2 * 5 * 4 * 4
    assert len(forced["scalars"]) == 2
    for it, s in enumerate(forced["scalars"]):
        reward, length = forced["means"][it]                            # _EpisodeTracker.means() on the same ring
        assert _close(s["Train/mean_reward"], reward) and _close(s["Train/mean_episode_length"], length), (it, s, reward, length)
        _check_throughput(s, N_ENVS)
        assert _close(s["Loss/value_function"], forced["losses"][it][0], 1e-12)
    assert torch.equal(forced["flat"], plain["flat"]) and forced["lr"] == plain["lr"]
    assert torch.isfinite(forced["flat"]).all()


def test_without_a_process_group_the_runner_is_the_plain_runner(tmp_path, capsys):
    from dtc_amd import distributed as dp
    assert not dist.is_initialized()
    dp.trace_collectives(True)
    try:
        with dp.force_data_parallel(True):                              # no group: forcing changes nothing
            r, res = _learn(0, 3, str(tmp_path))
        assert dp.collective_log() == []
    finally:
        dp.trace_collectives(False)
    assert {"model_0.pt", "model_1.pt", "model_2.pt"} <= set(res["files"])
    assert capsys.readouterr().out.count("Learning iteration") == 2
    assert len(res["scalars"]) == 2 and r.tot_timesteps == 2 * STEPS * N_ENVS
    for it, s in enumerate(res["scalars"]):
        assert (s["Train/mean_reward"], s["Train/mean_episode_length"]) == res["means"][it]
        _check_throughput(s, N_ENVS)
        for key, col in (("Loss/value_function", 0), ("Loss/surrogate", 1), ("Loss/recons_loss", 4), ("Loss/vel_loss", 5), ("Loss/kld_loss", 6)):
            assert s[key] == res["losses"][it][col]
    ck = torch.load(os.path.join(str(tmp_path), "model_2.pt"), map_location="cpu")
    assert ck["iter"] == 2 and ck["infos"] is None
    for k, v in r.alg.actor_critic.state_dict().items():
        assert torch.equal(ck["model_state_dict"][k], v.cpu()), k
    want = r.alg.optimizer.state_dict()
    assert ck["optimizer_state_dict"]["param_groups"] == want["param_groups"]
    for i, st in want["state"].items():
        assert torch.equal(ck["optimizer_state_dict"]["state"][i]["exp_avg"], st["exp_avg"].cpu())
