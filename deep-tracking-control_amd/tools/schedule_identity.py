"""Bit identity of the update's kernel schedule across a host-side change of the trainers: for each configuration below, two consecutive
updates from seeded inputs, then three SHA-256 digests -- the trained parameters, the statistics tables (and learning-rate histories)
and the ordered list of dtc_amd.ops / dtc_amd.h2i layer entry points called, each with its bound arguments reduced to shapes, types and
plain values.  Run the SAME file on two checkouts and compare the lines: it touches the public surface only (constructors,
init_storage, act / process_env_step / compute_returns, dtc_amd.synthetic, update()).

    python tools/schedule_identity.py [--out FILE] [--only NAME ...]     every configuration, each in a fresh child process under its
                                                                         own time limit, one at a time; stops at the first failure
    python tools/schedule_identity.py --child NAME                       one configuration in this process; prints one JSON line
"""
import argparse
import hashlib
import inspect
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

DEV = "cuda:0"
T = 24
ENTRY_POINTS = dict(ops=("linear_fwd", "linear_dgrad", "linear_wgrad", "wgrad_group", "linear_fwd_mse"),
                    h2i=("linear_fwd", "linear_fwd_chain", "linear_dgrad", "linear_dgrad_chain", "linear_fwd_mse", "wgrad_group"))
# name -> (trainer, envs, trainer keywords, environment of the child, model keywords)
CONFIGS = {
    "default_64": ("ppo", 64, {}, {}, {}),
    "ragged_20": ("ppo", 20, dict(ragged_images=True), {}, {}),
    "onepass_64": ("ppo", 64, dict(gemm_passes=1), {}, {}),
    "onepass_ragged_20": ("ppo", 20, dict(gemm_passes=1, ragged_images=True), {}, {}),
    "contain_64_nan_row": ("ppo", 64, dict(contain_nonfinite=True), {}, {}),
    "h2i_off_64": ("ppo", 64, {}, dict(DTC_H2I="0"), {}),
    "chain_off_64": ("ppo", 64, {}, dict(DTC_H2I_CHAIN="0"), {}),
    "narrow_images_off_64": ("ppo", 64, {}, {}, {}),
    "recurrent_gru_64": ("recurrent", 64, {}, {}, {}),
    "recurrent_lstm_64": ("recurrent", 64, {}, {}, dict(rnn_type="lstm")),
}
CHILD_SECONDS = 240


def _describe(v):
    """A call argument as something that is the same in two runs that launch the same work: shapes, types and plain values, no addresses"""
    import torch
    from dtc_amd import _ffi, h2i
    if v is None or isinstance(v, (bool, int, float, str)):
        return repr(v)
    if isinstance(v, torch.Tensor):
        return ["T", list(v.shape), list(v.stride()), str(v.dtype)]
    if isinstance(v, h2i.HImage):
        return ["I", v.M, v.K]
    if isinstance(v, _ffi.DtcSegMat):
        return ["S", int(v.cols)]
    if isinstance(v, dict):
        return {k: _describe(v[k]) for k in sorted(v) if v[k] is not None}
    if isinstance(v, (list, tuple)):
        return [_describe(x) for x in v]
    return type(v).__name__


def _wrap(calls):
    from dtc_amd import h2i, ops
    for mod, names in ((ops, ENTRY_POINTS["ops"]), (h2i, ENTRY_POINTS["h2i"])):
        for name in names:
            inner = getattr(mod, name)
            sig = inspect.signature(inner)

            def outer(*a, _inner=inner, _sig=sig, _tag=f"{mod.__name__.split('.')[-1]}.{name}", **k):
                b = _sig.bind(*a, **k)
                b.apply_defaults()
                args = {p: (_describe(v) if p != "stream_ptr" else repr(v is None)) for p, v in b.arguments.items()}
                calls.append(json.dumps([_tag, args], sort_keys=True))
                return _inner(*a, **k)
            setattr(mod, name, outer)


def _sha(chunks):
    h = hashlib.sha256()
    for c in chunks:
        h.update(c if isinstance(c, bytes) else c.encode())
    return h.hexdigest()


def _bytes(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


def _child(name):
    import torch
    from dtc_amd import synthetic as S
    from dtc_amd.algorithms import PPO, RecurrentDecoderPPO
    from dtc_amd.modules import ActorCriticDecoder, ActorCriticDecoderRecurrent
    kind, n, kw, _, model_kw = CONFIGS[name]
    torch.manual_seed(3)
    if kind == "ppo":
        ac = ActorCriticDecoder(53, 1389, 12)
        alg = PPO(ac, learning_rate=1e-3, entropy_coef=0.003, device=DEV, **kw)
    else:
        ac = ActorCriticDecoderRecurrent(53, 1389, 12, **model_kw)
        alg = RecurrentDecoderPPO(ac, learning_rate=1e-3, entropy_coef=0.003, device=DEV, **kw)
    if name == "narrow_images_off_64":
        alg.narrow_images = False
    alg.init_storage(n, T, [53], [1389], [265], [12])
    calls, tables = [], []
    _wrap(calls)
    for u in range(2):
        d = S.rollout(n, T, seed=4 + u)
        perm, e1, e2 = S.update_noise(n, T, 4, 5, seed=123 + u)
        if kind == "ppo":
            for k, v in d.items():
                if k != "last_values":
                    getattr(alg.storage, k).copy_(v.to(DEV))
            if name == "contain_64_nan_row":
                alg.storage.observations[3 + u, 1, 7] = float("nan")
            alg.storage.compute_returns(d["last_values"].to(DEV), 0.99, 0.95)
            out, host, lrs = alg.update(perm=perm, eps1=e1.to(DEV), eps2=e2.to(DEV), return_stats=True)
            tables += [_bytes(host), _bytes(lrs)]
        else:
            d = {k: v.to(DEV) for k, v in d.items()}
            torch.manual_seed(50 + u)                      # act draws its sampling noise from torch's generator
            for t in range(T):
                alg.act(d["observations"][t], d["privileged_observations"][t], d["observation_histories"][t], d["base_vel"][t])
                alg.process_env_step(d["rewards"][t, :, 0], d["dones"][t, :, 0], d["next_observations"][t], {})
            alg.compute_returns(d["observations"][-1], d["privileged_observations"][-1], d["base_vel"][-1])
            out, host = alg.update(e1.to(DEV), e2.to(DEV), return_stats=True)
            tables.append(_bytes(host))
        tables.append(json.dumps([float(x) for x in out]) + repr(alg.learning_rate))
    torch.cuda.synchronize()
    params = [_bytes(p) for _, p in sorted(ac.named_parameters())]
    print(json.dumps(dict(config=name, params=_sha(params), stats=_sha(tables), calls=_sha(calls), n_calls=len(calls),
                          learning_rate=alg.learning_rate)), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--child")
    ap.add_argument("--only", nargs="*")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.child:
        return _child(a.child)
    rows = []
    for name in (a.only or CONFIGS):
        env = dict(os.environ, **CONFIGS[name][3])
        # a fresh child per configuration, one at a time, each under its own time limit; nothing more is started after a failure
        r = subprocess.run(["timeout", "-k", "10", str(CHILD_SECONDS), sys.executable, os.path.abspath(__file__), "--child", name],
                           env=env, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            print(f"{name}: exit status {r.returncode}; stopping", flush=True)
            return r.returncode
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        print(line, flush=True)
        rows.append(json.loads(line))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
