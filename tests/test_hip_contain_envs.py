"""Kernels of contain_nonfinite_envs (csrc/contain_envs.hip) against numpy: the record over a saved hidden-state tensor, the fold of the
row record into an env record with the replacement sources (dtc_env_fold + dtc_compact_valid + dtc_perm_repair over the identity), and the
in-place repair of the storage's columns, compared byte for byte on whole tensors.  The references are restated here in numpy; the
reference project has no such function."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLT_MAX = float(np.finfo(np.float32).max)
POISONS = (float("nan"), float("inf"), float("-inf"))


# ------------------------------------------------------------------------------------------------ dtc_states_finite
def _states(T, L, N, H, offset=0, seed=0):
    """finite fp32 [T, L, N, H] with denormals, +-0 and +-FLT_MAX sprinkled in; `offset` floats off a 16-byte boundary"""
    g = np.random.default_rng(seed)
    s = g.standard_normal((T, L, N, H)).astype(np.float32)
    flat = s.reshape(-1)
    special = np.array([1e-45, -1e-45, 1e-39, 0.0, -0.0, FLT_MAX, -FLT_MAX], dtype=np.float32)
    where = g.integers(0, flat.size, size=min(flat.size, 2 * special.size))
    flat[where] = special[np.arange(where.size) % special.size]
    buf = torch.zeros(flat.size + 8, dtype=torch.float32, device=DEV)
    dev = buf[offset:offset + flat.size].view(T, L, N, H)
    dev.copy_(torch.from_numpy(s))
    assert dev.data_ptr() % 16 == (4 * offset) % 16 and dev.is_contiguous()
    return s, dev


def _positions(T, L, N, H):
    return sorted({(t, l, n, h) for t in (0, T - 1) for l in range(L) for n in (0, N - 1) for h in (0, H - 1)})


@pytest.mark.parametrize("offset", [0, 1, 3])
@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (3, 2, 5, 3), (2, 3, 9, 50), (4, 1, 67, 128)])
def test_states_finite_vs_numpy(shape, offset):
    from dtc_amd import ops
    T, L, N, H = shape
    host, dev = _states(T, L, N, H, offset)
    g = np.random.default_rng(1)
    before = (g.random(T * N) < 0.8).astype(np.uint8)                    # zeros already in the record survive
    if T * N > 1:
        before[0] = 1
    # all finite (denormals, +-0, +-FLT_MAX among them): the record does not move
    rec = torch.from_numpy(before).to(DEV)
    ops.states_finite(dev, rec)
    assert np.array_equal(rec.cpu().numpy(), before)
    k = 0
    for pos in _positions(T, L, N, H):
        for bad in POISONS:
            keep = float(dev[pos])
            dev[pos] = bad
            host[pos] = bad
            for init in (np.ones(T * N, dtype=np.uint8), before):
                rec = torch.from_numpy(init).to(DEV)
                ops.states_finite(dev, rec)
                want = init & np.isfinite(host).all(axis=(1, 3)).reshape(-1).astype(np.uint8)
                assert want[pos[0] * N + pos[2]] == 0 and int((init != want).sum()) <= 1
                assert np.array_equal(rec.cpu().numpy(), want), (shape, offset, pos, bad)
            dev[pos] = keep
            host[pos] = keep
            k += 1
    assert k == 3 * len(_positions(T, L, N, H))


def test_states_finite_several_poisons_and_layers_at_once():
    """more than one hit per 16-byte group, per row and per env; a row is cleared whichever layer holds the poison"""
    from dtc_amd import ops
    T, L, N, H = 5, 3, 70, 50
    host, dev = _states(T, L, N, H, offset=2, seed=3)
    g = np.random.default_rng(5)
    for _ in range(40):
        pos = tuple(int(g.integers(0, d)) for d in (T, L, N, H))
        host[pos] = POISONS[int(g.integers(0, 3))]
    host[2, 1, 7, 8:12] = np.nan
    host[4, 2, 69, 46:50] = np.inf
    dev.copy_(torch.from_numpy(host))
    rec = torch.ones(T * N, dtype=torch.uint8, device=DEV)
    ops.states_finite(dev, rec)
    want = np.isfinite(host).all(axis=(1, 3)).reshape(-1)
    assert 20 <= int((~want).sum()) <= 42
    assert np.array_equal(rec.cpu().numpy().astype(bool), want)


# ------------------------------------------------------------------------------------------------ fold + sources
def _sources_numpy(env_valid):
    """the replacement rule: env_src[n] = n where env n is valid, else valid_list[n % n_valid]; no valid env: the identity"""
    N = env_valid.size
    valid_list = np.nonzero(env_valid)[0].astype(np.int64)
    src = np.arange(N, dtype=np.int64)
    if valid_list.size:
        bad = np.nonzero(env_valid == 0)[0]
        src[bad] = valid_list[bad % valid_list.size]
    return valid_list, src


def _patterns(N):
    every_other = np.arange(N) % 2 == 1
    all_but_one = np.ones(N, dtype=bool)
    all_but_one[N // 2] = False
    one = lambda n: np.arange(N) == n
    return dict(none=np.zeros(N, dtype=bool), first=one(0), last=one(N - 1), every_other=every_other, all_but_one=all_but_one,
                all=np.ones(N, dtype=bool))


def _fold_and_sources(row_valid, T, N):
    from dtc_amd import ops
    rec = torch.from_numpy(row_valid.reshape(-1)).to(DEV)
    env_valid = ops.env_fold(rec, T, N)
    valid_list, n_valid = ops.compact_valid(env_valid)
    env_src = ops.perm_repair(torch.arange(N, dtype=torch.int64, device=DEV), env_valid, valid_list, n_valid)
    return env_valid.cpu().numpy(), valid_list.cpu().numpy(), int(n_valid), env_src.cpu().numpy()


@pytest.mark.parametrize("N", [1, 5, 64, 67, 1000])
def test_fold_and_sources_vs_numpy(N):
    for T in (1, 4, 24):
        for name, invalid in _patterns(N).items():
            row_valid = np.ones((T, N), dtype=np.uint8)
            for n in np.nonzero(invalid)[0]:
                row_valid[(3 * n + 1) % T, n] = 0                       # one bad step somewhere in the env's column ...
                if n % 3 == 0:
                    row_valid[:, n] = 0                                 # ... or all of them
            env_valid, valid_list, n_valid, env_src = _fold_and_sources(row_valid, T, N)
            want_valid = row_valid.all(axis=0).astype(np.uint8)
            assert np.array_equal(want_valid == 0, invalid)
            want_list, want_src = _sources_numpy(want_valid)
            assert np.array_equal(env_valid, want_valid), (N, T, name)
            assert n_valid == want_list.size == N - int(invalid.sum()), (N, T, name)
            assert np.array_equal(valid_list[:n_valid], want_list), (N, T, name)
            assert np.array_equal(env_src, want_src), (N, T, name)
            if n_valid:
                assert want_valid[env_src].all()                        # every source is a valid env
            else:
                assert np.array_equal(env_src, np.arange(N))


# ------------------------------------------------------------------------------------------------ dtc_env_columns_repair
T_R = 4


def _item_mix(N, seed=0):
    """the per-env buffers of one call: (kind, host array).  kind: "steps" [T, N, w], "states" [T, L, N, H], "env" [N, w]"""
    g = np.random.default_rng(seed)
    f = lambda *s: g.standard_normal(s).astype(np.float32)
    return [("steps", f(T_R, N, 1)), ("steps", f(T_R, N, 3)), ("steps", f(T_R, N, 53)), ("steps", f(T_R, N, 1389)),
            ("steps", (g.random((T_R, N, 1)) < 0.3).astype(np.uint8)), ("states", f(T_R, 2, N, 3)), ("states", f(T_R, 1, N, 128)),
            ("env", f(N, 1))]


def _env_axis(kind):
    return {"steps": 1, "states": 2, "env": 0}[kind]


def _poison(kind, a, invalid):
    a = np.moveaxis(a.copy(), _env_axis(kind), 0)
    a[invalid] = 255 if a.dtype == np.uint8 else np.nan
    return np.ascontiguousarray(np.moveaxis(a, 0, _env_axis(kind)))


def _repaired_numpy(kind, a, src):
    return np.ascontiguousarray(np.take(a, src, axis=_env_axis(kind)))


def _repair(items, env_valid, env_src):
    from dtc_amd import ops
    dev = [torch.from_numpy(a).to(DEV) for _, a in items]
    cols, count = ops.env_columns([t if kind == "steps" else (t, kind) for (kind, _), t in zip(items, dev)], env_valid.size)
    ops.env_columns_repair(cols, count, torch.from_numpy(env_valid).to(DEV), torch.from_numpy(env_src).to(DEV))
    return [t.cpu().numpy() for t in dev]


@pytest.mark.parametrize("pattern", ["none", "first", "last", "every_other", "all_but_one", "all"])
@pytest.mark.parametrize("N", [5, 67])
def test_columns_repair_vs_numpy_byte_for_byte(N, pattern):
    invalid = _patterns(N)[pattern]
    env_valid = (~invalid).astype(np.uint8)
    _list, env_src = _sources_numpy(env_valid)
    clean = _item_mix(N)
    dirty = [(kind, _poison(kind, a, invalid)) for kind, a in clean]
    got = _repair(dirty, env_valid, env_src)
    for (kind, a), (_, d), out in zip(clean, dirty, got):
        want = _repaired_numpy(kind, d, env_src)
        assert out.dtype == a.dtype and out.shape == a.shape
        assert np.array_equal(out.view(np.uint8), want.view(np.uint8)), (kind, a.shape, pattern)
        if pattern == "all":
            assert np.array_equal(out.view(np.uint8), d.view(np.uint8))                 # nothing to repair from: nothing is touched
            continue
        # valid envs keep their bits, repaired envs hold their source's, and nothing non-finite is left
        keep = np.moveaxis(out, _env_axis(kind), 0)[~invalid]
        assert np.array_equal(keep.view(np.uint8), np.moveaxis(a, _env_axis(kind), 0)[~invalid].view(np.uint8))
        assert np.array_equal(out.view(np.uint8), _repaired_numpy(kind, a, env_src).view(np.uint8))
        if a.dtype == np.float32:
            assert np.isfinite(out).all()
        else:
            assert out.max() <= 1
        if pattern == "none":
            assert np.array_equal(out.view(np.uint8), a.view(np.uint8))


def test_columns_repair_off_the_16_byte_grid():
    """a 512-byte row whose base is 4 bytes off a 16-byte boundary, and a 1-byte-wide item at an odd address: the narrower accesses"""
    from dtc_amd import ops
    N = 67
    invalid = _patterns(N)["every_other"]
    env_valid = (~invalid).astype(np.uint8)
    _list, env_src = _sources_numpy(env_valid)
    g = np.random.default_rng(2)
    a = g.standard_normal((T_R, 1, N, 128)).astype(np.float32)
    b = g.integers(0, 200, size=(T_R, N, 3)).astype(np.uint8)
    da, db = _poison("states", a, invalid), _poison("steps", b, invalid)
    buf_a = torch.zeros(a.size + 4, dtype=torch.float32, device=DEV)
    buf_b = torch.zeros(b.size + 4, dtype=torch.uint8, device=DEV)
    ta, tb = buf_a[1:1 + a.size].view(a.shape), buf_b[1:1 + b.size].view(b.shape)
    ta.copy_(torch.from_numpy(da))
    tb.copy_(torch.from_numpy(db))
    assert ta.data_ptr() % 16 == 4 and tb.data_ptr() % 2 == 1
    cols, count = ops.env_columns([(ta, "states"), tb], N)
    ops.env_columns_repair(cols, count, torch.from_numpy(env_valid).to(DEV), torch.from_numpy(env_src).to(DEV))
    assert np.array_equal(ta.cpu().numpy().view(np.uint8), _repaired_numpy("states", a, env_src).view(np.uint8))
    assert np.array_equal(tb.cpu().numpy(), _repaired_numpy("steps", b, env_src))
    assert float(buf_a[0]) == 0.0 and float(buf_a[-3:].abs().sum()) == 0.0 and int(buf_b[0]) == 0 and int(buf_b[-3:].sum()) == 0


def test_columns_repair_with_many_invalid_envs_over_several_chunks():
    """more envs than one chunk of the kernel's env walk (2048), invalid envs in every chunk and a chunk without any"""
    N = 5000
    invalid = np.zeros(N, dtype=bool)
    invalid[[0, 1, 2047, 2048, 2049, 4999]] = True
    invalid[4100:4400:3] = True
    env_valid = (~invalid).astype(np.uint8)
    _list, env_src = _sources_numpy(env_valid)
    g = np.random.default_rng(4)
    clean = [("steps", g.standard_normal((T_R, N, 53)).astype(np.float32)), ("states", g.standard_normal((T_R, 2, N, 4)).astype(np.float32)),
             ("env", g.standard_normal((N, 1)).astype(np.float32))]
    got = _repair([(kind, _poison(kind, a, invalid)) for kind, a in clean], env_valid, env_src)
    for (kind, a), out in zip(clean, got):
        assert np.array_equal(out.view(np.uint8), _repaired_numpy(kind, a, env_src).view(np.uint8)), kind


def test_columns_repair_beyond_4_gib():
    """fp32 [2, N, 4096] of more than 4 GiB with invalid envs at both ends: the byte offsets are 64-bit.  Compared: the touched columns
    and their neighbours."""
    from dtc_amd import ops
    N, W = 131073, 4096
    assert 2 * N * W * 4 > 4 * 2 ** 30
    x = torch.empty(2, N, W, dtype=torch.float32, device=DEV).normal_()
    invalid = np.zeros(N, dtype=bool)
    invalid[[0, N - 1]] = True
    env_valid = (~invalid).astype(np.uint8)
    _list, env_src = _sources_numpy(env_valid)
    assert env_src[0] == 1 and env_src[N - 1] == 2
    look = [0, 1, 2, 3, N // 2, N - 3, N - 2, N - 1]
    before = x[:, look].cpu().numpy()
    x[:, 0] = float("nan")
    x[:, N - 1] = float("nan")
    cols, count = ops.env_columns([x], N)
    ops.env_columns_repair(cols, count, torch.from_numpy(env_valid).to(DEV), torch.from_numpy(env_src).to(DEV))
    after = x[:, look].cpu().numpy()
    want = before.copy()
    want[:, 0], want[:, -1] = before[:, 1], before[:, 2]
    assert np.array_equal(after.view(np.uint8), want.view(np.uint8))
    assert bool(torch.isfinite(x[1]).all())                                # (the half behind 2 GiB as a whole)


def test_bad_arguments_are_rejected_with_no_launch():
    import test_contain_envs_host as H
    H.test_bad_arguments_are_rejected_before_any_launch()
    torch.cuda.synchronize()
