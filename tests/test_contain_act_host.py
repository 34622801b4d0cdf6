"""contain_nonfinite_act (containment of non-finite envs at the rollout step): the host side -- the declarations of include/dtc_hip.h and
their binding, the by-value struct's size, argument rejection before any launch, the keyword's rules on all three trainers and through
the runner, and the default path left as it was.  No GPU."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dtc_act_contain", "dtc_act_contain_cap", "dtc_act_contain_abi_sizes", "dtc_set_amax_finite_only", "dtc_get_amax_finite_only")


def _ffi_mod():
    from dtc_amd import _ffi
    return _ffi


def test_new_symbols_are_declared_bound_and_exported():
    _ffi = _ffi_mod()
    header = open(os.path.join(ROOT, "include", "dtc_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _ffi.lib()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", code), f"{name} is not declared in include/dtc_hip.h"
        assert name in _ffi.exported_symbols() and hasattr(lib, name)
    assert "typedef struct DtcActItem" in code
    assert int(re.search(r"#define DTC_ABI_VERSION (\d+)", header).group(1)) == _ffi.ABI_VERSION == lib.dtc_version() >= 21


def test_act_item_struct_size_matches_the_librarys_and_the_older_tables_keep_their_entries():
    _ffi = _ffi_mod()
    lib = _ffi.lib()
    sizes = (C.c_int64 * 8)()
    assert lib.dtc_act_contain_abi_sizes(sizes, 8) == 1 and sizes[0] == C.sizeof(_ffi.DtcActItem) == 40
    assert [n for n, _ in _ffi.DtcActItem._fields_] == ["base", "outer", "outer_stride_elems", "env_stride_elems", "width", "mode"]
    assert lib.dtc_abi_sizes(sizes, 0) == 18 and lib.dtc_contain_envs_abi_sizes(sizes, 0) == 1
    assert lib.dtc_act_contain_cap() >= 24                     # two 2-layer LSTMs (4 state tensors), actions and eight row tensors: 13


def test_finite_only_amax_is_off_by_default_and_on_inside_the_context_only():
    """the library switch behind ops.rows_to_themselves: host state only, no launch"""
    from dtc_amd import ops
    lib = _ffi_mod().lib()
    assert lib.dtc_get_amax_finite_only() == 0
    with ops.rows_to_themselves():
        assert lib.dtc_get_amax_finite_only() == 1
        with ops.rows_to_themselves():
            assert lib.dtc_get_amax_finite_only() == 1
        assert lib.dtc_get_amax_finite_only() == 1
    assert lib.dtc_get_amax_finite_only() == 0
    with pytest.raises(RuntimeError):
        with ops.rows_to_themselves():
            raise RuntimeError("a step that fails")
    assert lib.dtc_get_amax_finite_only() == 0


def _item(base, outer=1, outer_stride=0, env_stride=16, width=16, mode=0):
    it = _ffi_mod().DtcActItem()
    it.base, it.outer, it.outer_stride_elems, it.env_stride_elems, it.width, it.mode = base, outer, outer_stride, env_stride, width, mode
    return it


def test_bad_arguments_are_rejected_before_any_launch():
    """every call fails validation in front of the first HIP call: runs without a GPU.  The buffers are host memory filled with 7: a
    launch could not have written them, and no rejected call may have either"""
    _ffi = _ffi_mod()
    lib = _ffi.lib()
    buf = (C.c_float * 256)(*([7.0] * 256))
    out = (C.c_uint8 * 16)(*([7] * 16))
    p, o = C.cast(buf, C.c_void_p).value, C.cast(out, C.POINTER(C.c_uint8))
    cap = lib.dtc_act_contain_cap()
    items = (_ffi.DtcActItem * (cap + 1))()

    def fresh():
        for i in range(cap + 1):
            items[i] = _item(p, mode=i % 2)

    def err(rc, needle):
        assert rc == -1, rc                                    # DTC_ERR_ARG
        assert needle.encode() in lib.dtc_last_error(), (needle, lib.dtc_last_error())

    fresh()
    err(lib.dtc_act_contain(None, 1, 4, o, o, None), "items is a null pointer")
    err(lib.dtc_act_contain(items, 0, 4, o, o, None), "0 items")
    err(lib.dtc_act_contain(items, cap + 1, 4, o, o, None), f"{cap + 1} items")
    err(lib.dtc_act_contain(items, 2, 0, o, o, None), "env count N=0")
    err(lib.dtc_act_contain(items, 2, -3, o, o, None), "env count N=-3")
    err(lib.dtc_act_contain(items, 2, (1 << 31) + 1, o, o, None), "env count")
    for bad, needle in ((dict(base=None), "item 1 is a null pointer"), (dict(base=p + 2), "item 1 is not 4-byte aligned"),
                        (dict(base=p + 1), "item 1 is not 4-byte aligned"), (dict(base=p, width=0), "width=0"),
                        (dict(base=p, width=-4), "width=-4"), (dict(base=p, outer=0), "outer=0"), (dict(base=p, outer=-1), "outer=-1"),
                        (dict(base=p, env_stride=15), "env_stride_elems=15"),
                        (dict(base=p, outer=2, outer_stride=15), "outer_stride_elems=15"),
                        (dict(base=p, outer=2, outer_stride=0), "outer_stride_elems=0"),
                        (dict(base=p, mode=2), "mode=2"), (dict(base=p, mode=-1), "mode=-1")):
        fresh()
        items[1] = _item(**bad)
        err(lib.dtc_act_contain(items, 2, 4, o, o, None), needle)
    # outer == 1: the outer stride is not read, whatever it holds -- and only scan items with no output is nothing to do
    fresh()
    items[0], items[1] = _item(p, outer_stride=-5), _item(p)
    err(lib.dtc_act_contain(items, 2, 4, None, None, None), "nothing to do")
    assert all(v == 7.0 for v in buf) and all(v == 7 for v in out)


def test_keyword_is_keyword_only_and_off_by_default_on_all_three_trainers():
    from dtc_amd.algorithms import PPO, RecurrentDecoderPPO, RecurrentPPO
    for cls in (PPO, RecurrentPPO, RecurrentDecoderPPO):
        p = inspect.signature(cls.__init__).parameters["contain_nonfinite_act"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False, cls
        # the two containments of the update keep their defaults
        assert inspect.signature(cls.__init__).parameters["contain_nonfinite_envs"].default is False


def _trainers(**kw):
    """-> [(trainer with its storage, name)] for the three trainers on the CPU (construction and init_storage launch nothing)"""
    from dtc_amd.algorithms import PPO, RecurrentDecoderPPO, RecurrentPPO
    from dtc_amd.modules import ActorCriticDecoder, ActorCriticDecoderRecurrent, ActorCriticRecurrent
    algs = [PPO(ActorCriticDecoder(53, 1389, 12), device="cpu", **kw),
            RecurrentDecoderPPO(ActorCriticDecoderRecurrent(53, 1389, 12), device="cpu", **kw)]
    for alg in algs:
        alg.init_storage(4, 24, [53], [1389], [265], [12])
    algs.append(RecurrentPPO(ActorCriticRecurrent(53, 1389, 12), device="cpu", **kw))
    algs[-1].init_storage(4, 24, [53], [1389], [12])
    return algs


def test_the_flag_alone_is_refused_and_says_why():
    from dtc_amd.algorithms import PPO, RecurrentDecoderPPO, RecurrentPPO
    from dtc_amd.modules import ActorCriticDecoder, ActorCriticDecoderRecurrent, ActorCriticRecurrent
    for make in (lambda **kw: PPO(ActorCriticDecoder(53, 1389, 12), device="cpu", **kw),
                 lambda **kw: RecurrentDecoderPPO(ActorCriticDecoderRecurrent(53, 1389, 12), device="cpu", **kw),
                 lambda **kw: RecurrentPPO(ActorCriticRecurrent(53, 1389, 12), device="cpu", **kw)):
        with pytest.raises(ValueError, match="contain_nonfinite_envs=True") as e:
            make(contain_nonfinite_act=True)
        assert "recomputed" in str(e.value)
        make(contain_nonfinite_act=True, contain_nonfinite_envs=True)
    # the row-level containment carries it too, where it exists
    PPO(ActorCriticDecoder(53, 1389, 12), device="cpu", contain_nonfinite_act=True, contain_nonfinite=True)
    with pytest.raises(TypeError, match="contain_nonfinite"):
        RecurrentDecoderPPO(ActorCriticDecoderRecurrent(53, 1389, 12), device="cpu", contain_nonfinite_act=True, contain_nonfinite=True)


def test_flag_on_allocates_the_record_and_the_mask_and_flag_off_nothing(monkeypatch):
    import torch
    from dtc_amd import ops

    def never(*a, **k):
        raise AssertionError("ops.act_contain was reached")
    monkeypatch.setattr(ops, "act_contain", never)
    for alg in _trainers(contain_nonfinite_act=True, contain_nonfinite_envs=True):
        st = alg.storage
        assert alg.contain_nonfinite_act is True and alg.last_nonfinite_act == 0
        assert st.act_valid.dtype == torch.uint8 and st.act_valid.shape == (24, 4) and bool((st.act_valid == 1).all())
        assert alg.nonfinite_act_envs.dtype == torch.uint8 and alg.nonfinite_act_envs.shape == (4,) and not bool(alg.nonfinite_act_envs.any())
        st.act_valid[3, 2] = 0
        st.clear()                                             # a fill, no read-back
        assert bool((st.act_valid == 1).all()) and st.step == 0
    for alg in _trainers() + _trainers(contain_nonfinite_envs=True):
        st = alg.storage
        assert alg.contain_nonfinite_act is False and alg.last_nonfinite_act == 0
        assert st.act_valid is None and st.act_invalid is None and not hasattr(alg, "nonfinite_act_envs")
        st.clear()
        assert st.act_valid is None
        # the storage's records start from all ones: its present branch
        rows = torch.zeros(24 * 4, dtype=torch.uint8)
        assert st._start_record(rows) is rows and bool((rows == 1).all()) and st.act_invalid is None


def test_the_records_start_from_act_valid():
    """RolloutStorage._start_record with the flag on: a copy of act_valid, and the count of its zeros as a tensor (no host read)"""
    import torch
    alg = _trainers(contain_nonfinite_act=True, contain_nonfinite_envs=True)[0]
    st = alg.storage
    st.act_valid[5, 3] = 0
    st.act_valid[23, 0] = 0
    rows = torch.full((24 * 4,), 9, dtype=torch.uint8)
    st._start_record(rows)
    assert torch.equal(rows, st.act_valid.view(-1)) and rows[5 * 4 + 3] == 0 and int(rows.sum()) == 24 * 4 - 2
    assert torch.is_tensor(st.act_invalid) and st.act_invalid.dtype == torch.int64 and int(st.act_invalid) == 2


def test_ops_act_contain_never_copies():
    """tensors the kernel cannot take as they are raise ValueError in front of the library call (zeroing a copy would leave the
    caller's tensor as it was)"""
    import torch
    from dtc_amd import ops
    for bad in (dict(repair=[torch.zeros(4, 12)]),                                   # fp32, but not on the device
                dict(repair=[torch.zeros(4, 12, dtype=torch.float64)]), dict(scan=[torch.zeros(4, 12, dtype=torch.float16)]),
                dict(scan=[]), dict(scan=[object()])):
        with pytest.raises(ValueError, match="act_contain"):
            ops.act_contain(**bad)


def test_runner_passes_the_keyword_hands_the_mask_to_the_env_and_logs_the_count(monkeypatch):
    from dtc_amd import ops
    from dtc_amd.env import ReplayEnv
    from dtc_amd.runners import OnPolicyRunner

    def never(*a, **k):
        raise AssertionError("ops.act_contain was reached")
    monkeypatch.setattr(ops, "act_contain", never)
    runner = dict(policy_class_name="ActorCriticDecoderRecurrent", algorithm_class_name="RecurrentDecoderPPO", num_steps_per_env=24,
                  save_interval=10)
    cfg = lambda algo: dict(runner=runner, algorithm=algo, policy=dict())
    with pytest.raises(ValueError, match="contain_nonfinite_envs=True"):
        OnPolicyRunner(ReplayEnv(8, "cpu"), cfg(dict(learning_rate=1e-3, contain_nonfinite_act=True)), log_dir=None, device="cpu")
    for algo, want in ((dict(learning_rate=1e-3, contain_nonfinite_envs=True, contain_nonfinite_act=True), True),
                       (dict(learning_rate=1e-3, contain_nonfinite_envs=True), False), (dict(learning_rate=1e-3), False)):
        env = ReplayEnv(8, "cpu")
        r = OnPolicyRunner(env, cfg(algo), log_dir=None, device="cpu")
        assert r.alg.contain_nonfinite_act is want and (r.alg.storage.act_valid is not None) is want
        assert hasattr(r.alg, "nonfinite_act_envs") is want
        r.alg.last_nonfinite_act = 5 if want else 0
        scalars = r.log(0, 1, (0.0,) * 7, collection_time=1.0, learn_time=1.0, tracker=None, finished=None)
        assert ("Train/nonfinite_act" in scalars) is want and ("Train/nonfinite_envs" in scalars) is ("contain_nonfinite_envs" in algo)
        if want:
            assert scalars["Train/nonfinite_act"] == 5
        # learn() hands the mask to the env before its first step (zero iterations: no act(), no update())
        r.learn(0)
        assert hasattr(env, "nonfinite_act_envs") is want
        if want:
            assert env.nonfinite_act_envs is r.alg.nonfinite_act_envs
