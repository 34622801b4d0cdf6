"""contain_nonfinite_envs (containment of non-finite rollout envs in the storage): the host side -- the keyword on all three trainers, the
declarations of include/dtc_hip.h and their binding, the by-value struct's size, argument rejection before any launch.  No GPU."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dtc_states_finite", "dtc_env_fold", "dtc_env_columns_cap", "dtc_env_columns_repair", "dtc_contain_envs_abi_sizes")


def test_keyword_is_keyword_only_and_off_by_default_on_all_three_trainers():
    from dtc_amd.algorithms import PPO, RecurrentDecoderPPO, RecurrentPPO
    for cls in (PPO, RecurrentPPO, RecurrentDecoderPPO):
        p = inspect.signature(cls.__init__).parameters["contain_nonfinite_envs"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False, cls
    # the row-level keyword keeps its meaning and its reach
    assert "contain_nonfinite" not in inspect.signature(RecurrentPPO.__init__).parameters
    assert inspect.signature(PPO.__init__).parameters["contain_nonfinite"].default is False


def test_flag_reaches_the_storage_and_both_flags_together_are_refused():
    from dtc_amd.algorithms import PPO, RecurrentDecoderPPO, RecurrentPPO
    from dtc_amd.modules import ActorCriticDecoder, ActorCriticDecoderRecurrent, ActorCriticRecurrent
    for flag in (False, True):
        algs = [PPO(ActorCriticDecoder(53, 1389, 12), device="cpu", contain_nonfinite_envs=flag),
                RecurrentDecoderPPO(ActorCriticDecoderRecurrent(53, 1389, 12), device="cpu", contain_nonfinite_envs=flag)]
        for alg in algs:
            alg.init_storage(4, 24, [53], [1389], [265], [12])
        algs.append(RecurrentPPO(ActorCriticRecurrent(53, 1389, 12), device="cpu", contain_nonfinite_envs=flag))
        algs[-1].init_storage(4, 24, [53], [1389], [12])
        for alg in algs:
            st = alg.storage
            assert alg.contain_nonfinite_envs is flag and st.contain_nonfinite_envs is flag and alg.last_nonfinite_envs == 0
            # nothing is allocated before a compute_returns with the flag on -- and nothing ever with it off
            assert st.env_valid is None and st.env_src is None and st.n_valid_envs is None and not st.env_record_fresh
            assert st.contain_nonfinite is False and st.row_valid is None
    with pytest.raises(ValueError, match="contain_nonfinite_envs"):
        PPO(ActorCriticDecoder(53, 1389, 12), device="cpu", contain_nonfinite=True, contain_nonfinite_envs=True)
    # the recurrent trainers still refuse the row-level keyword; the text now names the one they take
    with pytest.raises(TypeError, match="contain_nonfinite_envs=True"):
        RecurrentDecoderPPO(ActorCriticDecoderRecurrent(53, 1389, 12), device="cpu", contain_nonfinite=True)
    with pytest.raises(TypeError, match="contain_nonfinite"):
        RecurrentPPO(ActorCriticRecurrent(53, 1389, 12), device="cpu", contain_nonfinite=True)


def test_new_symbols_are_declared_bound_and_exported():
    from dtc_amd import _ffi
    header = open(os.path.join(ROOT, "include", "dtc_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _ffi.lib()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", code), f"{name} is not declared in include/dtc_hip.h"
        assert name in _ffi.exported_symbols() and hasattr(lib, name)
    assert "typedef struct DtcEnvColumn" in code
    assert int(re.search(r"#define DTC_ABI_VERSION (\d+)", header).group(1)) == _ffi.ABI_VERSION == lib.dtc_version() >= 20


def test_env_column_struct_size_matches_the_librarys():
    from dtc_amd import _ffi
    lib = _ffi.lib()
    sizes = (C.c_int64 * 8)()
    assert lib.dtc_contain_envs_abi_sizes(sizes, 8) == 1 and sizes[0] == C.sizeof(_ffi.DtcEnvColumn) == 40
    assert [n for n, _ in _ffi.DtcEnvColumn._fields_] == ["base", "outer", "outer_stride_bytes", "env_stride_bytes", "width_bytes"]
    # the older structs' table keeps its entries
    assert lib.dtc_abi_sizes(sizes, 0) == 18


def _column(buf, outer=2, outer_stride=64, env_stride=16, width=16):
    c = _ffi_mod().DtcEnvColumn()
    c.base, c.outer, c.outer_stride_bytes, c.env_stride_bytes, c.width_bytes = buf, outer, outer_stride, env_stride, width
    return c


def _ffi_mod():
    from dtc_amd import _ffi
    return _ffi


def test_bad_arguments_are_rejected_before_any_launch():
    """every call fails validation in front of the first HIP call: runs without a GPU"""
    _ffi = _ffi_mod()
    lib = _ffi.lib()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p).value

    def err(rc, needle):
        assert rc == -1, rc
        assert needle.encode() in lib.dtc_last_error(), (needle, lib.dtc_last_error())

    err(lib.dtc_states_finite(None, 2, 1, 4, 8, p, None), "null")
    err(lib.dtc_states_finite(p, 2, 1, 4, 8, None, None), "null")
    err(lib.dtc_states_finite(p, 2, 1, 4, 0, p, None), "bad shape")
    err(lib.dtc_states_finite(p, 2, 0, 4, 8, p, None), "bad shape")
    err(lib.dtc_states_finite(p + 1, 2, 1, 4, 8, p, None), "aligned")
    err(lib.dtc_env_fold(None, 2, 4, p, None), "null")
    err(lib.dtc_env_fold(p, 2, 4, None, None), "null")
    err(lib.dtc_env_fold(p, 0, 4, p, None), "bad shape")
    err(lib.dtc_env_fold(p, 2, 0, p, None), "bad shape")
    cap = lib.dtc_env_columns_cap()
    assert cap >= 20                                           # eleven scanned tensors, dones, four LSTM state tensors, last_values: 17
    items = (_ffi.DtcEnvColumn * (cap + 1))()
    for i in range(cap + 1):
        items[i] = _column(p)
    err(lib.dtc_env_columns_repair(items, 0, p, p, 4, None), "items")
    err(lib.dtc_env_columns_repair(items, cap + 1, p, p, 4, None), "items")
    err(lib.dtc_env_columns_repair(None, 1, p, p, 4, None), "null")
    err(lib.dtc_env_columns_repair(items, 1, None, p, 4, None), "null")
    err(lib.dtc_env_columns_repair(items, 1, p, None, 4, None), "null")
    err(lib.dtc_env_columns_repair(items, 1, p, p, 0, None), "env count")
    items[1] = _column(None)
    err(lib.dtc_env_columns_repair(items, 2, p, p, 4, None), "item 1 is a null pointer")
    items[1] = _column(p, width=0)
    err(lib.dtc_env_columns_repair(items, 2, p, p, 4, None), "width_bytes=0")
    items[1] = _column(p, width=-4)
    err(lib.dtc_env_columns_repair(items, 2, p, p, 4, None), "width_bytes=-4")
    items[1] = _column(p, outer=0)
    err(lib.dtc_env_columns_repair(items, 2, p, p, 4, None), "outer=0")
    items[1] = _column(p, env_stride=8)
    err(lib.dtc_env_columns_repair(items, 2, p, p, 4, None), "env_stride_bytes=8")


def test_runner_logs_the_env_count_when_and_only_when_the_trainer_contains():
    from dtc_amd.env import ReplayEnv
    from dtc_amd.runners import OnPolicyRunner
    runner = dict(policy_class_name="ActorCriticDecoderRecurrent", algorithm_class_name="RecurrentDecoderPPO", num_steps_per_env=24,
                  save_interval=10)
    for algo, want in ((dict(learning_rate=1e-3, contain_nonfinite_envs=True), True), (dict(learning_rate=1e-3), False)):
        r = OnPolicyRunner(ReplayEnv(8, "cpu"), dict(runner=runner, algorithm=algo, policy=dict()), log_dir=None, device="cpu")
        assert r.alg.contain_nonfinite_envs is want and r.alg.storage.contain_nonfinite_envs is want
        r.alg.last_nonfinite_envs = 3 if want else 0
        scalars = r.log(0, 1, (0.0,) * 7, collection_time=1.0, learn_time=1.0, tracker=None, finished=None)
        assert ("Train/nonfinite_envs" in scalars) is want and "Train/nonfinite_rows" not in scalars
        if want:
            assert scalars["Train/nonfinite_envs"] == 3
